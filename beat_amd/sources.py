"""
Point-source moment tensors on the host, with the reference's names (beat/sources.py:19-40, 372-400, 403-559): the
Tape & Tape (2015) Q-T parameterisation ``MTQTSource`` and its helpers, plus the double couple of Aki & Richards.

These are the one-source host forms (set-up, export, tests).  Populations of chains are evaluated on the device by
``csrc/polarity.hip`` (``beat_amd.polarity_binding.mt6_batch``), which restates the same chain of operations.
"""
import numpy as np

pi = np.pi
SQRT2, SQRT3, SQRT6 = np.sqrt(2.0), np.sqrt(3.0), np.sqrt(6.0)

N_MAPPING = 1000
BETA_MAPPING = np.linspace(0, pi, N_MAPPING)
U_MAPPING = (3.0 / 4.0 * BETA_MAPPING) - (1.0 / 2.0 * np.sin(2.0 * BETA_MAPPING)) + (1.0 / 16.0 * np.sin(4.0 * BETA_MAPPING))
LAMPBDA_FACTOR_MATRIX = np.array([[SQRT3, -1.0, SQRT2], [0.0, 2.0, SQRT2], [-SQRT3, -1.0, SQRT2]], dtype="float64")

MTQT_VARIABLES = ("w", "v", "kappa", "sigma", "h")
MT_VARIABLES = ("mnn", "mee", "mdd", "mne", "mnd", "med")
DC_VARIABLES = ("strike", "dip", "rake")


def rotation_x(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype="float64")


def rotation_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype="float64")


def rotation_z(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype="float64")


def v_to_gamma(v):
    """v (Tape & Tape 2015) -> lune longitude [rad] (sources.py:372-376)"""
    return (1.0 / 3.0) * np.arcsin(3.0 * v)


def w_to_beta(w, u_mapping=None, beta_mapping=None, n=1000):
    """w (Tape & Tape 2015) -> lune co-latitude [rad] (sources.py:379-392): linear interpolation in the table of
    u(beta) = 3/4 beta - 1/2 sin 2 beta + 1/16 sin 4 beta"""
    if beta_mapping is None:
        beta_mapping = np.linspace(0, pi, n)
    if u_mapping is None:
        u_mapping = ((3.0 / 4.0 * beta_mapping) - (1.0 / 2.0 * np.sin(2.0 * beta_mapping))
                     + (1.0 / 16.0 * np.sin(4.0 * beta_mapping)))
    return np.interp(3.0 * pi / 8.0 - w, u_mapping, beta_mapping)


def w_to_delta(w, n=1000):
    """w -> lune latitude [rad] (sources.py:395-400)"""
    return pi / 2.0 - w_to_beta(w)


def to6(m9):
    """(mnn, mee, mdd, mne, mnd, med) of a symmetric 3 x 3 tensor: the order ``calculate_radiation_weights`` assumes"""
    m9 = np.asarray(m9)
    return np.array([m9[0, 0], m9[1, 1], m9[2, 2], m9[0, 1], m9[0, 2], m9[1, 2]])


def symmat6(mnn, mee, mdd, mne, mnd, med):
    return np.array([[mnn, mne, mnd], [mne, mee, med], [mnd, med, mdd]], dtype="float64")


class _M9(object):
    """what ``pol_synthetics`` asks of ``source.pyrocko_moment_tensor()``: ``.m()`` and ``.m6()``"""

    def __init__(self, m9):
        self._m9 = np.array(m9, dtype="float64")

    def m(self):
        return self._m9.copy()

    def m6(self):
        return to6(self._m9)


class MTQTSource(object):
    """A moment-tensor point source in the Q-T parameterisation of Tape & Tape (2015) (sources.py:403-559).
    w in [-3/8 pi, 3/8 pi], v in [-1/3, 1/3], kappa in [0, 2 pi], sigma in [-pi/2, pi/2], h in [0, 1]; ``rho`` is the
    tensor's norm sqrt(2) M0 (1 by default: polarities do not see the scale)."""

    def __init__(self, w=0.0, v=0.0, kappa=0.0, sigma=0.0, h=0.0, rho=1.0, **kwargs):
        self.w, self.v, self.kappa, self.sigma, self.h = float(w), float(v), float(kappa), float(sigma), float(h)
        self.rho = float(rho)
        for k, val in kwargs.items():   # location, time, magnitude ... are carried, not used
            setattr(self, k, val)

    def update(self, **kwargs):
        for k, val in kwargs.items():
            setattr(self, k, float(val) if k in MTQT_VARIABLES else val)

    @property
    def u(self):
        return (3.0 / 8.0) * pi - self.w

    @property
    def gamma(self):
        return v_to_gamma(self.v)

    @property
    def beta(self):
        return w_to_beta(self.w, u_mapping=U_MAPPING, beta_mapping=BETA_MAPPING)

    def delta(self):
        return (pi / 2.0) - self.beta

    @property
    def theta(self):
        return np.arccos(self.h)

    @property
    def lune_lambda(self):
        sb, cb = np.sin(self.beta), np.cos(self.beta)
        sg, cg = np.sin(self.gamma), np.cos(self.gamma)
        return 1.0 / SQRT6 * LAMPBDA_FACTOR_MATRIX.dot(np.array([sb * cg, sb * sg, cb])) * self.rho

    @property
    def lune_lambda_matrix(self):
        return np.diag(self.lune_lambda)

    @property
    def rot_V(self):
        return rotation_z(-self.kappa).dot(rotation_x(self.theta)).dot(rotation_z(self.sigma))

    @property
    def rot_U(self):
        return self.rot_V.dot(rotation_y(-pi / 4.0))

    @property
    def m9_nwu(self):
        """north-west-up"""
        U = self.rot_U
        return U.dot(self.lune_lambda_matrix).dot(U.T)   # (U is orthogonal)

    @property
    def m9(self):
        """north-east-down"""
        R = rotation_x(pi)
        return R.dot(self.m9_nwu).dot(R.T)

    @property
    def m6(self):
        return to6(self.m9)

    @property
    def m6_astuple(self):
        return tuple(self.m6.ravel().tolist())

    def pyrocko_moment_tensor(self, store=None, target=None):
        return _M9(self.m9)


class MTSource(object):
    """six free tensor entries (north-east-down)"""

    def __init__(self, mnn=0.0, mee=0.0, mdd=0.0, mne=0.0, mnd=0.0, med=0.0, **kwargs):
        self.mnn, self.mee, self.mdd, self.mne, self.mnd, self.med = (float(x) for x in (mnn, mee, mdd, mne, mnd, med))

    def update(self, **kwargs):
        for k, val in kwargs.items():
            setattr(self, k, val)

    @property
    def m6(self):
        return np.array([getattr(self, k) for k in MT_VARIABLES], dtype="float64")

    @property
    def m9(self):
        return symmat6(*self.m6)

    def pyrocko_moment_tensor(self, store=None, target=None):
        return _M9(self.m9)


def dc_m6(strike, dip, rake):
    """Aki & Richards (1980, box 4.4): the unit double couple of (strike, dip, rake) [deg], north-east-down, in the
    order of operations of ``csrc/polarity.hip`` (``pol_dc``)"""
    d2r = pi / 180.0
    ph, de, la = strike * d2r, dip * d2r, rake * d2r
    sp, cp, sd, cd, sl, cl = np.sin(ph), np.cos(ph), np.sin(de), np.cos(de), np.sin(la), np.cos(la)
    s2p, c2p, s2d, c2d = 2.0 * (sp * cp), cp * cp - sp * sp, 2.0 * (sd * cd), cd * cd - sd * sd
    return np.array([-((sd * cl) * s2p + (s2d * sl) * (sp * sp)),
                     (sd * cl) * s2p - (s2d * sl) * (cp * cp),
                     s2d * sl,
                     (sd * cl) * c2p + (0.5 * (s2d * sl)) * s2p,
                     -((cd * cl) * cp + (c2d * sl) * sp),
                     -((cd * cl) * sp - (c2d * sl) * cp)])


class DCSource(object):
    """a pure double couple (strike, dip, rake in degrees)"""

    def __init__(self, strike=0.0, dip=90.0, rake=0.0, **kwargs):
        self.strike, self.dip, self.rake = float(strike), float(dip), float(rake)

    def update(self, **kwargs):
        for k, val in kwargs.items():
            setattr(self, k, val)

    @property
    def m6(self):
        return dc_m6(self.strike, self.dip, self.rake)

    @property
    def m9(self):
        return symmat6(*self.m6)

    def pyrocko_moment_tensor(self, store=None, target=None):
        return _M9(self.m9)


SOURCE_KINDS = {"mtqt": (MTQTSource, MTQT_VARIABLES), "mt": (MTSource, MT_VARIABLES), "dc": (DCSource, DC_VARIABLES)}
