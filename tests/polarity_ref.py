"""numpy restatement of csrc/polarity.hip for the tests: the same chain of operations on whole populations, written from
the formulas (Tape & Tape 2015; Aki & Richards 1980; Pugh et al. 2016 Appendix A; Weber 2018 eqs 6, 7), float64.

    m6(kind, P)                      (C, nvar) source variables -> (C, 6), normalised to sqrt(sum m9^2) = sqrt 2
    amplitudes(rw, m6)               (6, NT), (C, 6) -> (C, NT), summed in the kernel's order
    llk(obs, amp, gamma, sigma)      -> (C, NT)
    forward(...)                     the model's rows: (C, NT + 1) = (polarity_like, like)
and the error bounds the GPU tests assert (K_M6, E_LLK and the propagated forms).
"""
import numpy as np
from scipy.special import erf

PI = np.pi
N_TABLE = 1000
BETA_TABLE = np.linspace(0, PI, N_TABLE)
U_TABLE = 0.75 * BETA_TABLE - 0.5 * np.sin(2.0 * BETA_TABLE) + 0.0625 * np.sin(4.0 * BETA_TABLE)
U2 = 2.0 ** -53

# K_M6: bound on |m6 - exact| per entry in units of 2^-53, for every source kind.  Worst-case first-order propagation
# through the kernel's chain (mtqt is the longest), absolute errors in units u = 2^-53, with the bounds the OpenCL
# full profile states for double sin, cos, asin, acos (<= 2 ulp; erf <= 2, log <= 1 below) -- the accuracy class the
# device library is built to; the ROCm installation carries no document that states them, so they are an assumption:
#   angles   beta <= 2.5 (the interpolation's two roundings on a value <= pi: ulp = 4u), gamma <= 2 (asin 2 ulp of a
#            value <= pi/2, then * 1/3 and one rounding), theta <= 4 (acos, 2 ulp at ulp = 2u); kappa, sigma exact
#   sin/cos  own error 2u on a value <= 1, plus the angle's: beta 4.5, gamma 4, theta 6, kappa / sigma 2
#   lambda   products sb cg .. <= 9.5; rows of LAMBDA / sqrt 6 have 1-norm <= 1.7: <= 1.7 * 9.5 + 3 roundings = 19
#   U        four rotations: 2 + 6 + 2 + 0.5 in operator norm, entrywise <= sqrt 3 of that, plus three 3 x 3
#            products (8): <= 26
#   m_nwu    sum_k U_ik lam_k U_jk: 2 * 26 * (sum |lam_k U_jk| <= 1) + 19 * (sum |U_ik U_jk| <= 1) + 4 = 75
#   scale    the relative error of sqrt(sum m9^2) is at most that of the Frobenius norm, <= 3 * 75 = 225; the quotient
#            has entries <= sqrt 2: sqrt 2 * (75 + 225) = 424, + 2 for sqrt and the division
# -> K_M6 = 512, the next power of two.  (dc: angles <= 5u after deg -> rad, three-factor products, same scale step:
# below 200.  mt: the scale step alone.)  The tests print the observed multiple: a few units.
K_M6 = 512.0
# E_LLK: the ulp bounds of double erf and log, plus 4, where a document states them; none does here: the issue's 16
E_LLK = 16.0


def interp_numpy_steps(x, xp, fp):
    """numpy.interp restated step by step (search, end and node cases, slope * (x - xp[j]) + fp[j]), elementwise"""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    n = xp.size
    for i, xv in np.ndenumerate(x):
        if xv != xv:
            out[i] = xv
        elif xv < xp[0]:
            out[i] = fp[0]
        elif xv > xp[n - 1]:
            out[i] = fp[n - 1]
        else:
            j = int(np.searchsorted(xp, xv, side="right")) - 1
            if j == n - 1 or xp[j] == xv:
                out[i] = fp[j]
            else:
                slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
                out[i] = slope * (xv - xp[j]) + fp[j]
    return out


def w_to_beta(w):
    """numpy.interp itself (test_polarity_host.py shows it equal to the steps above bit for bit)"""
    return np.interp(3.0 * PI / 8.0 - np.asarray(w, dtype=np.float64), U_TABLE, BETA_TABLE)


def _raw_mtqt(P):
    w, v, kappa, sigma, h = [P[:, k] for k in range(5)]
    s2, s3, s6, r = np.sqrt(2.0), np.sqrt(3.0), np.sqrt(6.0), np.sqrt(0.5)
    gamma = (1.0 / 3.0) * np.arcsin(3.0 * v)
    beta = w_to_beta(w)
    theta = np.arccos(h)
    sb, cb, sg, cg = np.sin(beta), np.cos(beta), np.sin(gamma), np.cos(gamma)
    v0, v1, v2 = sb * cg, sb * sg, cb
    f = 1.0 / s6
    lam = [f * ((s3 * v0 - v1) + s2 * v2), f * (2.0 * v1 + s2 * v2), f * ((-s3 * v0 - v1) + s2 * v2)]
    ck, sk, ct, st, cs, ss = np.cos(kappa), np.sin(kappa), np.cos(theta), np.sin(theta), np.cos(sigma), np.sin(sigma)
    z = np.zeros_like(ck)
    A = [[ck, sk * ct, -(sk * st)], [-sk, ck * ct, -(ck * st)], [z, st, ct]]
    U = []
    for i in range(3):
        V0, V1, V2 = A[i][0] * cs + A[i][1] * ss, A[i][1] * cs - A[i][0] * ss, A[i][2]
        U.append([V0 * r + V2 * r, V1, V2 * r - V0 * r])

    def M(i, j):
        return ((U[i][0] * lam[0]) * U[j][0] + (U[i][1] * lam[1]) * U[j][1]) + (U[i][2] * lam[2]) * U[j][2]

    return np.stack([M(0, 0), M(1, 1), M(2, 2), -M(0, 1), -M(0, 2), M(1, 2)], axis=1)


def _raw_dc(P):
    d2r = PI / 180.0
    ph, de, la = P[:, 0] * d2r, P[:, 1] * d2r, P[:, 2] * d2r
    sp, cp, sd, cd, sl, cl = np.sin(ph), np.cos(ph), np.sin(de), np.cos(de), np.sin(la), np.cos(la)
    s2p, c2p, s2d, c2d = 2.0 * (sp * cp), cp * cp - sp * sp, 2.0 * (sd * cd), cd * cd - sd * sd
    return np.stack([-((sd * cl) * s2p + (s2d * sl) * (sp * sp)), (sd * cl) * s2p - (s2d * sl) * (cp * cp), s2d * sl,
                     (sd * cl) * c2p + (0.5 * (s2d * sl)) * s2p, -((cd * cl) * cp + (c2d * sl) * sp),
                     -((cd * cl) * sp - (c2d * sl) * cp)], axis=1)


def m6(kind, P):
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):     # (points outside the prior box, the zero tensor: NaN rows)
        m = {"mtqt": _raw_mtqt, "dc": _raw_dc, "mt": lambda X: X[:, :6].copy()}[kind](P)
        ssq = ((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]) + 2.0 * (
            (m[:, 3] * m[:, 3] + m[:, 4] * m[:, 4]) + m[:, 5] * m[:, 5])
        return m / (np.sqrt(ssq) / np.sqrt(2.0))[:, None]


def amplitudes(rw, m):
    rw = np.asarray(rw, dtype=np.float64)
    a = rw[0][None] * m[:, 0:1] + rw[1][None] * m[:, 1:2]
    for k in range(2, 6):
        a = a + rw[k][None] * m[:, k:k + 1]
    return a


def llk(obs, amp, gamma, sigma):
    """sigma: scalar or broadcastable to amp"""
    obs = np.asarray(obs, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = gamma + (1.0 - 2.0 * gamma) * (0.5 + 0.5 * erf((amp / sigma) / np.sqrt(2.0)))
        return ((1.0 + obs) / 2.0) * np.log(p) + ((1.0 - obs) / 2.0) * np.log(1.0 - p)


def source_params(kind, Q, off, fix):
    """(C, nvar) source variables of the rows of Q from the (6,) offset / fixed tables"""
    nv = {"mtqt": 5, "mt": 6, "dc": 3}[kind]
    Q = np.atleast_2d(Q)
    return np.stack([Q[:, off[k]] if off[k] >= 0 else np.full(Q.shape[0], fix[k]) for k in range(nv)], axis=1)


def forward(kind, Q, off, fix, rw, obs, n_t, gamma, hp_off, hp_fix):
    """the rows the model writes: (C, NT + 1) = polarity_like of every station, then like = their serial sum"""
    Q = np.atleast_2d(np.asarray(Q, dtype=np.float64))
    amp = amplitudes(rw, m6(kind, source_params(kind, Q, off, fix)))
    sig = np.concatenate([np.repeat((Q[:, hp_off[i]] if hp_off[i] >= 0 else np.full(Q.shape[0], hp_fix[i]))[:, None], n, axis=1)
                          for i, n in enumerate(n_t)], axis=1)
    ll = llk(obs, amp, gamma, sig)
    like = np.zeros(Q.shape[0])
    for s in range(ll.shape[1]):
        like = like + ll[:, s]
    return np.concatenate([ll, like[:, None]], axis=1)


def normal_pdf(x):
    return np.exp(-0.5 * x * x) / np.sqrt(2.0 * PI)


def bound_m6():
    return K_M6 * U2


def bound_amplitudes(rw):
    """(K + 8) 2^-53 sqrt 2 |rw_s|_1 per station"""
    return (K_M6 + 8.0) * U2 * np.sqrt(2.0) * np.abs(rw).sum(axis=0)


def bound_llk(rw, amp, ll, gamma, sigma):
    """2^-53 [(K + 8) sqrt 2 |rw_s|_1 (1 - 2 g) phi(a / sigma) / (sigma m) + E (1 / m + |llk|)], m = min(p, 1 - p)"""
    p = gamma + (1.0 - 2.0 * gamma) * (0.5 + 0.5 * erf((amp / sigma) / np.sqrt(2.0)))
    m = np.minimum(p, 1.0 - p)
    return U2 * ((K_M6 + 8.0) * np.sqrt(2.0) * np.abs(rw).sum(axis=0) * (1.0 - 2.0 * gamma) * normal_pdf(amp / sigma) / (sigma * m)
                 + E_LLK * (1.0 / m + np.abs(ll)))
