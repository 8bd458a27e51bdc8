"""
From a dataset's covariance terms to the sampler's likelihood weights.

The log-likelihood kernels consume, per dataset, the whitening matrix ``W`` (upper triangular,
``W^T W = inv(C)``) and ``log|C|`` (``multivariate_normal_chol``,
beat/models/distributions.py:119-138).  In the reference both come from ``heart.Covariance``
(beat/heart.py:104-263: ``chol_inverse`` :211-237, ``log_pdet`` :239-245, the shared scalar
``slog_pdet`` :247-253).  This module builds the same two quantities once per stage:

  ``whitening(C)``          one covariance      -> (W, log_pdet)          host LAPACK
  ``chol_inverse_batch``    a stack (nd, n, n)  -> (W, log_pdet) arrays   on the GPU
  ``Covariance``            the container the composites hand around: the three additive terms
                            (data, pred_g, pred_v) and the derived weights under the
                            reference's attribute names, so code written against
                            ``dataset.covariance.chol_inverse`` / ``.slog_pdet`` keeps working.
"""
import numpy as np

TERMS = ("data", "pred_g", "pred_v")


def log_determinant(A, inverse=False):
    """log|A| of a positive definite matrix through its Cholesky factor (heart.py:65-89);
    ``inverse`` gives log|inv(A)| = -log|A| the way the reference forms it"""
    half = np.log(np.diag(_lower_factor(A, inverse))).sum()
    return 2.0 * half


def _lower_factor(A, inverted=False):
    from scipy.linalg import cholesky
    L = cholesky(np.asarray(A, dtype=np.float64), lower=True)
    return np.linalg.inv(L) if inverted else L


def whitening(C):
    """(W, log_pdet) of one total covariance: W = cholesky(inv(C)).T, upper triangular with
    W^T W = inv(C) (heart.py:231-233); when inv(C) is numerically not positive definite the R
    factor of QR(inv(chol(C))) is used instead -- same W^T W (heart.py:234-237).
    log_pdet = 2 sum log diag chol(C) (heart.py:239-245)."""
    C = np.asarray(C, dtype=np.float64)
    if not C.any():
        raise ValueError("No covariances given!")
    L = _lower_factor(C)
    try:
        W = np.linalg.cholesky(np.linalg.inv(C)).T
    except np.linalg.LinAlgError:
        W = np.linalg.qr(np.linalg.inv(L))[1]
    return np.ascontiguousarray(W, dtype=np.float64), np.float64(2.0 * np.log(np.diag(L)).sum())


class _Scalar(object):
    """get_value / set_value holder standing in for the reference's shared scalar"""

    def __init__(self, name, value=0.0):
        self.name, self._v = name, value

    def get_value(self, borrow=False):
        return self._v

    def set_value(self, value, borrow=False):
        self._v = value

    def __float__(self):
        return float(self._v)


class Covariance(object):
    """Additive covariance terms of one dataset: ``data`` (observation noise), ``pred_g``
    (fault-geometry prediction error), ``pred_v`` (velocity-model prediction error); any of the
    latter two may be missing (heart.py:104-156).  Derived quantities are computed on access from
    the current terms."""

    def __init__(self, data=None, pred_g=None, pred_v=None):
        self._terms = dict(data=data, pred_g=pred_g, pred_v=pred_v)
        self.slog_pdet = _Scalar("cov_normalisation")
        if data is not None:
            self.update_slog_pdet()

    # -- the three terms as attributes
    def _resolve(self, name):
        """the stored term; one that a covariance update left on the device (a torch-cuda tensor) is downloaded when it is
        first read and kept as a numpy array from then on"""
        m = self._terms[name]
        if hasattr(m, "is_cuda"):
            m = self._terms[name] = m.detach().cpu().numpy()
        return m

    def _get(name):
        return property(lambda self: self._resolve(name),
                        lambda self, value: self._terms.__setitem__(name, value))

    data, pred_g, pred_v = _get("data"), _get("pred_g"), _get("pred_v")
    del _get

    def covs_supported(self):
        return [t for t in TERMS[1:]] + [TERMS[0]]

    def _term(self, name):
        """the term as an array of the data covariance's shape (zeros when absent)"""
        if name not in TERMS:
            raise NotImplementedError("Covariance term %s not supported" % name)
        ref = self._resolve("data")
        m = self._resolve(name)
        if m is None or (np.size(m) != np.size(ref) and not np.any(m)):
            m = np.zeros_like(ref, dtype="float64")
            self._terms[name] = m
        elif np.size(m) != np.size(ref):
            raise ValueError("%s covariances defined but size inconsistent!" % name)
        return m

    check_matrix_init = _term

    def _sum(self, names):
        return sum(self._term(n) for n in names)

    c_total = property(lambda self: self._sum(TERMS))
    p_total = property(lambda self: self._sum(TERMS[1:]))

    # -- inverses
    @staticmethod
    def _inv(M, what):
        if M is None or not np.any(M):
            raise ValueError(what)
        return np.linalg.inv(M).astype("float64")

    def inverse(self, factor=1.0):
        return self._inv(self.c_total * factor, "No covariances given!")

    inverse_p = property(lambda self: self._inv(self.p_total, "No model covariance defined!"))

    @property
    def inverse_d(self):
        if self._terms["data"] is None:
            raise AttributeError("No data covariance matrix defined!")
        return self._inv(self._resolve("data"), "No covariances given!")

    # -- factors and weights
    def chol(self, factor=1.0):
        total = self.c_total * factor
        if not np.any(total):
            raise ValueError("No covariances given!")
        return _lower_factor(total).astype("float64")

    chol_inverse = property(lambda self: whitening(self.c_total)[0])
    log_pdet = property(lambda self: whitening(self.c_total)[1])

    def update_slog_pdet(self):
        self.slog_pdet.set_value(self.log_pdet)


def chol_inverse_batch(covs, device=None):
    """(W (nd,n,n), log_pdet (nd,)) of a stack of covariances at once on the GPU -- what
    ``update_weights`` needs per stage for every dataset of a wavemap (seismic.py:1509-1534).
    ``beatamd_chol_inverse_batch`` (csrc/chol.hip): blocked factorisation of the exchange-flipped
    matrices on the FP64 matrix cores; numpy in, numpy out."""
    from .engine import get_context
    dev_index = None if device is None else getattr(device, "index", device)
    W, log_pdet = get_context(dev_index).chol_inverse_batch(np.ascontiguousarray(covs, dtype=np.float64))
    return W, log_pdet


# ------------------------------------------------------------------------------------------------
# Geometry-mode synthetics seams (beat/heart.py:3564-3762 seis_synthetics, :4158-4239 geo_synthetics)
#
# In the reference both are thin wrappers around ``engine.process(sources, targets)`` of pyrocko's
# GF-store engine (layered medium; not in the reference tree).  The arithmetic shipped here is the
# homogeneous half space (``HalfspaceEngine``: rectangular dislocations, Okada 1985, and Mogi
# sources on the GPU); results are NOT comparable with a layered GF store to 1e-6 -- parity with
# BEAT is unpinned for geometry mode, the kernels are pinned to Okada's published check values
# (tests/test_geometry.py).  What is reproduced exactly is the call protocol: argument order,
# ``outmode`` values, ordering and stacking of the per-(source, target) results.

km = 1000.0


class StaticTarget(object):
    """observation points of one geodetic dataset: east / north shifts [m] from the reference
    location (the fields of pyrocko.gf.StaticTarget this path reads)"""

    def __init__(self, east_shifts, north_shifts, lats=None, lons=None):
        self.east_shifts = np.ascontiguousarray(east_shifts, dtype=np.float64)
        self.north_shifts = np.ascontiguousarray(north_shifts, dtype=np.float64)
        self.lats = np.zeros_like(self.east_shifts) if lats is None else np.asarray(lats)
        self.lons = np.zeros_like(self.east_shifts) if lons is None else np.asarray(lons)


class GeodeticDataset(StaticTarget):
    """the fields of heart.GeodeticDataset / DiffIFG (heart.py:1040-1520) the library builder and the discretizer read:
    local coordinates [m] relative to the event (all datasets and subfaults share its reference location),
    the line-of-sight vectors (n, 3) = [Sn, Se, Su], the weights ``odw`` (default ones) and the displacements"""

    def __init__(self, east_shifts, north_shifts, los_vector, odw=None, displacement=None, name=""):
        super(GeodeticDataset, self).__init__(east_shifts, north_shifts)
        n = self.east_shifts.size
        self.los_vector = np.ascontiguousarray(los_vector, dtype=np.float64).reshape(n, 3)
        self.odw = np.ones(n) if odw is None else np.ascontiguousarray(odw, dtype=np.float64).reshape(n)
        self.displacement = (np.zeros(n) if displacement is None
                             else np.ascontiguousarray(displacement, dtype=np.float64).reshape(n))
        self.name = name

    samples = property(lambda self: self.east_shifts.size)

    def update_local_coords(self, loc=None):
        """heart.py:1117-1140 -> (north_shifts, east_shifts) [m]; no reprojection"""
        return self.north_shifts, self.east_shifts


def concatenate_datasets(datasets):
    """heart.py:3495-3530 -> (displacements, los_vectors, odws, sizes); ``sizes`` (samples per dataset, in order)
    stands where the reference returns its ListToArrayBijection"""
    disp = np.hstack([d.displacement for d in datasets])
    los = np.vstack([d.los_vector for d in datasets])
    odws = np.hstack([d.odw for d in datasets])
    return disp, los, odws, [int(d.samples) for d in datasets]


class HalfspaceSource(object):
    """attribute bag with pyrocko's RectangularSource field names (SI units: m, deg);
    kind "rectangular" | "mogi" (for Mogi: ``volume_change`` [m^3])"""

    _defaults = dict(east_shift=0.0, north_shift=0.0, depth=0.0, strike=0.0, dip=90.0, rake=0.0,
                     length=0.0, width=0.0, slip=0.0, opening_fraction=0.0, volume_change=0.0,
                     time=0.0)

    def __init__(self, kind="rectangular", **kwargs):
        if kind not in ("rectangular", "mogi"):
            raise ValueError("unknown source kind %s" % kind)
        self.kind = kind
        for k, v in self._defaults.items():
            setattr(self, k, float(kwargs.pop(k, v)))
        if kwargs:
            raise TypeError("unknown source attributes: %s" % ", ".join(sorted(kwargs)))

    def update(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, float(np.ravel(v)[0]))

    def kernel_parameters(self):
        """the 10 slots of beatamd_halfspace_displacements_batch ([km], [deg], [m])"""
        amp = self.volume_change if self.kind == "mogi" else self.slip
        return [self.east_shift / km, self.north_shift / km, self.depth / km, self.strike, self.dip,
                self.rake, self.length / km, self.width / km, amp, self.opening_fraction]


class HalfspaceEngine(object):
    """stands where the reference passes a pyrocko ``LocalEngine``: static displacements of
    half-space sources at surface points, evaluated on the GPU"""

    def __init__(self, nu=0.25, ctx=None):
        self.nu, self._ctx = float(nu), ctx

    @property
    def ctx(self):
        if self._ctx is None:
            from .engine import get_context
            self._ctx = get_context()
        return self._ctx

    def close_cashed_stores(self):   # the reference's Ops call this before pickling
        pass

    def __getstate__(self):
        return {"nu": self.nu}       # the device context is per process: looked up again on use

    def __setstate__(self, state):
        self.nu, self._ctx = state["nu"], None

    def static_displacements(self, sources, targets):
        """-> list, index i_t + i_s * n_targets (heart.py:4213-4216), of (n_points, 3) arrays
        [north, east, up] = [n, e, -d] (heart.py:4218-4224)"""
        kinds = [1 if s.kind == "mogi" else 0 for s in sources]
        prm = np.array([[s.kernel_parameters() for s in sources]])
        east = np.concatenate([t.east_shifts for t in targets]) / km
        north = np.concatenate([t.north_shifts for t in targets]) / km
        out = self.ctx.halfspace_displacements_batch(kinds, prm, east, north, self.nu)[0]
        bounds = np.cumsum([0] + [t.east_shifts.size for t in targets])
        return [out[i_s, bounds[i_t]:bounds[i_t + 1]].copy()
                for i_s in range(len(sources)) for i_t in range(len(targets))]


def geo_synthetics(engine, targets, sources, outmode="stacked_array", plot=False, nthreads=1):
    """heart.py:4158-4239 with the same arguments and ``outmode`` values:
    "arrays" one array per (source, target); "array" all of them stacked vertically;
    "stacked_arrays" per target, summed over the sources; "stacked_array" those stacked."""
    if not hasattr(engine, "static_displacements"):
        raise TypeError("engine %r provides no static displacements (HalfspaceEngine does; the "
                        "reference's layered GF-store engine is pyrocko's and out of scope)" % (engine,))
    disp_arrays = engine.static_displacements(list(sources), list(targets))
    ns, nt = len(sources), len(targets)

    def per_target():
        return [sum(disp_arrays[i_t + i_s * nt] for i_s in range(ns)) for i_t in range(nt)]

    if outmode == "arrays":
        return disp_arrays
    if outmode == "array":
        return np.vstack(disp_arrays)
    if outmode == "stacked_arrays":
        return per_target()
    if outmode == "stacked_array":
        return np.vstack(per_target())
    raise ValueError("Outmode %s not available" % outmode)


def fft_transforms(time_domain_signals, valid_spectrum_indices, outmode="array", pad_to_pow2=True, ctx=None):
    """heart.py:4091-4155 with outmode "array": the amplitude spectra ``abs(rfft(tr, ntrans))[lower_idx:upper_idx]`` of
    the rows of an (n, N) array, ntrans = nextpow2(N) -- on the device (``beatamd_amp_spectrum_batch``), all rows in one
    launch instead of one numpy transform per trace.  A numpy array gives a numpy array, a torch-cuda tensor (e.g. the
    synthetics of an ensemble as ``LogpForwFunc.synthetics`` returns them, reshaped to rows) a tensor on its device: what
    ``fuzzy_spectrum`` plots.  The other outmodes return pyrocko traces and are not offered; ``pad_to_pow2=False`` (a
    transform of length N) is offered where N is a power of two, the only lengths the device transform has."""
    from .engine import get_context
    from .utility import nextpow2
    if outmode != "array":
        raise TypeError("Outmode %s not supported!" % outmode)
    lower_idx, upper_idx = valid_spectrum_indices
    x = time_domain_signals
    if not hasattr(x, "data_ptr") or isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("fft_transforms: outmode \"array\" takes an (n_data, n_samples) array, got %s" % (tuple(x.shape),))
    n_samples = int(x.shape[1])
    ntrans = nextpow2(n_samples)
    if not pad_to_pow2 and ntrans != n_samples:
        raise NotImplementedError("fft_transforms: pad_to_pow2=False needs a power-of-two trace length on the device, "
                                  "got %d samples" % n_samples)
    ctx = ctx or get_context()
    return ctx.amp_spectrum_batch(x, ntrans, (int(lower_idx), int(upper_idx)))


def seis_synthetics(engine, sources, targets, arrival_taper=None, wavename="any_P", filterer=None,
                    reference_taperer=None, plot=False, nthreads=1, outmode="array",
                    pre_stack_cut=False, taper_tolerance_factor=0.0, arrival_times=None,
                    chop_bounds=["b", "c"]):
    """heart.py:3564-3762 call protocol.  The waveform synthesis itself (``engine.process`` on a
    layered GF store, then filter / taper / chop through pyrocko ``Trace`` methods,
    heart.py:3658-3700) is third-party arithmetic outside the reference tree and is NOT
    re-implemented: ``engine`` must provide ``seismograms(sources, targets, ...) ->
    (traces (n_sources * n_targets, n_samples), tmins (n_targets,))`` already post-processed.  This
    function does what the reference does with them afterwards: the stack over sources
    (:3719-3724) and the ``outmode`` dispatch ("array", "data")."""
    if not hasattr(engine, "seismograms"):
        raise NotImplementedError(
            "geometry-mode seismic synthetics need a waveform engine (pyrocko GF stores in the "
            "reference); none is part of this package -- the finite-fault (FFI) path computes its "
            "synthetics from the linear GF library instead (beat_amd.ffi)")
    synths, tmins = engine.seismograms(sources, targets, arrival_taper=arrival_taper, wavename=wavename,
                                       filterer=filterer, arrival_times=arrival_times,
                                       chop_bounds=chop_bounds)
    synths = np.asarray(synths, dtype=np.float64)
    ns, nt = len(sources), len(targets)
    if synths.shape[0] != ns * nt:
        raise ValueError("Stacking error, traces different lengths!")
    outstack = synths if ns == 1 else sum(synths[k * nt:(k + 1) * nt] for k in range(ns))
    if outmode == "array":
        return outstack, np.asarray(tmins)
    if outmode == "data":
        return list(synths), np.asarray(tmins)
    raise TypeError("Outmode %s not supported!" % outmode)


# ------------------------------------------------------------------ first-motion polarities (heart.py:3891-4088)
# Station propagation coefficients after Pugh et al. (2016, GJI, Appendix A).  Takeoff angles are measured from the
# downward vertical, azimuths from north, both in radians; the rows multiply (mnn, mee, mdd, mne, mnd, med).
def _sincos(takeoff_angles, azimuths):
    t = np.asarray(takeoff_angles, dtype=np.float64)
    a = np.asarray(azimuths, dtype=np.float64)
    return np.sin(t), np.cos(t), np.sin(a), np.cos(a)


def radiation_weights_p(takeoff_angles, azimuths):
    """P waves -> (6, n_stations) (heart.py:3891-3912)"""
    st, ct, sa, ca = _sincos(takeoff_angles, azimuths)
    stp2, st2, sa2 = st ** 2, 2 * st * ct, 2 * ca * sa
    return np.array([stp2 * ca ** 2, stp2 * sa ** 2, ct ** 2, stp2 * sa2, st2 * ca, st2 * sa])


def radiation_weights_sv(takeoff_angles, azimuths):
    """SV waves -> (6, n_stations) (heart.py:3915-3935)"""
    st, ct, sa, ca = _sincos(takeoff_angles, azimuths)
    sct = st * ct
    ct2 = np.cos(2 * np.asarray(takeoff_angles, dtype=np.float64))
    return np.array([sct * ca ** 2, sct * sa ** 2, -sct, 2 * sct * sa * ca, ct2 * ca, ct2 * sa])


def radiation_weights_sh(takeoff_angles, azimuths):
    """SH waves -> (6, n_stations) (heart.py:3938-3958)"""
    st, ct, sa, ca = _sincos(takeoff_angles, azimuths)
    ca2 = np.cos(2 * np.asarray(azimuths, dtype=np.float64))
    a1 = st * (sa * ca)
    return np.array([-a1, a1, np.zeros_like(st), st * ca2, -ct * sa, ct * ca])


def radiation_gamma(takeoff_angles_rad, azimuths_rad):
    """unit ray direction -> (3, n_stations) (heart.py:3961-3973)"""
    st, ct, sa, ca = _sincos(takeoff_angles_rad, azimuths_rad)
    return np.array([st * ca, st * sa, ct])


def radiation_theta(takeoff_angles_rad, azimuths_rad):
    """SV polarisation direction -> (3, n_stations) (heart.py:3976-3988)"""
    st, ct, sa, ca = _sincos(takeoff_angles_rad, azimuths_rad)
    return np.array([ct * ca, ct * sa, -st])


def radiation_phi(azimuths_rad):
    """SH polarisation direction -> (3, n_stations) (heart.py:3991-4001)"""
    a = np.asarray(azimuths_rad, dtype=np.float64)
    ca, sa = np.cos(a), np.sin(a)
    return np.array([-sa, ca, np.zeros_like(ca)])


def radiation_matmul(m9, takeoff_angles_rad, azimuths_rad, wavename):
    """the radiation pattern as the bilinear form direction^T . m9 . gamma per station (heart.py:4004-4025)"""
    gamma = radiation_gamma(takeoff_angles_rad, azimuths_rad)
    if wavename == "any_P":
        left = gamma
    elif wavename == "any_SV":
        left = radiation_theta(takeoff_angles_rad, azimuths_rad)
    elif wavename == "any_SH":
        left = radiation_phi(azimuths_rad)
    else:
        return None
    return np.einsum("is,ij,js->s", left, np.asarray(m9, dtype=np.float64), gamma)


radiation_function_mapping = {"any_P": radiation_weights_p, "any_SH": radiation_weights_sh, "any_SV": radiation_weights_sv}


def calculate_radiation_weights(takeoff_angles_rad, azimuths_rad, wavename):
    """(6, n_stations) propagation coefficients of a wave type (heart.py:4035-4050)"""
    return radiation_function_mapping[wavename](takeoff_angles_rad, azimuths_rad)


def pol_synthetics(source, takeoff_angles_rad=None, azimuths_rad=None, wavename="any_P", radiation_weights=None):
    """first-motion amplitudes of ``source`` at the stations (heart.py:4053-4088): the tensor scaled to
    ``sqrt(sum m9^2) = sqrt 2`` times the propagation coefficients.  One source on the host; populations go through
    ``beat_amd.polarity_binding.polarity_amplitudes_batch``."""
    from .sources import to6
    if radiation_weights is None:
        if takeoff_angles_rad is None or azimuths_rad is None:
            raise ValueError("Need to either provide radiation weights or takeoff-angles and azimuths!")
        radiation_weights = calculate_radiation_weights(takeoff_angles_rad, azimuths_rad, wavename=wavename)
    m9 = np.array(source.pyrocko_moment_tensor().m(), dtype=np.float64)
    m9 /= np.sqrt(np.sum(m9 ** 2)) / np.sqrt(2.0)
    return np.asarray(radiation_weights).T.dot(to6(m9))
