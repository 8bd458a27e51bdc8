"""
Host-side description of a distributed-slip (FFI) problem and its compilation to the
fused GPU model -- the counterpart of what the reference assembles in

  beat/models/problems.py:212-248        Problem.built_model  (like = sum of composites)
  beat/models/seismic.py:1210-1349       SeismicDistributerComposite.get_formula
  beat/models/geodetic.py:1030-1084      GeodeticDistributerComposite.get_formula
  beat/models/laplacian.py:98-139        LaplacianDistributerComposite.get_formula
  beat/sampler/base.py:598-615           logp_forw  (the compiled function seam, "B1")

The reference builds a pytensor graph and compiles it to a one-chain function
``f(q) -> [unobserved RVs..., seis_like, geo_like, laplacian_like, like]``.  Here the
same description is uploaded once to HBM and evaluated for a whole batch of chains per
call; ``LogpForwFunc`` keeps the one-chain call signature on top of the batched one.
"""
import logging
from collections import OrderedDict

import numpy as np

from .. import _lib
from .._marshal import upload
from ..engine import get_context
from .corrections import correction_tables

logger = logging.getLogger("beat_amd.models")

hyper_name_laplacian = "h_laplacian"  # beat/config.py:126
hypo_vars = ["nucleation_strike", "nucleation_dip", "time"]  # beat/config.py:86
static_dist_vars = ["uparr", "uperp", "utens"]  # beat/config.py:83


class ParameterLayout(object):
    """Flat parameter vector q: concatenation of the raveled value variables in model
    order (pymc DictToArrayBijection; reference backend.py:147,165)."""

    def __init__(self, varsizes):
        self.varsizes = OrderedDict((k, int(v)) for k, v in varsizes.items())
        self.offsets = OrderedDict()
        o = 0
        for k, v in self.varsizes.items():
            self.offsets[k] = o
            o += v
        self.size = o

    def offset(self, name, index=0):
        if name not in self.offsets:
            raise KeyError("variable %s is not part of the parameter vector" % name)
        if not (0 <= index < self.varsizes[name]):
            raise IndexError("index %d outside variable %s" % (index, name))
        return self.offsets[name] + index

    def map(self, point):
        """dict -> flat array (bij.map)"""
        q = np.empty(self.size)
        for k, o in self.offsets.items():
            q[o:o + self.varsizes[k]] = np.ravel(point[k])
        return q

    def rmap(self, q):
        """flat array -> dict (bij.rmap)"""
        q = np.asarray(q)
        return OrderedDict((k, q[..., o:o + self.varsizes[k]]) for k, o in self.offsets.items())

    def bounds(self, lower, upper):
        lo, up = np.empty(self.size), np.empty(self.size)
        for k, o in self.offsets.items():
            lo[o:o + self.varsizes[k]] = lower[k]
            up[o:o + self.varsizes[k]] = upper[k]
        return lo, up


class SeismicWavemap(object):
    """One wavemap of the seismic composite (seismic.py:1274-1341).

    gfs            dict slip-varname -> beat_amd.ffi.SeismicGFLibrary (HBM resident)
    data           (T, N) observed, tapered/filtered traces (wmap.shared_data_array)
    weights        (T,) scalars [W = w I] or (T, N, N) dense chol_inverse matrices
    slog_pdet      (T,)
    hypers         list of (hyper-parameter name, index) per dataset
                   (distributions.py:117-126: index 0 unless hp_specific)
    time_shifts    None or (name of the hierarchical variable, station_correction_idxs (T,))
    domain         "time" | "spectrum" (WaveformFitConfig.domain, heart.py:526).  In the spectrum domain the likelihood
                   is formed on amplitude spectra, as the reference's geometry mode does it (pytensorf.py:294-311,
                   heart.py:3086-3095, 4091-4155) -- its own FFI composite refuses the domain (seismic.py:1277-1278), so
                   this goes beyond it.  ``data`` stays the (T, N) time-domain traces; ``deltat`` (s) and
                   ``taper_frequencies`` (f_lo, f_hi) [Hz] (``filterer_minmax(filterer)`` in the reference) give
                       ntrans = nextpow2(N); deltaf = 1 / (ntrans * deltat)                          heart.py:3122-3124
                       valid_spectrum_indices = (lo, hi) = get_valid_spectrum_data(deltaf, taper_frequencies)
                   and M = ``nsamples_spectrum`` = hi - lo samples per dataset: weights are (T,) or (T, M, M).
                   0 <= lo < hi <= ntrans/2 + 1 is required (numpy's slice would silently shorten a longer band).
    """

    def __init__(self, gfs, data, weights, slog_pdet, hypers, time_shifts=None,
                 interpolation="nearest_neighbor", name="any_P_0", domain="time", deltat=None, taper_frequencies=None):
        self.gfs = gfs
        self.data = np.ascontiguousarray(data, dtype=np.float64)
        self.weights = weights
        self.slog_pdet = np.ascontiguousarray(slog_pdet, dtype=np.float64)
        self.hypers = list(hypers)
        self.time_shifts = time_shifts
        self.interpolation = interpolation
        self.name = name
        self._wset = None
        self.is_prewhitened = False
        if domain not in ("time", "spectrum"):
            raise ValueError("wavemap %s: domain must be \"time\" or \"spectrum\", got %r" % (name, domain))
        self.domain = domain
        self.deltat, self.taper_frequencies = deltat, taper_frequencies
        self.ntrans, self.valid_spectrum_indices, self._data_spec = None, None, None
        if domain == "spectrum":
            self._setup_spectrum()

    def _setup_spectrum(self):
        from ..utility import get_valid_spectrum_data, nextpow2
        what = "wavemap %s in the spectrum domain" % self.name
        if self.deltat is None or not float(self.deltat) > 0.0:
            raise ValueError("%s needs the sampling interval deltat > 0 of its traces" % what)
        if self.taper_frequencies is None or len(self.taper_frequencies) != 2:
            raise ValueError("%s needs taper_frequencies = (f_lo, f_hi)" % what)
        if self.data.ndim != 2 or self.data.shape[1] < 2:
            raise ValueError("%s needs (T, N) time-domain data with N >= 2" % what)
        T, N = self.data.shape
        ntrans = nextpow2(N)
        if not 2 <= ntrans <= 8192:
            raise ValueError("%s: transform length %d outside [2, 8192]" % (what, ntrans))
        deltaf = 1.0 / (ntrans * float(self.deltat))
        lo, hi = get_valid_spectrum_data(deltaf, [float(f) for f in self.taper_frequencies])
        if not 0 <= lo < hi <= ntrans // 2 + 1:
            raise ValueError("%s: the band %s Hz gives the spectrum indices [%d, %d), outside the %d bins of a transform of "
                             "%d samples at deltaf = %g Hz (numpy's slice would shorten it silently)"
                             % (what, tuple(self.taper_frequencies), lo, hi, ntrans // 2 + 1, ntrans, deltaf))
        self.ntrans, self.valid_spectrum_indices = ntrans, (lo, hi)
        M = hi - lo
        w = np.shape(self.weights)
        if w not in ((T,), (T, M, M)):
            raise ValueError("%s: weights must be (%d,) or (%d, %d, %d) -- M = hi - lo spectrum samples, not the %d time "
                             "samples -- got %s" % (what, T, T, M, M, N, w))

    @property
    def n_t(self):
        return self.data.shape[0]

    @property
    def nsamples_spectrum(self):
        """M = hi - lo, samples per dataset of a spectrum wavemap (None in the time domain)"""
        if self.domain != "spectrum":
            return None
        return self.valid_spectrum_indices[1] - self.valid_spectrum_indices[0]

    @property
    def nsamples(self):
        """samples per dataset as the likelihood counts them: N, or M in the spectrum domain"""
        return self.nsamples_spectrum if self.domain == "spectrum" else self.data.shape[1]

    @property
    def data_spec(self):
        """(T, M) observed amplitude spectra, the reference's own host arithmetic for the observed side (prepare_data,
        heart.py:3086-3095 -> fft_transforms): ``abs(rfft(data, ntrans, axis=1))[:, lo:hi]``"""
        if self.domain != "spectrum":
            return None
        if self._data_spec is None:
            lo, hi = self.valid_spectrum_indices
            self._data_spec = np.ascontiguousarray(np.abs(np.fft.rfft(self.data, self.ntrans, axis=1))[:, lo:hi])
        return self._data_spec

    def prewhitened(self, ctx=None, inplace=False):
        """Pre-whitened twin of this wavemap: every library row
        and the data are multiplied by W_t once, G'[t,p,d,s,:] = W_t . G[t,p,d,s,:] and
        d'_t = W_t . d_t, so that ||W_t (d_t - syn_t)||^2 = ||d'_t - syn'_t||^2 and the dense
        W.r product (distributions.py:128) drops out of the per-step path.  Legal because
        the sampler records likelihoods, not synthetics (metropolis.py:160-162); the values
        agree with the unwhitened path to rounding.  The row products run on the FP64 matrix
        cores (``beatamd_whiten_rows``: rows . W_t^T, the zero half of the upper-triangular W_t
        skipped), in place on the HBM-resident library, chunked so that no second library copy is
        needed when ``inplace``.  A weight update (seismic.py:1509-1534) re-whitens rows and data in
        place with ``M_t = W_new,t . inv(W_old,t)`` (``LogpForwFunc.update_weights``)."""
        if self.domain == "spectrum":
            raise ValueError("wavemap %s is in the spectrum domain: it cannot be pre-whitened, |rfft(W s)| is not "
                             "W |rfft(s)| (the amplitude does not commute with the whitening operator)" % self.name)
        import torch

        from ..engine import get_context
        from ..ffi import SeismicGFLibrary, SeismicGFLibraryConfig
        w = np.asarray(self.weights, dtype=np.float64)
        if w.ndim != 3:
            return self  # scalar weights need no whitening
        ctx = ctx or get_context()
        dev = torch.device("cuda", ctx.device)
        T, N = self.data.shape
        gfs = {}
        w = upload(w, dev)    # (one upload; a host array would be staged per call)
        for name, gf in self.gfs.items():
            if gf._device_tensor is not None:
                G = gf._device_tensor if inplace else gf._device_tensor.clone()
            else:
                G = upload(gf._gfmatrix, dev)
            ctx.whiten_rows_batch(G.view(T, -1, N), w)
            cfg = gf.config
            g2 = SeismicGFLibrary(SeismicGFLibraryConfig(
                dimensions=cfg.dimensions, starttime_sampling=cfg.starttime_sampling,
                duration_sampling=cfg.duration_sampling, starttime_min=cfg.starttime_min,
                duration_min=cfg.duration_min, component=cfg.component, datatype=cfg.datatype,
                mapnumber=cfg.mapnumber, wavename=cfg.wavename, crust_ind=cfg.crust_ind))
            g2.adopt_device_tensor(G)
            gfs[name] = g2
        d = torch.from_numpy(self.data).to(dev).contiguous()
        ctx.whiten_rows_batch(d.view(T, 1, N), w)     # (W d)^T = d^T W^T
        ctx.synchronize()
        wm = SeismicWavemap(gfs, d.cpu().numpy(), np.ones(T), self.slog_pdet, self.hypers,
                            self.time_shifts, self.interpolation, self.name)
        wm.is_prewhitened = True
        wm._whitened_with = w      # the operator folded into rows and data (for update_weights)
        return wm


class GeodeticData(object):
    """The geodetic composite (geodetic.py:1030-1084).

    gfs        dict slip-varname -> beat_amd.ffi.GeodeticGFLibrary
    data/odws  (Nobs,) concatenated over datasets (heart.concatenate_datasets :3356-3384)
    sizes      samples per dataset (Bij.srmap split)
    weights    list of (n_k, n_k) chol_inverse matrices or scalars
    corrections  None or one list of set-up correction objects (models.corrections) per dataset, subtracted from
               the weighted residual in list order (geodetic.py:411-427, 1076-1077); their variables are sampled
               where the layout holds them and constant where ``fixed`` {name: value} does (lower == upper in
               the reference, geodetic.py:401-405)
    """

    def __init__(self, gfs, data, odws, sizes, weights, slog_pdets, hypers, corrections=None, fixed=None):
        self.gfs = gfs
        self.data = np.ascontiguousarray(data, dtype=np.float64)
        self.odws = np.ascontiguousarray(odws, dtype=np.float64)
        self.sizes = [int(s) for s in sizes]
        self.weights = weights
        self.slog_pdets = [float(s) for s in slog_pdets]
        self.hypers = list(hypers)
        self.corrections = corrections
        self.fixed = dict(fixed or {})
        self._wsets = []


class FFIProblem(object):
    """Distributed-slip problem: which variables are sampled and which composites make up
    ``like``.  Output vector order: seis_like (per wavemap, per dataset), geo_like (per
    dataset), laplacian_like, like  (SURVEY Appendix C)."""

    def __init__(self, layout, n_patch_dip, n_patch_strike, patch_sizes, slip_varnames,
                 wavemaps=(), geodetic=None, laplacian=None, lower=None, upper=None):
        self.layout = layout
        self.n_patch_dip = [int(v) for v in np.atleast_1d(n_patch_dip)]
        self.n_patch_strike = [int(v) for v in np.atleast_1d(n_patch_strike)]
        self.patch_sizes = [float(v) for v in np.atleast_1d(patch_sizes)]
        self.slip_varnames = list(slip_varnames)
        self.wavemaps = list(wavemaps)
        self.geodetic = geodetic
        self.laplacian = laplacian  # (L (P,P), logdet) or None
        self.lower, self.upper = lower, upper
        if not (1 <= len(self.slip_varnames) <= 3):
            raise ValueError("1..3 slip variables supported")
        for v in self.slip_varnames:
            if v not in static_dist_vars:
                raise ValueError("%s is not a slip variable %s" % (v, static_dist_vars))

    @property
    def npatches(self):
        return int(sum(d * s for d, s in zip(self.n_patch_dip, self.n_patch_strike)))

    @property
    def out_names(self):
        names = []
        for wm in self.wavemaps:
            names += ["seis_like_%s_%d" % (wm.name, i) for i in range(wm.n_t)]
        if self.geodetic is not None:
            names += ["geo_like_%d" % i for i in range(len(self.geodetic.sizes))]
        if self.laplacian is not None:
            names.append("laplacian_like")
        names.append("like")
        return names

    def c_layout(self):
        L = _lib.FfiLayout()
        lay = self.layout
        L.nparams = lay.size
        L.nvar = len(self.slip_varnames)
        for i in range(4):
            L.slip_off[i] = lay.offsets[self.slip_varnames[i]] if i < L.nvar else -1
        L.durations_off = lay.offsets.get("durations", -1)
        L.velocities_off = lay.offsets.get("velocities", -1)
        L.nuc_strike_off = lay.offsets.get("nucleation_strike", -1)
        L.nuc_dip_off = lay.offsets.get("nucleation_dip", -1)
        L.time_off = lay.offsets.get("time", -1)
        L.h_laplacian_off = lay.offsets.get(hyper_name_laplacian, -1)
        return L

    def compile(self, ctx=None, prewhiten=False, return_rvs=False):
        """Upload to HBM and return the batched log-likelihood function (``logp_forw``).
        prewhiten: False | True (whitened copy of the library) | "inplace".
        return_rvs: f(q) lists the free variables in front of the deterministics like the
        reference's compiled function (model.unobserved_RVs)."""
        ctx = ctx or get_context()
        lay = self.layout
        seismic = len(self.wavemaps) > 0
        if prewhiten:
            self.wavemaps = [wm.prewhitened(ctx, inplace=(prewhiten == "inplace"))
                             for wm in self.wavemaps]
        mid = ctx.ffi_model_create(self.c_layout(),
                                   self.n_patch_dip if seismic else [],
                                   self.n_patch_strike if seismic else [],
                                   self.patch_sizes if seismic else [])
        owned_wm, owned_geo = [], []     # weight sets THIS compiled model creates (released by it alone: ADVICE r5)
        for wm in self.wavemaps:
            libs = []
            for v in self.slip_varnames:
                gf = wm.gfs[v]
                gf.init_optimization(ctx)
                libs.append(gf.lib_id)
            T, N = wm.data.shape
            w = np.asarray(wm.weights, dtype=np.float64)
            if w.ndim == 1:
                wm._wset = ctx.weights_create_scalar(w, wm.slog_pdet, wm.nsamples)
            else:
                wm._wset = ctx.weights_create_dense(w, wm.slog_pdet)
                _log_band(ctx, wm._wset, "wavemap %s" % getattr(wm, "name", len(owned_wm)))
            owned_wm.append(wm._wset)
            hp_off = [lay.offset(n, i) for n, i in wm.hypers]
            shift_off = None
            if wm.time_shifts is not None:
                name, sidx = wm.time_shifts
                shift_off = [lay.offset(name, int(i)) for i in sidx]
            if wm.domain == "spectrum":
                ctx.ffi_model_add_wavemap_spectrum(mid, libs, wm.data_spec, wm._wset, hp_off, wm.ntrans,
                                                   wm.valid_spectrum_indices, shift_off, wm.interpolation)
            else:
                ctx.ffi_model_add_wavemap(mid, libs, wm.data, wm._wset, hp_off, shift_off,
                                          wm.interpolation)
        if self.geodetic is not None:
            g = self.geodetic
            libs = []
            for v in self.slip_varnames:
                gf = g.gfs[v]
                gf.init_optimization(ctx)
                libs.append(gf.lib_id)
            g._wsets = []
            for n, W, sl in zip(g.sizes, g.weights, g.slog_pdets):
                if np.ndim(W) == 0:
                    g._wsets.append(ctx.weights_create_scalar([float(W)], [sl], n))
                else:
                    g._wsets.append(ctx.weights_create_dense(np.asarray(W), [sl]))
            owned_geo = list(g._wsets)
            hp_off = [lay.offset(n, i) for n, i in g.hypers]
            ctx.ffi_model_add_geodetic(mid, libs, g.data, g.odws, g.sizes, g._wsets, hp_off)
            if g.corrections is not None:
                ctx.ffi_model_add_geodetic_corrections(mid, *correction_tables(g.corrections, g.sizes, lay, g.fixed, kinds=True))
        if self.laplacian is not None:
            L, logdet = self.laplacian
            self._lap = ctx.laplacian_create(L, logdet)
            ctx.ffi_model_set_laplacian(mid, self._lap)
        return LogpForwFunc(ctx, mid, self, return_rvs=return_rvs, wsets=owned_wm, geo_wsets=owned_geo)


class _SharedView(object):
    """Stand-in for the pytensor shared variables the reference exposes through
    ``f.get_shared()`` (sampler/base.py:274-282, 541-555): name/get_value/set_value."""

    def __init__(self, name, getter, setter=None):
        self.name = name
        self._get, self._set = getter, setter

    def get_value(self, borrow=False):
        return self._get()

    def set_value(self, value, borrow=False):
        if self._set is None:
            raise AttributeError("%s is resident in HBM and read-only" % self.name)
        self._set(value)


class LogpForwFunc(object):
    """Duck-type of the compiled ``logp_forw_func`` (sampler/base.py:598-615):
    ``f(q) -> list of arrays``, ``f.trust_input``, ``f.get_shared()``; plus the batched form
    ``f.batch(Q)``.

    The reference function returns every entry of ``model.unobserved_RVs``: the free random
    variables (in the order of q) followed by the deterministics ``seis_like.., geo_like..,
    laplacian_like, like`` (SURVEY Appendix C "Outputs"); traces store that list
    (backend.py:156-173) and ``astep`` reads ``out[_llk_index]``.  ``return_rvs=True`` gives exactly
    that list; the default returns the deterministics block only (the variables are the input).
    Either way ``f._llk_index`` points at ``like``."""

    def __init__(self, ctx, model_id, problem, return_rvs=False, wsets=None, geo_wsets=None):
        self.ctx, self.model_id, self.problem = ctx, model_id, problem
        # the weight sets of THIS model, per wavemap / geodetic dataset (the ids on the shared wavemap / geodetic objects
        # are those of the most recent compile: a second model over the same objects must not free or update ours)
        self._wsets = list(wsets) if wsets is not None else [wm._wset for wm in problem.wavemaps]
        self._geo_wsets = list(geo_wsets) if geo_wsets is not None else list(getattr(problem.geodetic, "_wsets", []) or [])
        self.nllk = ctx.ffi_model_nllk(model_id)
        self.nparams = problem.layout.size
        self.trust_input = True
        self.return_rvs = bool(return_rvs)
        self._polarity = getattr(problem, "polarity", None)
        nblocks = (len(problem.wavemaps) + (problem.geodetic is not None) + (self._polarity is not None)
                   + (problem.laplacian is not None) + 1)
        self._llk_index = nblocks - 1 + (len(problem.layout.varsizes) if self.return_rvs else 0)
        self._dirty = None   # set while a weight update rewrites the HBM library in place

    @property
    def out_names(self):
        """names of the entries of ``f(q)`` (model.unobserved_RVs order)"""
        names = list(self.problem.layout.varsizes) if self.return_rvs else []
        names += ["seis_like_%s" % wm.name if len(self.problem.wavemaps) > 1 else "seis_like"
                  for wm in self.problem.wavemaps]
        if self.problem.geodetic is not None:
            names.append("geo_like")
        if self._polarity is not None:
            names.append("polarity_like")
        if self.problem.laplacian is not None:
            names.append("laplacian_like")
        return names + ["like"]

    def __call__(self, q):
        q = np.ascontiguousarray(q, dtype=np.float64).reshape(1, -1)
        ll = self.batch(q)[0]
        out = []
        if self.return_rvs:
            out += [v.copy() for v in self.problem.layout.rmap(q[0]).values()]
        o = 0
        for wm in self.problem.wavemaps:
            out.append(ll[o:o + wm.n_t].copy())
            o += wm.n_t
        if self.problem.geodetic is not None:
            n = len(self.problem.geodetic.sizes)
            out.append(ll[o:o + n].copy())
            o += n
        if self._polarity is not None:   # a vector, one entry per station of every map (polarity.py:133)
            n = self._polarity.n_t
            out.append(ll[o:o + n].copy())
            o += n
        if self.problem.laplacian is not None:
            out.append(np.array(ll[o]))
            o += 1
        out.append(np.array(ll[o]))
        return out

    def astep_batch(self, Q0, L0, delta, scaling, lower, upper, log_u, beta, accepted=None):
        return self.ctx.ffi_astep_batch(self.model_id, Q0, L0, delta, scaling, lower, upper, log_u,
                                        beta, accepted)

    def mstep_batch(self, Q0, L0, factor, kind, df, seed, step, first_chain, scaling, lower, upper, beta,
                    accepted, accepted_sum=None, n_accepted=None):
        """the whole Metropolis step, proposal draw included, as one device call (metropolis.py:276-422)"""
        return self.ctx.ffi_mstep_batch(self.model_id, Q0, L0, factor, kind, df, seed, step, first_chain,
                                        scaling, lower, upper, beta, accepted, accepted_sum, n_accepted)

    def mstep_batch_grouped(self, Q0, L0, factors, df, seed, step, first_chain, scaling, lower, upper, beta,
                            accepted, accepted_sum=None, n_accepted=None):
        """``mstep_batch`` with one multivariate factor per group of chains (the temperatures of a PT run)"""
        return self.ctx.ffi_mstep_batch_grouped(self.model_id, Q0, L0, factors, df, seed, step, first_chain,
                                                scaling, lower, upper, beta, accepted, accepted_sum, n_accepted)

    def round_libraries_to_f32(self):
        """Float-storage mode (SURVEY 8(f) row 2 "optional fp32 layout"), an explicit and IRREVERSIBLE choice of
        the caller: every seismic library of the model is rounded in HBM to float-representable values
        (``SeismicGFLibrary.round_to_f32``: up to 6e-8 relative; likelihoods move by about that much) and the
        kernels that can read the float copies do so -- half the row traffic, float64 accumulation.  The float64
        storage holds the same rounded values, so small batches and fall-back kernels agree bit for bit.
        Pre-whitened wavemaps are refused: whitened rows are not float-representable and a re-whitening rewrites
        them (the library drops the float copy when its rows are rewritten)."""
        for wm in self.problem.wavemaps:
            if getattr(wm, "is_prewhitened", False):
                raise ValueError("float storage is not offered for a pre-whitened wavemap (%s)" % wm.name)
        for i, wm in enumerate(self.problem.wavemaps):
            for gf in wm.gfs.values():
                gf.round_to_f32(self.ctx)
            self.ctx.ffi_model_set_f32(self.model_id, i, True)

    def set_f32(self, on=True):
        """which kernels read the rows of ALREADY ROUNDED libraries (``round_libraries_to_f32``): the float
        copies (on) or the float64 storage holding the same values (off) -- identical results, a timing choice.
        ``set_f32(False)`` restores nothing: the unrounded values are gone until the library is reloaded."""
        for wm in self.problem.wavemaps:
            for gf in wm.gfs.values():
                if not getattr(gf, "rounded_to_f32", False):
                    raise ValueError("library %s holds unrounded float64 values: float storage has to be chosen "
                                     "explicitly with round_libraries_to_f32() (irreversible)" % gf.filename)
        for i in range(len(self.problem.wavemaps)):
            self.ctx.ffi_model_set_f32(self.model_id, i, on)

    def get_shared(self):
        """the model's shared storage under the reference's access pattern (name / get_value /
        set_value; sampler/base.py:274-282, 541-555 uses it to share memory between workers):
        GF libraries (read-only, HBM resident), observed data, weights and log-determinants."""
        sh = []
        for i, wm in enumerate(self.problem.wavemaps):
            for v, gf in wm.gfs.items():
                sh.append(_SharedView(gf.filename, gf.get_all))
            sh.append(_SharedView("%s_data" % wm.name, lambda wm=wm: wm.data))
            sh.append(_SharedView("%s_weights" % wm.name, lambda wm=wm: wm.weights,
                                  lambda value, i=i: self.update_weights(i, value, self.problem.wavemaps[i].slog_pdet)))
            sh.append(_SharedView("%s_slog_pdet" % wm.name, lambda wm=wm: wm.slog_pdet))
        if self.problem.geodetic is not None:
            g = self.problem.geodetic
            for v, gf in g.gfs.items():
                sh.append(_SharedView(gf.filename, gf.get_all))
            sh.append(_SharedView("geodetic_data", lambda: g.data))
            sh.append(_SharedView("geodetic_odws", lambda: g.odws))
        return sh

    def synthetics(self, Q, wavemap_index=0, residuals=False):
        """synthetics [C, T, N] (or data - synthetics) of one wavemap at the points Q [C, nparams]:
        SeismicComposite.get_synthetics of the distributed-slip composite (seismic.py:1351-1507);
        numpy or torch-cuda in, same kind out"""
        wm = self.problem.wavemaps[wavemap_index]
        T, N = wm.data.shape
        if _is_spectrum(wm):
            # [C, T, M] amplitude spectra of the stacked traces, or data_spec - spectra: the reference's geometry-mode
            # get_synthetics of a spectrum wavemap (seismic.py:932-941)
            N = wm.nsamples_spectrum
        return self.ctx.ffi_synthetics_batch(self.model_id, wavemap_index, Q, T, N, residuals=residuals)

    def start_times(self, Q, chain_bad=None):
        """rupture onset times [C, npatches] at the points Q [C, nparams]: the rupture onset loop of the distributed-slip
        composite (seismic.py:1253-1272) for a batch; chain_bad: see Context.ffi_start_times_batch"""
        return self.ctx.ffi_start_times_batch(self.model_id, Q, self.problem.npatches, chain_bad=chain_bad)

    # -- moment, magnitude and moment-rate functions (csrc/momentrate.hip)
    def _slip_offsets(self, components, what):
        """offsets in q of the named slip variables (None: all of the model's, in its order)"""
        lay = self.problem.layout
        if components is None:
            components = self.problem.slip_varnames
        components = list(components)
        missing = [v for v in components if v not in self.problem.slip_varnames]
        if missing or not components:
            raise ValueError("%s: %s not among the model's slip variables %s"
                             % (what, ", ".join(missing) or "no component", ", ".join(self.problem.slip_varnames)))
        return [lay.offset(v, 0) for v in components]

    def magnitudes(self, Q, moment_per_slip, components=None):
        """(M0, Mw), each (C,), at the points Q (C, nparams): ``FaultGeometry.get_moment`` / ``get_magnitude``
        (ffi/fault.py:284-359) for a batch.  moment_per_slip (npatches,): the moment of every patch at unit slip
        (INTEGRATION.md); components: names of the slip variables the total slip is formed from (None: all of them, as
        ``get_total_slip(components=None)``).  numpy in -> numpy out, torch-cuda in -> tensors."""
        self._ready(Q)
        return self.ctx.ffi_magnitudes_batch(self.model_id, Q, moment_per_slip, self.problem.npatches,
                                             self._slip_offsets(components, "magnitudes"))

    def moment_rates(self, Q, moment_per_slip, deltat, individual=False):
        """moment-rate functions at the points Q (C, nparams): ``FaultGeometry.get_moment_rate_function``
        (ffi/fault.py:361-474) for a batch, on ONE index grid for all draws.  Returns a dict:

          rates   (C, NT) the total, or with ``individual`` (C, nsubfaults + 1, NT): the subfaults, then the total; zero
                  outside a draw's own span; a moment per sample as in the reference
          kbase   index of sample 0;  times (NT,) = (kbase + arange(NT)) * deltat
          spans   (C, nsubfaults + 1, 2) int64: (first index, count) of every subfault's own time axis, the total's last

        The span kernel runs first, one device min / max sizes the grid, then the rate kernel.  The slip is
        sqrt(uparr^2 + uperp^2) as fault.py:412 (the ones the model samples).  numpy in -> numpy out, torch-cuda in ->
        tensors (kbase stays an int).  ValueError: a hypocentre outside the patch grid."""
        self._ready(Q)
        prob = self.problem
        comps = [v for v in ("uparr", "uperp") if v in prob.slip_varnames]
        off = self._slip_offsets(comps, "moment_rates")
        nsub, P = len(prob.n_patch_dip), prob.npatches
        C = int(Q.shape[0])
        tensor_in = hasattr(Q, "data_ptr") and not isinstance(Q, np.ndarray)
        st = self.start_times(Q)                                   # (raises for a flagged draw, as the likelihood's sweep)
        spans = self.ctx.ffi_moment_rate_spans_batch(self.model_id, Q, nsub, P, deltat, start_times=st)
        if C:
            tot = spans[:, nsub]
            kbase, kend = int(tot[:, 0].min()), int((tot[:, 0] + tot[:, 1]).max())
        else:
            kbase, kend = 0, 1
        NT = kend - kbase
        rates = self.ctx.ffi_moment_rates_batch(self.model_id, Q, moment_per_slip, nsub, P, deltat, kbase, NT, comp_off=off,
                                                start_times=st)
        idx = np.arange(NT, dtype=np.float64)
        times = (float(kbase) + idx) * float(deltat)
        if tensor_in:
            import torch
            times = torch.from_numpy(times).to(Q.device)
        return dict(rates=rates if individual else rates[:, nsub], kbase=kbase, times=times, spans=spans)

    def release(self):
        """free what this compiled model holds on the device BESIDES the libraries: the model record and the weight sets
        (a dense set is T x N x N doubles: 8.6 GB at config 3).  The function cannot be called afterwards.  Explicit, not
        a finaliser: wavemap objects may be shared between models."""
        if self.model_id is None:
            return
        self.ctx.ffi_model_destroy(self.model_id)
        self.model_id = None
        for wm, ws in zip(self.problem.wavemaps, self._wsets):
            if ws is not None:
                self.ctx.weights_destroy(ws)
                if wm._wset == ws:
                    wm._wset = None
            if getattr(wm, "_whitened_with", None) is not None:
                wm._whitened_with = None
        self._wsets = [None] * len(self._wsets)
        g = self.problem.geodetic
        for ws in self._geo_wsets:
            self.ctx.weights_destroy(ws)
        if g is not None and list(getattr(g, "_wsets", [])) == self._geo_wsets:
            g._wsets = []
        self._geo_wsets = []

    def batch(self, Q, out=None):
        """Q (C, nparams) numpy or torch-cuda -> LL (C, nllk)"""
        if self.model_id is None:
            raise RuntimeError("this compiled model was released")
        if Q.shape[-1] != self.nparams:
            raise ValueError("expected %d parameters, got %d" % (self.nparams, Q.shape[-1]))
        if self._dirty:
            raise RuntimeError("a weight update of this model did not complete: %s" % self._dirty)
        return self.ctx.ffi_logp_batch(self.model_id, Q, self.nllk, out)

    @property
    def nterm(self):
        """columns of ``update_llks``: seismic datasets, geodetic datasets, one per slip variable of the Laplacian"""
        return self.ctx.ffi_model_nterm(self.model_id)

    def update_llks(self, Q, out=None):
        """the hyper model's cached misfits at the points Q (C, nparams) -> (C, nterm): ``update_llks`` of every
        composite (seismic.py:510-525, geodetic.py:429-444, laplacian.py:141-154) for a batch of chains -- the
        quadratic forms |W r|^2 the likelihood hands to its epilogues, from the same kernels (the geodetic ones with
        the odw factor, unlike the reference's: DESIGN.md).  The hyper-parameter entries of Q are not read.  numpy in
        -> numpy out, torch-cuda in -> tensor on the same device."""
        refuse_polarity(self.problem, "update_llks")
        if self.model_id is None:
            raise RuntimeError("this compiled model was released")
        if Q.shape[-1] != self.nparams:
            raise ValueError("expected %d parameters, got %d" % (self.nparams, Q.shape[-1]))
        if self._dirty:
            raise RuntimeError("a weight update of this model did not complete: %s" % self._dirty)
        return self.ctx.ffi_llks_batch(self.model_id, Q, out)

    # -- polarity composite (csrc/polarity.hip)
    def _polarity_or_raise(self, Q):
        self._ready(Q)
        if self._polarity is None:
            raise ValueError("the model has no polarity composite")
        return self._polarity

    def moment_tensors(self, Q):
        """Q (C, nparams) -> (C, 6): the normalised (mnn, mee, mdd, mne, mnd, med) of every row -- the tensor that
        ``heart.pol_synthetics`` multiplies with the propagation coefficients (heart.py:4086-4088) -- by the kernel of
        the likelihood.  numpy in -> numpy out, torch-cuda in -> tensor."""
        pol = self._polarity_or_raise(Q)
        from ..polarity_binding import mt6_batch
        return mt6_batch(self.ctx, Q, pol.source_kind, *pol.source_tables())

    def polarity_synthetics(self, Q):
        """Q (C, nparams) -> (C, n_t): ``heart.pol_synthetics`` of every row at the stations of all polarity maps,
        map by map (``PolarityComposite.get_synthetics(order="list")``, polarity.py:261-291)"""
        pol = self._polarity_or_raise(Q)
        from ..polarity_binding import polarity_amplitudes_batch
        return polarity_amplitudes_batch(self.ctx, Q, pol.source_kind, *pol.source_tables(), rw=pol.radiation_weights())

    # -- posterior diagnostics of a population (csrc/summary.hip)
    def _ready(self, Q=None):
        if self.model_id is None:
            raise RuntimeError("this compiled model was released")
        if Q is not None and Q.shape[-1] != self.nparams:
            raise ValueError("expected %d parameters, got %d" % (self.nparams, Q.shape[-1]))
        if self._dirty:
            raise RuntimeError("a weight update of this model did not complete: %s" % self._dirty)

    @property
    def ndata(self):
        """datasets of the model: the seismic datasets wavemap by wavemap, then the geodetic ones"""
        g = self.problem.geodetic
        return sum(wm.n_t for wm in self.problem.wavemaps) + (len(g.sizes) if g is not None else 0)

    @property
    def dataset_names(self):
        """column labels of ``variance_reductions`` / ``obs_quads``"""
        return list(self.problem.out_names[:self.ndata])

    @property
    def dataset_nsamples(self):
        """samples per dataset, in the order of ``dataset_names``: N of a time-domain wavemap, M = hi - lo of a spectrum
        wavemap, the size of a geodetic dataset"""
        g = self.problem.geodetic
        n = [int(getattr(wm, "nsamples", wm.data.shape[1])) for wm in self.problem.wavemaps for _ in range(wm.n_t)]
        return n + ([int(s) for s in g.sizes] if g is not None else [])

    def obs_quads(self):
        """|W_k d_k|^2 per dataset -> (ndata,) numpy: the denominators ``data.T.dot(icov).dot(data)`` of the variance
        reduction (seismic.py:612-616, geodetic.py:497-501; geodetic data with its odw factor: DESIGN.md 3.9).  Cached
        on the device model until weights, data or corrections change."""
        refuse_polarity(self.problem, "obs_quads")
        self._ready()
        return self.ctx.ffi_obs_quads(self.model_id, self.ndata)

    def variance_reductions(self, Q, out=None):
        """Q (C, nparams) -> (C, ndata): ``1 - nom / denom`` per dataset (columns: ``dataset_names``) and draw --
        ``get_variance_reductions`` (seismic.py:564-634, geodetic.py:446-511) for a batch, as a fraction (the
        reference's plots multiply by 100).  The hyper-parameter entries of Q are not read: ``inverse(exp(2h))``
        scales numerator and denominator alike.  numpy in -> numpy out, torch-cuda in -> tensor on the same device."""
        refuse_polarity(self.problem, "variance_reductions")
        self._ready(Q)
        return self.ctx.ffi_variance_reductions_batch(self.model_id, Q, self.ndata, out)

    def geodetic_residuals(self, Q, residuals=True):
        """Q (C, nparams) -> (C, nobs_total): the geodetic composite's residual ``(d - mu) * odw - corrections`` in the
        order of geodetic.py:1072-1077 (residuals=False: its synthetics mu); FFI and geometry composites"""
        self._ready(Q)
        g = self.problem.geodetic
        if g is None:
            raise ValueError("the model has no geodetic composite")
        return self.ctx.ffi_geo_residuals_batch(self.model_id, Q, int(sum(g.sizes)), residuals=residuals)

    # -- lsq start (csrc/lsq.hip)
    def _lsq_setup(self, Q=None):
        """the checks of DistributionOptimizer.lsq_solution (problems.py:768-787) and the model's inverted variable"""
        refuse_spectrum_wavemaps(self.problem, "the least-squares start")
        refuse_polarity(self.problem, "the least-squares start")
        self._ready(Q)
        prob = self.problem
        if prob.laplacian is None:
            raise ValueError("Least-squares- solution for distributed slip is only "
                             "available with laplacian regularization!")
        inverted = [v for v in ("uparr", "utens") if v in prob.slip_varnames]
        if len(inverted) != 1:
            raise ValueError("LSQ distributed slip solution inverts for exactly one of uparr, utens; the sampled slip "
                             "variables are %s (the reference's stacking of its blocks is shape-consistent for one only)"
                             % ", ".join(prob.slip_varnames))
        for wm in prob.wavemaps:
            if getattr(wm, "is_prewhitened", False):
                raise ValueError("wavemap %s is pre-whitened: its rows and data hold W.G and W.d, the least-squares "
                                 "start is defined on the unweighted ones" % wm.name)
        others = [v for v in prob.slip_varnames if v != inverted[0]]
        if others not in ([], ["uperp"]):
            raise ValueError("LSQ distributed slip solution: besides %s only uperp may be sampled, got %s"
                             % (inverted[0], ", ".join(others)))
        key = (prob.slip_varnames.index(inverted[0]), prob.slip_varnames.index("uperp") if others else -1)
        if getattr(self, "_lsq_vars", None) != key:
            self.ctx.ffi_model_set_lsq_variables(self.model_id, *key)
            self._lsq_vars = key
        return inverted[0]

    def lsq_normal_equations(self, Q, chain_bad=None):
        """Q (C, nparams) -> N (C, P, P), b (C, P): the normal equations A^T A, A^T d of the linear problem that
        ``lsq_solution`` solves per chain, A and d in the order seismic (wavemap, target, sample), geodetic, laplacian
        (``include/beat_amd.h``).  numpy in -> numpy out, torch-cuda in -> tensors.  A chain whose times leave the library
        grid raises IndexError (chain_bad, int32 (C,), is filled first)."""
        self._lsq_setup(Q)
        return self.ctx.ffi_lsq_normal_batch(self.model_id, Q, self.problem.npatches, chain_bad=chain_bad)

    def lsq_solution(self, Q, return_info=False):
        """``DistributionOptimizer.lsq_solution`` (problems.py:753-873) for a batch: Q (C, nparams) -> Q with the inverted
        slip variable (uparr or utens) replaced by the non-negative least-squares slip at the chain's kinematics and uperp,
        where sampled, by zeros; every other column bit for bit the input.  The solution is not clipped to the prior box
        (nor is the reference's).  return_info: also the iteration counts and status words (C,)."""
        self._lsq_setup(Q)
        out, it, st = self.ctx.ffi_lsq_solution_batch(self.model_id, Q)
        stat = _host(st)
        if np.any(stat == 1):
            raise RuntimeError("Maximum number of iterations reached.")
        if np.any(stat == 2):
            raise ValueError("lsq_solution: the normal equations of chain(s) %s are not finite or not positive definite"
                             % np.nonzero(stat == 2)[0].tolist())
        return (out, it, st) if return_info else out

    def _hp_columns(self, Q, hypers):
        offs = [self.problem.layout.offset(n, i) for n, i in hypers]
        if hasattr(Q, "data_ptr") and not isinstance(Q, np.ndarray):
            import torch
            return Q[:, torch.as_tensor(offs, device=Q.device)].contiguous()
        return np.ascontiguousarray(np.asarray(Q)[:, offs])

    def standardized_residuals(self, Q, covariances, wavemap_index=0):
        """``get_standardized_residuals`` (seismic.py:527-562, geodetic.py:513-543) for a batch: per dataset
        ``inv(cov.chol(exp(2 h))) . residual`` = ``exp(-h) * inv(cov.chol()) . residual``.

        covariances: the datasets' ``beat_amd.heart.Covariance`` objects (or plain variances sigma^2); the operators
        ``inv(cov.chol())`` are formed on the host once per call -- they are lower triangular and are NOT the
        whitening operators ``chol_inverse`` the likelihood holds (same norm of the product, other elements).
        h is read from Q as the model reads it (per dataset or shared).
        wavemap_index: a wavemap -> (C, T, N); "geodetic" -> list of (C, n_k) per dataset (the sizes differ).
        A pre-whitened wavemap is refused: its residuals are whitened by another operator already."""
        refuse_polarity(self.problem, "standardized_residuals")
        if wavemap_index != "geodetic":
            refuse_spectrum_wavemaps(self.problem, "standardized_residuals", wavemap_index)
        self._ready(Q)
        if wavemap_index == "geodetic":
            g = self.problem.geodetic
            if g is None:
                raise ValueError("the model has no geodetic composite")
            if len(covariances) != len(g.sizes):
                raise ValueError("%d covariances for %d geodetic datasets" % (len(covariances), len(g.sizes)))
            res = self.geodetic_residuals(Q)
            hp = self._hp_columns(Q, g.hypers)
            out, o = [], 0
            for k, n in enumerate(g.sizes):
                S = _standardizing_operators([covariances[k]], n)
                r = res[:, o:o + n].reshape(-1, 1, n)
                r = r.contiguous() if hasattr(r, "contiguous") else np.ascontiguousarray(r)
                h = hp[:, k:k + 1]
                h = h.contiguous() if hasattr(h, "contiguous") else np.ascontiguousarray(h)
                out.append(self.ctx.standardize_batch(S, r, h).reshape(-1, n))
                o += n
            return out
        wm = self.problem.wavemaps[wavemap_index]
        if getattr(wm, "is_prewhitened", False):
            raise ValueError("wavemap %s is pre-whitened: its residuals are W (d - s) already, the standardizing "
                             "operator inv(chol(C)) does not apply to them" % wm.name)
        T, N = wm.data.shape
        if len(covariances) != T:
            raise ValueError("%d covariances for %d datasets" % (len(covariances), T))
        S = _standardizing_operators(covariances, N)
        return self.ctx.standardize_batch(S, self.synthetics(Q, wavemap_index, residuals=True),
                                          self._hp_columns(Q, wm.hypers))

    def update_weights(self, wavemap_index, weights, slog_pdet):
        """seismic.py:1509-1534 update_weights: new chol_inverse + slog_pdet per dataset.  Kind
        and size must match the uploaded set (checked by the library).  numpy arrays or torch-cuda
        tensors (the per-stage covariance update keeps them on the device).

        Pre-whitened wavemaps are re-whitened IN PLACE through the chain of ratios M = W_new . inv(W_old); a RESUMED run
        (smc_sample(resume_stage=...)) installs the saved stage's weights by whitening from the operator it was compiled
        with instead of replaying that chain, so the restored likelihoods agree with the saved ones to rounding
        (~1e-12 relative), not bit for bit."""
        import torch
        wm = self.problem.wavemaps[wavemap_index]
        T, N = wm.data.shape
        if _is_spectrum(wm):
            N = wm.nsamples_spectrum     # the operators of a spectrum wavemap act on its M = hi - lo spectrum samples
        on_dev = torch.is_tensor(weights) and weights.is_cuda
        if on_dev:
            w = weights.contiguous()
            sl = (slog_pdet if torch.is_tensor(slog_pdet) else torch.from_numpy(np.asarray(slog_pdet))).to(w.device)
            sl = sl.double().reshape(-1).contiguous()
        else:
            w = np.ascontiguousarray(weights, dtype=np.float64)
            sl = np.ascontiguousarray(slog_pdet, dtype=np.float64).ravel()
        if getattr(wm, "is_prewhitened", False):
            # The old operator is folded into the library rows and the data: rows . W_new^T =
            # (rows . W_old^T) . M^T with M = W_new . inv(W_old) (upper triangular, solved on the
            # device), applied in place -- no copy of the unwhitened library is needed.
            if tuple(w.shape) != (T, N, N) or tuple(sl.shape) != (T,):
                raise ValueError("a pre-whitened wavemap takes dense weights (%d,%d,%d) and slog_pdet (%d,)"
                                 % (T, N, N, T))
            dev = torch.device("cuda", self.ctx.device)
            wd = w if on_dev else torch.from_numpy(w).to(dev)
            old = wm._whitened_with
            old = old if torch.is_tensor(old) else upload(old, dev)
            # M is computed and checked (a singular old operator raises here) BEFORE any row is touched
            M = self.ctx.whitening_ratio_batch(wd, old)
            self.ctx.synchronize()
            self._dirty = "re-whitening of wavemap %d was interrupted" % wavemap_index
            seen = set()   # (two slip components may share one adopted tensor: whiten it once)
            for gf in wm.gfs.values():
                if gf._device_tensor.data_ptr() in seen:
                    continue
                seen.add(gf._device_tensor.data_ptr())
                self.ctx.whiten_rows_batch(gf._device_tensor.view(T, -1, N), M)
            d = upload(wm.data, dev)
            self.ctx.whiten_rows_batch(d.view(T, 1, N), M)
            self.ctx.ffi_model_update_data(self.model_id, wavemap_index, d)
            self.ctx.weights_update(self._wsets[wavemap_index], np.ones(T), sl)
            self.ctx.synchronize()
            #  M (T x N x N, 8.6 GB at config 3) and the old operator go before the new one is kept: the peak
            # next to the libraries is then two operators (new + M), not three.  The operator stays on the device because
            # the next update needs it at once; release() / a dead wavemap frees it.
            del M, old
            wm.data, wm.slog_pdet, wm._whitened_with = d.cpu().numpy(), _host(sl), wd
            self._dirty = None
            return
        if tuple(w.shape) not in ((T,), (T, N, N)) or tuple(sl.shape) != (T,):
            raise ValueError("weights must be (%d,) or (%d,%d,%d) and slog_pdet (%d,)" % (T, T, N, N, T))
        self.ctx.weights_update(self._wsets[wavemap_index], w, sl)
        if len(tuple(w.shape)) == 3:
            _log_band(self.ctx, self._wsets[wavemap_index], "wavemap %d (update)" % wavemap_index)
        wm.weights, wm.slog_pdet = w, _host(sl)

    def update_geodetic_weights(self, weights, slog_pdets):
        """geodetic.py:1197-1202: new ``chol_inverse`` (an (n_i, n_i) operator, or a scalar where the dataset was compiled
        with one) and log-determinant per geodetic dataset, numpy or torch-cuda.  Kind and size must match the dataset's
        weight set (checked here and by the library); every operator is checked before the first is installed.  The
        cached |W d|^2 of the diagnostics go with the weights (``beatamd_weights_update``)."""
        import torch
        self._ready()
        g = self.problem.geodetic
        if g is None:
            raise ValueError("the model has no geodetic composite")
        nd = len(g.sizes)
        weights = list(weights)
        slog = [float(s) for s in np.ravel(_host(slog_pdets) if torch.is_tensor(slog_pdets) else
                                           [_host(s) for s in slog_pdets])]
        if len(weights) != nd or len(slog) != nd:
            raise ValueError("%d weights and %d log-determinants for %d geodetic datasets" % (len(weights), len(slog), nd))
        new = []
        for k, (n, W, old) in enumerate(zip(g.sizes, weights, g.weights)):
            if torch.is_tensor(W) and W.is_cuda:
                w = W.detach().double().contiguous()
            else:
                w = np.ascontiguousarray(_host(W), dtype=np.float64)
            dense = np.ndim(old) != 0
            want = (n, n) if dense else ()
            if tuple(w.shape) == (1,) + want:
                w = w.reshape(want)
            if tuple(w.shape) != want:
                raise ValueError("geodetic dataset %d holds %s weights: expected shape %s, got %s"
                                 % (k, "dense" if dense else "scalar", want, tuple(w.shape)))
            new.append(w.reshape((1, n, n) if dense else (1,)))
        for ws, w, sl in zip(self._geo_wsets, new, slog):
            self.ctx.weights_update(ws, w, np.array([sl]))
        g.weights = [w[0] if w.ndim == 3 else float(w[0]) for w in new]
        g.slog_pdets = slog


def _log_band(ctx, wset, what):
    """once per weights_create / weights_update of a dense set: how the library evaluates it (the
    banded evaluation is chosen by a device scan -- say so where the user can see it)"""
    band, dropped = ctx.weights_band_info(wset)
    if band >= 0:
        logger.info("%s: whitening operators evaluated on their band (half bandwidth %d; largest entry beyond it %.3g of its "
                    "row's largest; BEATAMD_QF_BAND=0 keeps the dense kernel)", what, band, dropped)
    else:
        logger.info("%s: dense whitening operators (FP64 matrix-core kernel)", what)


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else a


def _is_spectrum(wm):
    return getattr(wm, "domain", "time") == "spectrum"


# why each of these stops at a spectrum-domain wavemap (refuse_spectrum_wavemaps)
_SPECTRUM_REASONS = {
    "the least-squares start": "the amplitude is taken after the stack, the problem is not linear in the slips",
    "standardized_residuals": "the standardizing operators of amplitude-spectrum residuals are a follow-up",
    "NoiseCovarianceUpdate": "the spectral noise-covariance estimate (covariance.py:366-373) is a follow-up",
    "TargetShardedLogp": "sharding the targets of a spectrum wavemap over ranks is a follow-up",
}


def refuse_spectrum_wavemaps(problem, what, wavemap_index=None):
    """NotImplementedError naming the spectrum domain if ``problem`` has a spectrum wavemap (wavemap_index: that one alone);
    a host check in front of any device call"""
    wms = list(getattr(problem, "wavemaps", []))
    for wm in wms if wavemap_index is None else [wms[wavemap_index]]:
        if _is_spectrum(wm):
            raise NotImplementedError("%s is not available for wavemap %s in the spectrum domain: %s"
                                      % (what, wm.name, _SPECTRUM_REASONS[what]))


def refuse_polarity(problem, what):
    """NotImplementedError if ``problem`` has a polarity composite: a host check in front of any device call"""
    if getattr(problem, "polarity", None) is not None:
        raise NotImplementedError("%s is not available for a model with a polarity composite: the reference defines no "
                                  "Gaussian misfit for it (beat/models/polarity.py has no update_llks, variance "
                                  "reduction or standardized residual)" % what)


def _standardizing_operators(covariances, n):
    """S_t = inv(cov_t.chol()) of datasets of n samples (seismic.py:560): (T,) = 1 / sigma_t when every covariance is a
    plain variance sigma^2, else (T, n, n), lower triangular"""
    if all(np.ndim(c) == 0 and not hasattr(c, "chol") for c in covariances):
        return 1.0 / np.sqrt(np.asarray(covariances, dtype=np.float64))
    S = np.empty((len(covariances), n, n))
    for t, c in enumerate(covariances):
        if hasattr(c, "chol"):
            L = np.asarray(c.chol(), dtype=np.float64)
            if L.shape != (n, n):
                raise ValueError("covariance %d is %s, the dataset has %d samples" % (t, L.shape, n))
            S[t] = np.linalg.inv(L)
        else:
            S[t] = np.eye(n) / np.sqrt(float(c))
    return S


def prior_logp_func(lower, upper):
    """metropolis.py:176-181: with Uniform priors and no transform the prior logp is a
    constant inside the box and -inf outside."""
    lower, upper = np.asarray(lower), np.asarray(upper)
    const = -np.sum(np.log(np.where(upper > lower, upper - lower, 1.0)))

    def f(q):
        q = np.asarray(q)
        inside = np.all((q >= lower) & (q <= upper))
        return np.array(const if inside else -np.inf)

    return f
