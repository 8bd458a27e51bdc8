"""
Thin object layer over the C ABI: one :class:`Context` per (process, GPU).

Arrays may be numpy arrays (host; results come back as numpy) or torch CUDA tensors
(device; results are torch tensors on the same device, the call is asynchronous on the
context stream).  PyTorch is only plumbing here (device memory, streams); all arithmetic
is in ``libbeat_amd.so``.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import INTERPOLATIONS, check, ptr
from ._marshal import as_input, checked, is_canonical, is_dev, new, on_side, upload


def _interp(interpolation):
    if interpolation not in INTERPOLATIONS:
        raise NotImplementedError("Interpolation scheme %s not implemented!" % interpolation)
    return INTERPOLATIONS[interpolation]


class Context(object):
    """Owns the HBM-resident state of one GPU: GF libraries, weights, models, scratch."""

    def __init__(self, device=0):
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.beatamd_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._lib.beatamd_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _adopt_stream(self, *arrays):
        """Device tensors are produced on torch's current stream: launch there too, so the
        kernels are ordered after their producers without an explicit synchronisation."""
        for a in arrays:
            if is_dev(a):
                import torch
                s = torch.cuda.current_stream(self.device).cuda_stream
                if s != getattr(self, "_stream", None):
                    check(self._lib.beatamd_ctx_set_stream(self._h, C.c_void_p(s)))
                    self._stream = s
                return

    def _q_out(self, Q, out, tail):
        """the opening of every Q -> out call: launch on Q's stream; -> (Q as the library reads it, its chains, ``out`` or
        -- for None -- a new (chains,) + tail array on Q's side).  tail may be a function of the converted Q; a caller's
        ``out`` is handed on as it is"""
        self._adopt_stream(Q)
        Q = as_input(Q)
        Cn = int(Q.shape[0])
        if out is None:
            out = new(Q, (Cn,) + (tail(Q) if callable(tail) else tail))
        return Q, Cn, out

    def use_torch_stream(self):
        """Launch on torch's current stream of this device (so torch ops interleave in order)."""
        import torch
        s = torch.cuda.current_stream(self.device).cuda_stream
        check(self._lib.beatamd_ctx_set_stream(self._h, C.c_void_p(s)))
        self._stream = s

    def set_stream(self, stream_ptr):
        """stream_ptr 0 / None = the HIP null stream (torch's default stream)"""
        check(self._lib.beatamd_ctx_set_stream(self._h, C.c_void_p(stream_ptr or 0)))
        self._stream = stream_ptr or 0

    def use_own_stream(self):
        check(self._lib.beatamd_ctx_use_own_stream(self._h))
        self._stream = None

    def synchronize(self):
        check(self._lib.beatamd_ctx_synchronize(self._h))

    def set_step_counter(self, counter):
        """counter: torch int32 tensor (1,) on the device, or None -- see beatamd_ctx_set_step_counter"""
        check(self._lib.beatamd_ctx_set_step_counter(self._h, ptr(counter) if counter is not None else None))

    def enable_timing(self, on=True):
        check(self._lib.beatamd_ctx_enable_timing(self._h, int(bool(on))))

    def reset_timing(self):
        check(self._lib.beatamd_ctx_reset_timing(self._h))

    def kernel_time(self, name):
        """-> (total_ms, launches) measured with HIP events on the launch stream"""
        ms, n = C.c_double(), C.c_int64()
        check(self._lib.beatamd_ctx_kernel_time(self._h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # -- fast sweep
    def fast_sweep_batch(self, slowness, patch_size, h_strk, h_dip, num_strk, num_dip):
        self._adopt_stream(slowness)
        slowness = as_input(slowness)
        n = int(num_strk) * int(num_dip)
        Cn = int(slowness.shape[0]) if slowness.ndim == 2 else 1
        if slowness.ndim == 1:
            slowness = slowness.reshape(1, -1)
        if slowness.shape[1] != n:
            raise ValueError("slowness has %d entries per chain, grid has %d" % (slowness.shape[1], n))
        hs, hd = as_input(h_strk, np.int32), as_input(h_dip, np.int32)
        out = new(slowness, (Cn, n))
        check(self._lib.beatamd_fast_sweep_batch(self._h, ptr(slowness), float(patch_size), ptr(hs),
                                                 ptr(hd), int(num_strk), int(num_dip), Cn, ptr(out)))
        return out

    # -- seismic GF library
    def seis_gflib_create(self, dims, starttime_min, starttime_sampling, duration_min,
                          duration_sampling):
        T, P, D, S, N = [int(d) for d in dims]
        lid = C.c_int32()
        check(self._lib.beatamd_seis_gflib_create(self._h, T, P, D, S, N, float(starttime_min),
                                                  float(starttime_sampling), float(duration_min),
                                                  float(duration_sampling), C.byref(lid)))
        return lid.value

    def seis_gflib_set_split_targets(self, lib_id, ntargets):
        check(self._lib.beatamd_seis_gflib_set_split_targets(self._h, lib_id, int(ntargets)))

    def seis_gflib_upload(self, lib_id, array, offset=0):
        a = as_input(array)
        count = int(a.numel()) if is_dev(a) else int(a.size)
        check(self._lib.beatamd_seis_gflib_upload(self._h, lib_id, ptr(a), int(offset), count))

    def seis_gflib_adopt(self, lib_id, device_tensor):
        self._adopt_stream(device_tensor)
        check(self._lib.beatamd_seis_gflib_adopt(self._h, lib_id, ptr(device_tensor)))

    def seis_gflib_round_to_f32(self, lib_id):
        """float copy of the library + the float64 storage rounded to the same values"""
        check(self._lib.beatamd_seis_gflib_round_to_f32(self._h, lib_id))

    def ffi_model_set_f32(self, model_id, wavemap_index, on=True):
        check(self._lib.beatamd_ffi_model_set_f32(self._h, model_id, int(wavemap_index), 1 if on else 0))

    def seis_gflib_device_ptr(self, lib_id):
        p = C.c_void_p()
        check(self._lib.beatamd_seis_gflib_device_ptr(self._h, lib_id, C.byref(p)))
        return p.value

    def seis_gflib_destroy(self, lib_id):
        check(self._lib.beatamd_seis_gflib_destroy(self._h, lib_id))

    def seis_stack_all_batch(self, lib_id, dims, durations, starttimes, slips,
                             interpolation="nearest_neighbor"):
        self._adopt_stream(durations, starttimes, slips)
        T, P, D, S, N = dims
        it = _interp(interpolation)
        du, st, sl = as_input(durations), as_input(starttimes), as_input(slips)
        Cn = int(du.shape[0])
        if tuple(du.shape) != (Cn, P) or tuple(sl.shape) != (Cn, P) or tuple(st.shape) != (Cn, T, P):
            raise ValueError("stack_all_batch: expected durations/slips (C,%d) and starttimes (C,%d,%d)"
                             % (P, T, P))
        out = new(du, (Cn, T, N))
        check(self._lib.beatamd_seis_stack_all_batch(self._h, lib_id, Cn, ptr(du), ptr(st), ptr(sl), it,
                                                     ptr(out)))
        return out

    # -- geodetic GF library
    def geo_gflib_create(self, G):
        G = as_input(G)
        lid = C.c_int32()
        check(self._lib.beatamd_geo_gflib_create(self._h, int(G.shape[0]), int(G.shape[1]), ptr(G),
                                                 C.byref(lid)))
        return lid.value

    def geo_gflib_destroy(self, lib_id):
        check(self._lib.beatamd_geo_gflib_destroy(self._h, lib_id))

    def geo_stack_all_batch(self, lib_id, nobs, slips, out=None):
        acc = out is not None
        sl, Cn, out = self._q_out(slips, out, (nobs,))
        check(self._lib.beatamd_geo_stack_all_batch(self._h, lib_id, Cn, ptr(sl), int(acc), ptr(out)))
        return out

    # -- velocity-model prediction covariance (csrc/predcov.hip)
    def geo_ensemble_create(self, lib_ids, K, nvar):
        """the libraries of K crust-model variants for nvar slip variables (ids of geo_gflib_create, variant-major
        (K, nvar)); all of one shape"""
        ids = np.ascontiguousarray(lib_ids, dtype=np.int32).ravel()
        if ids.size != int(K) * int(nvar):
            raise ValueError("geo_ensemble_create: %d library ids for %d variants of %d variables" % (ids.size, K, nvar))
        eid = C.c_int32()
        check(self._lib.beatamd_geo_ensemble_create(self._h, ptr(ids), int(K), int(nvar), C.byref(eid)))
        return eid.value

    def geo_ensemble_destroy(self, ens_id):
        check(self._lib.beatamd_geo_ensemble_destroy(self._h, ens_id))

    def geo_ensemble_stack(self, ens_id, K, nobs, slips):
        """slips (nvar * P,) at one point -> X (K, nobs): the synthetics of every variant (geodetic.py:1167-1176);
        numpy or torch-cuda in, same kind out"""
        self._adopt_stream(slips)
        sl = as_input(slips)
        X = new(sl, (int(K), int(nobs)))
        check(self._lib.beatamd_geo_ensemble_stack(self._h, ens_id, ptr(sl), ptr(X)))
        return X

    def pred_covariance_batch(self, X, sizes, base=None, out=None):
        """X (K, Nobs) -> list of (n_i, n_i): base_i + numpy.cov(X[:, o_i:o_i + n_i], rowvar=0) per dataset, in the fixed
        order of k_pred_center / k_pred_cov (tests/predcov_ref.py restates it bit for bit).  base: None or a list whose
        entries are None (zeros) or contiguous float64 (n_i, n_i) arrays on either side; out: None (allocated on X's
        side) or such a list, written in place."""
        self._adopt_stream(X)
        x = as_input(X)
        if x.ndim != 2:
            raise ValueError("pred_covariance_batch: X must be (K, Nobs)")
        K, nobs = int(x.shape[0]), int(x.shape[1])
        n = as_input(sizes, np.int64).ravel()
        nd = int(n.size)
        base = [None] * nd if base is None else list(base)
        if out is None:
            out = [new(x, (int(k), int(k))) for k in n]
        out = list(out)
        if len(base) != nd or len(out) != nd:
            raise ValueError("pred_covariance_batch: %d sizes, %d base and %d output matrices" % (nd, len(base), len(out)))
        for i, k in enumerate(n):
            for a, what in ((base[i], "base"), (out[i], "out")):
                if a is not None and not is_canonical(a, np.float64, (int(k), int(k))):
                    raise ValueError("pred_covariance_batch: %s[%d] must be a contiguous float64 (%d, %d) array"
                                     % (what, i, k, k))
        if any(o is None for o in out):
            raise ValueError("pred_covariance_batch: every dataset needs an output matrix")
        pb = (C.c_void_p * max(nd, 1))(*[ptr(b) for b in base])
        po = (C.c_void_p * max(nd, 1))(*[ptr(o) for o in out])
        check(self._lib.beatamd_pred_covariance_batch(self._h, K, nobs, ptr(x), nd, ptr(n), C.addressof(pb), C.addressof(po)))
        return out

    # -- weights / likelihood
    def weights_create_scalar(self, w, slog_pdet, M):
        w, sl = as_input(w).ravel(), as_input(slog_pdet).ravel()
        wid = C.c_int32()
        check(self._lib.beatamd_weights_create(self._h, _lib.W_SCALAR, int(w.size), int(M), ptr(w),
                                               ptr(sl), C.byref(wid)))
        return wid.value

    def weights_create_dense(self, W, slog_pdet):
        W, sl = as_input(W), as_input(slog_pdet).ravel()
        if W.ndim == 2:
            W = W.reshape((1,) + W.shape)
        nd, M, M2 = W.shape
        if M != M2:
            raise ValueError("weights must be square")
        wid = C.c_int32()
        check(self._lib.beatamd_weights_create(self._h, _lib.W_DENSE, int(nd), int(M), ptr(W), ptr(sl),
                                               C.byref(wid)))
        return wid.value

    def weights_update(self, wset_id, weights, slog_pdet):
        """new weights of an existing set; scalar (nd,) or dense (nd, M, M) -- kind and size are
        checked against the set by the library"""
        W, sl = as_input(weights), as_input(slog_pdet).ravel()
        kind = _lib.W_DENSE if W.ndim >= 2 else _lib.W_SCALAR
        count = int(W.numel()) if is_dev(W) else int(W.size)
        check(self._lib.beatamd_weights_update(self._h, wset_id, kind, count, ptr(W), ptr(sl)))

    def weights_band(self, wset_id):
        """half bandwidth a dense weight set is evaluated on (banded upper-triangular whitening operators, e.g. the
        bidiagonal ones of the reference's "exponential" noise structure), -1: the dense kernel"""
        b = C.c_int64()
        check(self._lib.beatamd_weights_band(self._h, wset_id, C.byref(b)))
        return b.value

    def weights_band_info(self, wset_id):
        """-> (half bandwidth or -1, largest entry beyond the band relative to the largest entry of its row): what the banded
        evaluation of this weight set leaves out (<= 2^-40 by construction)"""
        b, d = C.c_int64(), C.c_double()
        check(self._lib.beatamd_weights_band_info(self._h, wset_id, C.byref(b), C.byref(d)))
        return b.value, d.value

    def weights_destroy(self, wset_id):
        check(self._lib.beatamd_weights_destroy(self._h, wset_id))

    def mvn_chol_logp_batch(self, wset_id, residuals, hp):
        self._adopt_stream(residuals, hp)
        r, h = as_input(residuals), as_input(hp)
        Cn, nd = int(r.shape[0]), int(r.shape[1])
        out = new(r, (Cn, nd))
        check(self._lib.beatamd_mvn_chol_logp_batch(self._h, wset_id, Cn, ptr(r), ptr(h), ptr(out)))
        return out

    def laplacian_create(self, L, logdet):
        L = as_input(L)
        lid = C.c_int32()
        check(self._lib.beatamd_laplacian_create(self._h, int(L.shape[0]), ptr(L), float(logdet),
                                                 C.byref(lid)))
        return lid.value

    def laplacian_destroy(self, lap_id):
        check(self._lib.beatamd_laplacian_destroy(self._h, lap_id))

    def laplacian_logp_batch(self, lap_id, slips, hp):
        self._adopt_stream(slips, hp)
        s, h = as_input(slips), as_input(hp)
        Cn, nvar = int(s.shape[0]), int(s.shape[1])
        out = new(s, (Cn,))
        check(self._lib.beatamd_laplacian_logp_batch(self._h, lap_id, Cn, nvar, ptr(s), ptr(h), ptr(out)))
        return out

    # -- noise covariance estimation
    def autocovariance_batch(self, data):
        d = as_input(data)
        self._adopt_stream(d)
        # device traces: the kernel takes each row's mean in numpy's summation order (torch.mean sums in another
        # order and moved the result in the last bits); host traces: numpy's own mean
        mean = None if is_dev(d) else np.ascontiguousarray(d.mean(axis=1))
        out = new(d, tuple(d.shape))
        check(self._lib.beatamd_autocovariance_batch(self._h, int(d.shape[0]), int(d.shape[1]), ptr(d),
                                                     ptr(mean), ptr(out)))
        return out

    def scaled_toeplitz_batch(self, coeffs, stds):
        c, s = as_input(coeffs), as_input(stds)
        self._adopt_stream(c, s)
        nd, n = int(c.shape[0]), int(c.shape[1])
        out = new(c, (nd, n, n))
        check(self._lib.beatamd_scaled_toeplitz_batch(self._h, nd, n, ptr(c), ptr(s), ptr(out)))
        return out

    def ball_rms_batch(self, coords, data, sizes, max_dist_perc):
        """covariance.k_nearest_neighbor_rms (covariance.py:774-811, max_dist_perc branch) for the datasets of a composite
        in one call: coords (Ntot, 2) east / north, data (Ntot,), both concatenated over datasets of ``sizes`` points ->
        (radius (nd,), counts (Ntot,) int32, stds (Ntot,)) in the one order include/beat_amd.h states
        (tests/noise2d_ref.py restates it bit for bit).  numpy in -> numpy out, torch-cuda in -> tensors on the same device."""
        c, d = as_input(coords), as_input(data)
        self._adopt_stream(c, d)
        n = as_input(sizes, np.int64).ravel()
        nd, ntot = int(n.size), int(n.sum()) if n.size else 0
        if tuple(c.shape) != (ntot, 2) or tuple(d.shape) != (ntot,):
            raise ValueError("ball_rms_batch: coords %s and data %s for %d points in all: expected (%d, 2) and (%d,)"
                             % (tuple(c.shape), tuple(d.shape), ntot, ntot, ntot))
        if is_dev(c) != is_dev(d):
            raise ValueError("ball_rms_batch: coords and data must live on the same side")
        radius, counts, stds = new(c, (nd,)), new(c, (ntot,), np.int32), new(c, (ntot,))
        check(self._lib.beatamd_ball_rms_batch(self._h, nd, ptr(n), ptr(c), ptr(d), float(max_dist_perc), ptr(radius),
                                               ptr(counts), ptr(stds)))
        return radius, counts, stds

    # -- fused FFI model
    def ffi_model_create(self, layout, n_patch_dip, n_patch_strike, patch_size):
        nd = np.ascontiguousarray(n_patch_dip, dtype=np.int32)
        ns = np.ascontiguousarray(n_patch_strike, dtype=np.int32)
        ps = np.ascontiguousarray(patch_size, dtype=np.float64)
        mid = C.c_int32()
        check(self._lib.beatamd_ffi_model_create(self._h, C.byref(layout), int(nd.size), ptr(nd) if nd.size else None,
                                                 ptr(ns) if ns.size else None, ptr(ps) if ps.size else None,
                                                 C.byref(mid)))
        return mid.value

    def ffi_model_add_wavemap(self, model_id, lib_ids, data, wset_id, hp_off, shift_off=None,
                              interpolation="nearest_neighbor"):
        libs = np.ascontiguousarray(lib_ids, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.float64)
        hp = as_input(hp_off, np.int64)
        sh = as_input(shift_off, np.int64)
        check(self._lib.beatamd_ffi_model_add_wavemap(self._h, model_id, ptr(libs), ptr(data), wset_id,
                                                      ptr(hp), ptr(sh), _interp(interpolation)))

    def ffi_model_add_wavemap_spectrum(self, model_id, lib_ids, data_spec, wset_id, hp_off, ntrans, valid_spectrum_indices,
                                       shift_off=None, interpolation="nearest_neighbor"):
        """a wavemap in the spectrum domain: data_spec (T, hi - lo) observed amplitude spectra, the weight set of that size"""
        libs = np.ascontiguousarray(lib_ids, dtype=np.int32)
        data_spec = np.ascontiguousarray(data_spec, dtype=np.float64)
        hp = as_input(hp_off, np.int64)
        sh = as_input(shift_off, np.int64)
        lo, hi = valid_spectrum_indices
        if data_spec.ndim != 2 or data_spec.shape[1] != int(hi) - int(lo):
            raise ValueError("spectrum domain: data_spec must be (T, %d), got %s" % (int(hi) - int(lo), data_spec.shape))
        check(self._lib.beatamd_ffi_model_add_wavemap_spectrum(self._h, model_id, ptr(libs), ptr(data_spec), wset_id, ptr(hp),
                                                               ptr(sh), _interp(interpolation), int(ntrans), int(lo), int(hi)))

    def amp_spectrum_batch(self, X, ntrans, valid_spectrum_indices, data_spec=None, out=None):
        """X (R, N) -> (R, hi - lo) = abs(rfft(X[r], ntrans))[lo:hi] on the device (csrc/spectrum.hip), or with data_spec
        (T, hi - lo) the residual data_spec[r mod T] - that.  numpy in -> numpy out, torch-cuda in -> tensor."""
        self._adopt_stream(X)
        X = as_input(X)
        if X.ndim != 2:
            raise ValueError("amp_spectrum: X must be (R, N), got %s" % (tuple(X.shape),))
        R, N = int(X.shape[0]), int(X.shape[1])
        lo, hi = int(valid_spectrum_indices[0]), int(valid_spectrum_indices[1])
        T = 0
        if data_spec is not None:
            if not hasattr(data_spec, "shape"):
                data_spec = np.asarray(data_spec, dtype=np.float64)
            data_spec = on_side(data_spec, X, np.float64, (int(data_spec.shape[0]), hi - lo), "data_spec")
            T = int(data_spec.shape[0])
        out = checked(out, X, (R, max(hi - lo, 0)), np.float64, "out")
        check(self._lib.beatamd_amp_spectrum_batch(self._h, R, N, int(ntrans), lo, hi, ptr(X), ptr(data_spec), T, ptr(out)))
        return out

    def ffi_model_add_geodetic(self, model_id, geo_lib_ids, data, odws, sizes, wset_ids, hp_off):
        libs = np.ascontiguousarray(geo_lib_ids, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.float64)
        odws = np.ascontiguousarray(odws, dtype=np.float64)
        sizes = as_input(sizes, np.int64)
        ws = np.ascontiguousarray(wset_ids, dtype=np.int32)
        hp = as_input(hp_off, np.int64)
        check(self._lib.beatamd_ffi_model_add_geodetic(self._h, model_id, ptr(libs), ptr(data), ptr(odws),
                                                       int(sizes.size), ptr(sizes), ptr(ws), ptr(hp)))

    def ffi_model_add_geodetic_geometry(self, model_id, kinds, param_off, param_fixed, east, north,
                                        los, nu, data, odws, sizes, wset_ids, hp_off):
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        po = np.ascontiguousarray(param_off, dtype=np.int64)
        pf = np.ascontiguousarray(param_fixed, dtype=np.float64)
        east = np.ascontiguousarray(east, dtype=np.float64)
        north = np.ascontiguousarray(north, dtype=np.float64)
        los = np.ascontiguousarray(los, dtype=np.float64)
        data = np.ascontiguousarray(data, dtype=np.float64)
        odws = np.ascontiguousarray(odws, dtype=np.float64)
        sizes = as_input(sizes, np.int64)
        ws = np.ascontiguousarray(wset_ids, dtype=np.int32)
        hp = as_input(hp_off, np.int64)
        check(self._lib.beatamd_ffi_model_add_geodetic_geometry(
            self._h, model_id, int(kinds.size), ptr(kinds), ptr(po), ptr(pf), int(east.size), ptr(east),
            ptr(north), ptr(los), float(nu), ptr(data), ptr(odws), int(sizes.size), ptr(sizes), ptr(ws),
            ptr(hp)))

    @staticmethod
    def check_correction_kinds(ncol, kind, earth):
        """the argument rules of the ..._kinds entry that need no model, checked ahead of the call (the library checks
        them again, and the offsets against the model's q): kind 0 or 1; a pole term has three columns and an earth of
        positive radii and an oblateness in [0, 1).  -> (kind int32 (nterm,), earth float64 (nterm, 3))"""
        nc = np.ascontiguousarray(ncol, dtype=np.int32)
        kd = np.ascontiguousarray(kind, dtype=np.int32)
        if kd.shape != nc.shape:
            raise ValueError("correction kinds: %d for %d terms" % (kd.size, nc.size))
        ea = np.ascontiguousarray(earth, dtype=np.float64)
        if ea.size != 3 * nc.size:
            raise ValueError("correction earth constants: %d values for %d terms (3 each)" % (ea.size, nc.size))
        ea = ea.reshape(nc.size, 3)
        for j in range(nc.size):
            if kd[j] not in (0, 1):
                raise ValueError("correction term %d has the unknown kind %d" % (j, kd[j]))
            if kd[j] == 1:
                if nc[j] != 3:
                    raise ValueError("the Euler-pole term %d has %d basis columns, not 3" % (j, nc[j]))
                r, a, f = ea[j]
                if not (r > 0.0 and a > 0.0 and 0.0 <= f < 1.0):
                    raise ValueError("correction term %d: earth (radius %g, equator radius %g, oblateness %g)"
                                     % (j, r, a, f))
        return kd, ea

    def ffi_model_add_geodetic_corrections(self, model_id, dataset, ncol, basis, coef_off, coef_fixed, kind=None,
                                           earth=None):
        """dataset corrections of the model's geodetic composite: per term its dataset index, column count, basis
        (n x K, one array per term), coefficient offsets in q (-1: fixed) and fixed values (K each).  kind / earth
        (``correction_tables(kinds=True)``): per term 0 (linear) or 1 (Euler pole: the offsets name pole_lat, pole_lon,
        omega) and its earth constants (radius, equator radius, oblateness) -- the ..._kinds entry"""
        nterm = len(dataset)
        ds = np.ascontiguousarray(dataset, dtype=np.int32)
        nc = np.ascontiguousarray(ncol, dtype=np.int32)
        if kind is not None:
            kd, ea = self.check_correction_kinds(nc, kind, earth)
        off = -np.ones((nterm, 4), dtype=np.int64)
        fix = np.zeros((nterm, 4))
        cols = []
        for j in range(nterm):
            k = int(nc[j])
            off[j, :k] = coef_off[j]
            fix[j, :k] = coef_fixed[j]
            B = np.asarray(basis[j], dtype=np.float64)
            if B.ndim != 2 or B.shape[1] != k:
                raise ValueError("correction term %d: basis of shape %s, expected (n, %d)" % (j, B.shape, k))
            cols.append(np.ravel(B, order="F"))
        flat = np.ascontiguousarray(np.concatenate(cols)) if cols else np.zeros(0)
        if kind is not None:
            check(self._lib.beatamd_ffi_model_add_geodetic_corrections_kinds(
                self._h, model_id, nterm, ptr(ds), ptr(nc), ptr(flat), ptr(off), ptr(fix), ptr(kd), ptr(ea)))
            return
        check(self._lib.beatamd_ffi_model_add_geodetic_corrections(
            self._h, model_id, nterm, ptr(ds), ptr(nc), ptr(flat), ptr(off), ptr(fix)))

    def ffi_model_set_laplacian(self, model_id, lap_id):
        check(self._lib.beatamd_ffi_model_set_laplacian(self._h, model_id, lap_id))

    def ffi_model_nllk(self, model_id):
        n = C.c_int64()
        check(self._lib.beatamd_ffi_model_nllk(self._h, model_id, C.byref(n)))
        return n.value

    def ffi_model_destroy(self, model_id):
        check(self._lib.beatamd_ffi_model_destroy(self._h, model_id))

    def ffi_logp_batch(self, model_id, Q, nllk, out=None):
        Q, Cn, out = self._q_out(Q, out, (nllk,))
        check(self._lib.beatamd_ffi_logp_batch(self._h, model_id, Cn, ptr(Q), ptr(out)))
        return out

    def ffi_synthetics_batch(self, model_id, wavemap_index, Q, T, N, residuals=False, out=None):
        """synthetics (or data - synthetics) [C, T, N] of one wavemap at the points Q [C, nparams]"""
        Qc, Cn, out = self._q_out(Q, out, (int(T), int(N)))
        check(self._lib.beatamd_ffi_synthetics_batch(self._h, model_id, int(wavemap_index), Cn, ptr(Qc),
                                                     int(bool(residuals)), ptr(out)))
        return out

    def ffi_start_times_batch(self, model_id, Q, npatches, out=None, chain_bad=None):
        """rupture onset times [C, npatches] of the model at the points Q [C, nparams]; chain_bad (int32 [C], optional,
        filled also when the call raises): chains whose hypocentre lies outside the patch grid"""
        Qc, Cn, out = self._q_out(Q, out, (int(npatches),))
        check(self._lib.beatamd_ffi_start_times_batch(self._h, model_id, Cn, ptr(Qc), ptr(out), ptr(chain_bad)))
        return out

    # -- moment, magnitude and moment-rate functions of a batch of draws (csrc/momentrate.hip)
    def ffi_magnitudes_batch(self, model_id, Q, moment_per_slip, npatches, comp_off=None):
        """(M0, Mw), each (C,): total moment ``sum_p k_p sqrt(sum_comp s^2)`` in patch order and its moment magnitude
        (ffi/fault.py:284-359) at the points Q (C, nparams); moment_per_slip (npatches,): the moment of a patch at unit
        slip; comp_off: offsets in q of the slip variables (None: the layout's own)"""
        self._adopt_stream(Q)
        Qc = as_input(Q)
        Cn = int(Qc.shape[0])
        k = on_side(moment_per_slip, Qc, np.float64, (int(npatches),), "moment_per_slip")
        off = as_input(comp_off, np.int64)
        M0, Mw = new(Qc, (Cn,)), new(Qc, (Cn,))
        check(self._lib.beatamd_ffi_magnitudes_batch(self._h, model_id, Cn, ptr(Qc), ptr(k), ptr(off),
                                                     0 if off is None else int(off.size), ptr(M0), ptr(Mw)))
        return M0, Mw

    def ffi_moment_rate_spans_batch(self, model_id, Q, nsubfaults, npatches, deltat, start_times=None, chain_bad=None,
                                    out=None):
        """spans (C, nsubfaults + 1, 2) int64 = (first index, count) of every subfault's moment-rate time axis and, in the
        last row, the total's (ffi/fault.py:413-420, 461-465); a time is index * deltat.  start_times (C, npatches) /
        chain_bad (C,) int32: onsets the caller holds (None: the model's sweep).  A flagged draw gets count 0 and the call
        raises ValueError after filling ``out``"""
        self._adopt_stream(Q)
        Qc = as_input(Q)
        Cn = int(Qc.shape[0])
        st = on_side(start_times, Qc, np.float64, (Cn, int(npatches)), "start_times")
        bad = on_side(chain_bad, Qc, np.int32, (Cn,), "chain_bad")
        out = checked(out, Qc, (Cn, int(nsubfaults) + 1, 2), np.int64, "spans")
        check(self._lib.beatamd_ffi_moment_rate_spans_batch(self._h, model_id, Cn, ptr(Qc), ptr(st), ptr(bad), float(deltat),
                                                            ptr(out)))
        return out

    def ffi_moment_rates_batch(self, model_id, Q, moment_per_slip, nsubfaults, npatches, deltat, kbase, NT, comp_off=None,
                               start_times=None, chain_bad=None, stf=0, out=None, spans=None):
        """rates (C, nsubfaults + 1, NT) on the index grid [kbase, kbase + NT): the subfaults' moment-rate functions and,
        in the last row, their sum (ffi/fault.py:361-474).  A draw that does not fit the grid, or is flagged, gets NaN
        rows and the call raises ValueError after filling ``out`` (and ``spans``, when given)"""
        self._adopt_stream(Q)
        Qc = as_input(Q)
        Cn = int(Qc.shape[0])
        k = on_side(moment_per_slip, Qc, np.float64, (int(npatches),), "moment_per_slip")
        off = as_input(comp_off, np.int64)
        st = on_side(start_times, Qc, np.float64, (Cn, int(npatches)), "start_times")
        bad = on_side(chain_bad, Qc, np.int32, (Cn,), "chain_bad")
        out = checked(out, Qc, (Cn, int(nsubfaults) + 1, int(NT)), np.float64, "rates")
        if spans is not None:
            spans = checked(spans, Qc, (Cn, int(nsubfaults) + 1, 2), np.int64, "spans")
        check(self._lib.beatamd_ffi_moment_rates_batch(self._h, model_id, Cn, ptr(Qc), ptr(k), ptr(off),
                                                       0 if off is None else int(off.size), ptr(st), ptr(bad), float(deltat),
                                                       int(stf), int(kbase), int(NT), ptr(out), ptr(spans)))
        return out

    def ffi_astep_batch(self, model_id, Q0, L0, delta, scaling, lower, upper, log_u, beta,
                        accepted=None):
        """In-place update of Q0 / L0 (must be contiguous float64); returns accepted (int32)."""
        self._adopt_stream(Q0, delta)
        Cn = int(Q0.shape[0])
        if accepted is None:
            accepted = new(Q0, (Cn,), np.int32)
        for a in (Q0, L0):
            if isinstance(a, np.ndarray) and not is_canonical(a):
                raise ValueError("Q0 / L0 must be C-contiguous float64 (updated in place)")
        # converted arrays are bound to locals: a temporary would be freed before the call reads it
        de, sc, lo, up, lu = as_input(delta), as_input(scaling), as_input(lower), as_input(upper), as_input(log_u)
        if np.ndim(beta) == 0 and not hasattr(beta, "data_ptr"):
            check(self._lib.beatamd_ffi_astep_batch(self._h, model_id, Cn, ptr(Q0), ptr(L0), ptr(de),
                                                    ptr(sc), ptr(lo), ptr(up), ptr(lu), float(beta),
                                                    ptr(accepted)))
        else:  # one beta per chain (parallel tempering replicas)
            be = as_input(beta)
            check(self._lib.beatamd_ffi_astep_batch_betas(self._h, model_id, Cn, ptr(Q0), ptr(L0),
                                                          ptr(de), ptr(sc), ptr(lo), ptr(up), ptr(lu),
                                                          ptr(be), ptr(accepted)))
        return accepted

    def ffi_mstep_batch(self, model_id, Q0, L0, factor, kind, df, seed, step, first_chain, scaling, lower,
                        upper, beta, accepted, accepted_sum=None, n_accepted=None):
        """One Metropolis step of every chain with the proposal drawn on the device
        (beatamd_ffi_mstep_batch): device tensors only, nothing returns to the host.
        kind None / -1: multivariate proposal with ``factor`` [K, nparams] (df > 0: multivariate t);
        0/1/2: per-parameter Normal / Cauchy / Laplace with ``factor`` = scales [nparams]."""
        self._adopt_stream(Q0, L0)
        Cn = int(Q0.shape[0])
        kind = -1 if kind is None else int(kind)
        fa, sc, lo, up = as_input(factor), as_input(scaling), as_input(lower), as_input(upper)
        K = int(fa.shape[0]) if kind < 0 else 0
        scalar = np.ndim(beta) == 0 and not hasattr(beta, "data_ptr")
        be = None if scalar else as_input(beta)
        check(self._lib.beatamd_ffi_mstep_batch(
            self._h, model_id, Cn, ptr(Q0), ptr(L0), ptr(fa), K, kind, int(df), int(seed) & (2 ** 64 - 1),
            int(step) & 0xffffffff, int(first_chain), ptr(sc), ptr(lo), ptr(up), float(beta) if scalar else 1.0,
            None if scalar else ptr(be), ptr(accepted), None if accepted_sum is None else ptr(accepted_sum),
            None if n_accepted is None else ptr(n_accepted)))
        return accepted

    def ffi_mstep_batch_grouped(self, model_id, Q0, L0, factors, df, seed, step, first_chain, scaling, lower, upper,
                                beta, accepted, accepted_sum=None, n_accepted=None):
        """``ffi_mstep_batch`` with one multivariate factor per group of chains (beatamd_ffi_mstep_batch_grouped):
        ``factors`` [G, K, nparams], chain c draws with factor c // (C // G)"""
        self._adopt_stream(Q0, L0)
        Cn = int(Q0.shape[0])
        fa, sc, lo, up = as_input(factors), as_input(scaling), as_input(lower), as_input(upper)
        if fa.ndim != 3:
            raise ValueError("ffi_mstep_batch_grouped: factors must be (groups, K, nparams)")
        G, K = int(fa.shape[0]), int(fa.shape[1])
        scalar = np.ndim(beta) == 0 and not hasattr(beta, "data_ptr")
        be = None if scalar else as_input(beta)
        check(self._lib.beatamd_ffi_mstep_batch_grouped(
            self._h, model_id, Cn, G, ptr(Q0), ptr(L0), ptr(fa), K, int(df), int(seed) & (2 ** 64 - 1),
            int(step) & 0xffffffff, int(first_chain), ptr(sc), ptr(lo), ptr(up), float(beta) if scalar else 1.0,
            None if scalar else ptr(be), ptr(accepted), None if accepted_sum is None else ptr(accepted_sum),
            None if n_accepted is None else ptr(n_accepted)))
        return accepted

    # -- introspection
    def last_kernel(self):
        """name<template arguments> of the stacking kernel the most recent call launched"""
        buf = C.create_string_buffer(128)
        check(self._lib.beatamd_ctx_last_kernel(self._h, buf, 128))
        return buf.value.decode()

    def gf_group_stats(self):
        """-> dict(chains_per_group, mean_rows, max_rows, row_bytes) of the last chain-shared launch"""
        cg, mx, rb, mean = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        check(self._lib.beatamd_ctx_gf_group_stats(self._h, C.byref(cg), C.byref(mean), C.byref(mx),
                                                   C.byref(rb)))
        return dict(chains_per_group=cg.value, mean_rows=mean.value, max_rows=mx.value,
                    row_bytes=rb.value)

    def reload_knobs(self):
        """read the BEATAMD_G* / BEATAMD_WS_MAP / BEATAMD_SWEEP_V1 knobs from the environment again (they are read once,
        when the context is created, unless it was created under BEATAMD_KNOBS_LIVE=1)"""
        check(self._lib.beatamd_ctx_reload_knobs(self._h))

    def gf_plan(self, passes=True):
        """-> dict(plan=<what the kernel selection chose for the last stacking launch and why>, mean_passes, max_passes:
        row passes per (chain group, target, patch); 1 unless a patch touched more rows than an LDS buffer holds)"""
        buf = C.create_string_buffer(512)
        mean, mx = C.c_double(), C.c_int64()
        check(self._lib.beatamd_ctx_gf_plan(self._h, buf, 512, C.byref(mean) if passes else None,
                                            C.byref(mx) if passes else None))
        out = dict(plan=buf.value.decode())
        if passes:
            out.update(mean_passes=mean.value, max_passes=mx.value)
        return out

    def gf_tune_log(self):
        """the most recent group-size measurement of the lane <-> chain stacking kernels, in words (empty before the
        first one): the first call of a problem shape launches every candidate group size twice and keeps the fastest"""
        buf = C.create_string_buffer(512)
        check(self._lib.beatamd_ctx_gf_tune_log(self._h, buf, 512))
        return buf.value.decode()

    def gf_chain_groups(self, key0, key1, chains_per_group=512):
        """how a batch is cut into its chain groups (scheduling only): key0 / key1 (C,) per-chain keys -- the hypocentre
        (strike, dip) in the fused model path -> uint32 array [ngroups, chains_per_group] of chain ids, 0xffffffff behind
        the last chain (recursive bisection along the key of the wider extent, k_gc_cut)"""
        k0, k1 = [k if is_dev(k) else upload(k, "cuda:%d" % self.device, np.float64) for k in (key0, key1)]
        self._adopt_stream(k0, k1)
        k0, k1 = as_input(k0), as_input(k1)
        Cn = int(k0.numel())
        ng = (Cn + chains_per_group - 1) // chains_per_group
        out = np.empty(ng * chains_per_group, dtype=np.uint32)
        check(self._lib.beatamd_ctx_gf_chain_groups(self._h, Cn, ptr(k0), ptr(k1), int(chains_per_group),
                                                    out.ctypes.data_as(C.c_void_p)))
        return out.reshape(ng, chains_per_group)

    # -- sampler steps on the device (SMC stage transition, proposals, exchange)
    def smc_calc_beta(self, likelihoods, beta, coef_variation, stride=1, n=None):
        """smc.py:133-165 -> (beta_new, weights); likelihoods: (C,) array or a strided view
        described by (tensor, stride, n)"""
        self._adopt_stream(likelihoods)
        lk = as_input(likelihoods)
        Cn = int(n if n is not None else (lk.numel() if is_dev(lk) else lk.size))
        w = new(lk, (Cn,))
        b = C.c_double()
        check(self._lib.beatamd_smc_calc_beta(self._h, Cn, ptr(lk), int(stride), float(beta),
                                              float(coef_variation), C.byref(b), ptr(w)))
        return b.value, w

    def smc_stage_weights(self, likelihoods, dbeta, stride=1, n=None):
        self._adopt_stream(likelihoods)
        lk = as_input(likelihoods)
        Cn = int(n if n is not None else (lk.numel() if is_dev(lk) else lk.size))
        w = new(lk, (Cn,))
        check(self._lib.beatamd_smc_stage_weights(self._h, Cn, ptr(lk), int(stride), float(dbeta), ptr(w)))
        return w

    def smc_resample(self, weights, aux):
        """smc.py:290-324 -> resampling indexes (int32)"""
        self._adopt_stream(weights)
        w = as_input(weights)
        Cn = int(w.numel()) if is_dev(w) else int(w.size)
        idx = new(w, (Cn,), np.int32)
        check(self._lib.beatamd_smc_resample(self._h, Cn, ptr(w), float(aux), ptr(idx)))
        return idx

    def smc_population_factor(self, population, weights):
        self._adopt_stream(population, weights)
        X, w = as_input(population), as_input(weights)
        Cn, npar = int(X.shape[0]), int(X.shape[1])
        F = new(X, (Cn, npar))
        check(self._lib.beatamd_smc_population_factor(self._h, Cn, npar, ptr(X), ptr(w), ptr(F)))
        return F

    def proposal_draw(self, factor, n_chains, seed, step, first_chain=0, df=0, delta=None, log_u=None,
                      want_log_u=True):
        """delta (n_chains, nparams) = z . factor with z from Philox4x32-10; -> (delta, log_u)"""
        self._adopt_stream(factor)
        F = as_input(factor)
        K, npar = int(F.shape[0]), int(F.shape[1])
        if delta is None:
            delta = new(F, (int(n_chains), npar))
        if log_u is None and want_log_u:
            log_u = new(F, (int(n_chains),))
        check(self._lib.beatamd_proposal_draw(self._h, int(n_chains), K, npar, ptr(F), int(seed) & (2 ** 64 - 1),
                                              int(step) & 0xffffffff, int(first_chain), int(df), ptr(delta),
                                              ptr(log_u)))
        return delta, log_u

    def proposal_draw_grouped(self, factors, n_chains, seed, step, first_chain=0, df=0, delta=None, log_u=None,
                              want_log_u=True):
        """``proposal_draw`` with one factor per group of chains: factors (G, K, nparams), chain c of the call draws with
        factor c // (n_chains // G) (beatamd_proposal_draw_grouped); -> (delta, log_u)"""
        self._adopt_stream(factors)
        F = as_input(factors)
        if F.ndim != 3:
            raise ValueError("proposal_draw_grouped: factors must be (groups, K, nparams)")
        G, K, npar = int(F.shape[0]), int(F.shape[1]), int(F.shape[2])
        if delta is None:
            delta = new(F, (int(n_chains), npar))
        if log_u is None and want_log_u:
            log_u = new(F, (int(n_chains),))
        check(self._lib.beatamd_proposal_draw_grouped(self._h, int(n_chains), G, K, npar, ptr(F), int(seed) & (2 ** 64 - 1),
                                                      int(step) & 0xffffffff, int(first_chain), int(df), ptr(delta),
                                                      ptr(log_u)))
        return delta, log_u

    # -- PT proposal adaptation: streaming likelihood-weighted moments per group of chains (ptadapt.hip)
    @staticmethod
    def group_moments_stride(nparams):
        """doubles of one group's state: header (m, S0, Sw2, count, nbad, 3 spare), S1 [n], S2 [n, n] (lower triangle)"""
        return 8 + int(nparams) + int(nparams) ** 2

    def group_moments_reset(self, state, nparams, Q=None, ref=None):
        """state (G, 8 + n + n*n), numpy or torch-cuda, in place: m = -inf, every sum 0.  With Q (G * R, n) and ref (G, n):
        ref[g] = mean of the group's rows, written in place (the reference point of the window that opens)"""
        self._adopt_stream(state)
        S = self._group_state(state, nparams)
        G, R, Qc = int(S.shape[0]), 0, None
        if ref is not None:
            Qc = as_input(Q)
            if isinstance(ref, np.ndarray) and not is_canonical(ref):
                raise ValueError("group_moments_reset: ref must be C-contiguous float64 (written in place)")
            if int(Qc.shape[0]) % G or int(Qc.shape[1]) != int(nparams) or tuple(as_input(ref).shape) != (G, int(nparams)):
                raise ValueError("group_moments_reset: Q (G * R, nparams), ref (G, nparams) for the G groups of the state")
            R = int(Qc.shape[0]) // G
        check(self._lib.beatamd_group_moments_reset(self._h, G, int(nparams), ptr(S), R, ptr(Qc),
                                                    None if ref is None else ptr(ref)))
        return state

    def _group_state(self, state, nparams):
        ok = is_canonical(state) if isinstance(state, np.ndarray) else True
        S = as_input(state)
        if not ok or S.ndim != 2 or int(S.shape[1]) != self.group_moments_stride(nparams):
            raise ValueError("group moments: state must be C-contiguous float64 (groups, 8 + nparams + nparams^2)")
        return S

    def group_moments_update(self, state, Q, like, ref, like_stride=1):
        """add the rows of Q (G * R, n) -- R consecutive rows per group -- with weights exp(like - running maximum) to
        state, in place; like: (G * R,) array, or a strided view (see ``sampler.ops._Base``) with like_stride; ref (G, n)"""
        self._adopt_stream(state, Q)
        Qc, rf = as_input(Q), as_input(ref)
        lk = as_input(like)
        npar = int(Qc.shape[1])
        S = self._group_state(state, npar)
        G = int(S.shape[0])
        if int(Qc.shape[0]) % G or tuple(rf.shape) != (G, npar):
            raise ValueError("group_moments_update: Q (G * R, nparams), ref (G, nparams) for the G groups of the state")
        check(self._lib.beatamd_group_moments_update(self._h, G, int(Qc.shape[0]) // G, npar, ptr(Qc), ptr(lk),
                                                     int(like_stride), ptr(rf), ptr(S)))
        return state

    def group_moments_factor(self, state, nparams, factor, want_cov=False):
        """-> (factor, cov or None, flags int32 (G,)): the upper Cholesky factors (G, n, n) of the groups' weighted sample
        covariances written into ``factor`` (a flagged group's is left untouched; flags: 1 degenerate or non-finite
        moments, 2 not positive definite)"""
        self._adopt_stream(state, factor)
        S = self._group_state(state, nparams)
        G, n = int(S.shape[0]), int(nparams)
        if isinstance(factor, np.ndarray) and not is_canonical(factor):
            raise ValueError("group_moments_factor: factor must be C-contiguous float64 (written in place)")
        F = as_input(factor)
        if tuple(F.shape) != (G, n, n):
            raise ValueError("group_moments_factor: factor must be (groups, nparams, nparams)")
        cov = new(S, (G, n, n)) if want_cov else None
        flags = new(S, (G,), np.int32)
        check(self._lib.beatamd_group_moments_factor(self._h, G, n, ptr(S), ptr(F), ptr(cov), ptr(flags)))
        return factor, cov, flags

    def proposal_draw_univariate(self, kind, scale, n_chains, seed, step, first_chain=0, delta=None, log_u=None,
                                 want_log_u=True):
        """delta (n_chains, nparams): independent Normal (0) / Cauchy (1) / Laplace (2) draws per
        component times scale[j] (beat/sampler/base.py:129-160); -> (delta, log_u)"""
        self._adopt_stream(scale)
        sc = as_input(scale)
        npar = int(sc.shape[0])
        if delta is None:
            delta = new(sc, (int(n_chains), npar))
        if log_u is None and want_log_u:
            log_u = new(sc, (int(n_chains),))
        check(self._lib.beatamd_proposal_draw_univariate(self._h, int(n_chains), npar, int(kind), ptr(sc),
                                                         int(seed) & (2 ** 64 - 1), int(step) & 0xffffffff,
                                                         int(first_chain), ptr(delta), ptr(log_u)))
        return delta, log_u

    def gather_rows(self, src, indexes, out=None):
        self._adopt_stream(src, indexes)
        S = as_input(src)
        idx = as_input(indexes, np.int32)
        nout = int(idx.numel()) if is_dev(idx) else int(idx.size)
        if out is None:
            out = new(S, (nout, int(S.shape[1])))
        check(self._lib.beatamd_gather_rows(self._h, nout, int(S.shape[1]), ptr(S), int(S.shape[0]),
                                            ptr(idx), ptr(out)))
        return out

    def metropolis_tune(self, scaling, accepted, tune_interval):
        """in place: scaling *= pymc tune factor(accepted / interval); accepted = 0"""
        self._adopt_stream(scaling)
        check(self._lib.beatamd_metropolis_tune(self._h, int(scaling.shape[0]), ptr(scaling), ptr(accepted),
                                                int(tune_interval)))

    # -- a Metropolis step in pieces (a collective between forward model and acceptance: target-sharded models)
    def like_assemble(self, gathered, dst_col, local_ll, local_col0, n_rest, rest_dst0, group_end, LL):
        """LL [C, nllk] (device) from the all-gathered rows `gathered` [nsrc, C] of all ranks: row r -> column dst_col[r]
        (-1: a rank's flag row, NaN = chain outside the library grid there), the replicated columns
        local_ll[:, local_col0 : local_col0 + n_rest] -> columns rest_dst0.., like = the composites' sums (k_like_sum's order)"""
        self._adopt_stream(gathered, LL)
        dc = np.ascontiguousarray(dst_col, dtype=np.int32)
        ge = np.ascontiguousarray(group_end, dtype=np.int32)
        Cn, nllk = int(LL.shape[0]), int(LL.shape[1])
        if int(gathered.shape[0]) != dc.size or int(gathered.shape[1]) != Cn or not gathered.is_contiguous() or not LL.is_contiguous():
            raise ValueError("like_assemble: gathered must be a contiguous (nsrc, C) tensor, LL a contiguous (C, nllk) one")
        check(self._lib.beatamd_like_assemble(self._h, Cn, nllk, dc.size, ptr(gathered), dc.ctypes.data,
                                              ptr(local_ll) if n_rest else None, int(local_ll.stride(0)) if n_rest else 0,
                                              int(local_col0), int(n_rest), int(rest_dst0), ge.size, ge.ctypes.data, ptr(LL)))
        return LL

    def metropolis_propose(self, Q0, delta, scaling, lower, upper, Qprop, inbounds):
        """metropolis.py:313-343 for all chains: Qprop = Q0 + delta * scaling inside the prior box, else Q0; inbounds int32 [C]"""
        self._adopt_stream(Q0, Qprop)
        check(self._lib.beatamd_metropolis_propose(self._h, int(Q0.shape[0]), int(Q0.shape[1]), ptr(as_input(Q0)),
                                                   ptr(as_input(delta)), ptr(as_input(scaling)), ptr(as_input(lower)),
                                                   ptr(as_input(upper)), ptr(Qprop), ptr(inbounds)))

    def metropolis_accept(self, Q0, L0, Qprop, Lprop, inbounds, log_u, beta, accepted):
        """metropolis.py:344-385 for all chains, in place on Q0 / L0; beta: float or a device tensor [C]"""
        self._adopt_stream(Q0, L0)
        per_chain = hasattr(beta, "data_ptr")
        check(self._lib.beatamd_metropolis_accept(self._h, int(Q0.shape[0]), int(Q0.shape[1]), int(L0.shape[1]), ptr(Q0), ptr(L0),
                                                  ptr(Qprop), ptr(Lprop), ptr(inbounds), ptr(as_input(log_u)),
                                                  1.0 if per_chain else float(beta), ptr(as_input(beta)) if per_chain else None,
                                                  ptr(accepted)))

    # -- hyper-parameter estimation (csrc/hyper.hip)
    # -- lsq start (csrc/lsq.hip; reference problems.py:753-873)
    def ffi_model_set_lsq_variables(self, model_id, inverted, zeroed=-1):
        check(self._lib.beatamd_ffi_model_set_lsq_variables(self._h, model_id, int(inverted), int(zeroed)))

    def ffi_lsq_normal_batch(self, model_id, Q, npatches, chain_bad=None):
        """normal equations of the chains' linear slip problems at the points Q [C, nparams] -> N [C, P, P], b [C, P];
        chain_bad (int32 [C], optional, filled also when the call raises IndexError): chains outside the library grid"""
        self._adopt_stream(Q)
        Qc = as_input(Q)
        Cn, P = int(Qc.shape[0]), int(npatches)
        N, b = new(Qc, (Cn, P, P)), new(Qc, (Cn, P))
        check(self._lib.beatamd_ffi_lsq_normal_batch(self._h, model_id, Cn, ptr(Qc), ptr(N), ptr(b), ptr(chain_bad)))
        return N, b

    def nnls_batch(self, N, b):
        """min |A x - d| s.t. x >= 0 from N = A^T A [C, n, n] and b = A^T d [C, n] -> x [C, n], iters [C], status [C]
        (0 ok, 1 iteration cap, 2 non-finite input / passive block not positive definite)"""
        self._adopt_stream(N, b)
        N, b = as_input(N), as_input(b)
        Cn, n = int(b.shape[0]), int(b.shape[1])
        if tuple(N.shape) != (Cn, n, n):
            raise ValueError("nnls_batch: N %s does not match b %s" % (tuple(N.shape), tuple(b.shape)))
        x, it, st = new(b, (Cn, n)), new(b, (Cn,), np.int32), new(b, (Cn,), np.int32)
        check(self._lib.beatamd_nnls_batch(self._h, Cn, n, ptr(N), ptr(b), ptr(x), ptr(it), ptr(st)))
        return x, it, st

    def ffi_lsq_solution_batch(self, model_id, Q):
        """Q [C, nparams] -> (Q with the inverted slip variable replaced by its non-negative least-squares solution and
        the perpendicular one by zeros, iters [C], status [C])"""
        Qc, Cn, out = self._q_out(Q, None, lambda q: tuple(q.shape[1:]))
        it, st = new(Qc, (Cn,), np.int32), new(Qc, (Cn,), np.int32)
        check(self._lib.beatamd_ffi_lsq_solution_batch(self._h, model_id, Cn, ptr(Qc), ptr(out), ptr(it), ptr(st)))
        return out, it, st

    def ffi_model_nterm(self, model_id):
        n = C.c_int64()
        check(self._lib.beatamd_ffi_model_nterm(self._h, model_id, C.byref(n)))
        return n.value

    def ffi_llks_batch(self, model_id, Q, out=None):
        """the cached misfits |W r|^2 of every dataset (and |L s_v|^2 per slip variable) at the points Q [C, nparams]
        -> [C, nterm]: update_llks of every composite (seismic.py:510-525, geodetic.py:429-444, laplacian.py:141-154)"""
        Q, Cn, out = self._q_out(Q, out, lambda q: (self.ffi_model_nterm(model_id),))
        check(self._lib.beatamd_ffi_llks_batch(self._h, model_id, Cn, ptr(Q), ptr(out)))
        return out

    def hyper_model_create(self, nh, M, slog, kind, hp_index, group_end):
        M = np.ascontiguousarray(M, dtype=np.int64)
        slog = np.ascontiguousarray(slog, dtype=np.float64)
        kind = np.ascontiguousarray(kind, dtype=np.int32)
        hp_index = np.ascontiguousarray(hp_index, dtype=np.int32)
        ge = np.ascontiguousarray(group_end, dtype=np.int32)
        if not (M.size == slog.size == kind.size == hp_index.size):
            raise ValueError("hyper model: M, slog, kind and hp_index have one entry per term")
        hid = C.c_int32()
        check(self._lib.beatamd_hyper_model_create(self._h, M.size, int(nh), M.ctypes.data, slog.ctypes.data, kind.ctypes.data,
                                                   hp_index.ctypes.data, ge.size, ge.ctypes.data, C.byref(hid)))
        return hid.value

    def hyper_model_destroy(self, hyper_id):
        check(self._lib.beatamd_hyper_model_destroy(self._h, hyper_id))

    def hyper_logp_batch(self, hyper_id, H, llks, out=None):
        """H [C, nh], llks [C, nterm] -> LL [C, nterm + 1] (terms, like): hyper_normal / _eval_prior for C chains"""
        self._adopt_stream(H, llks)
        H, llks = as_input(H), as_input(llks)
        if is_dev(H) != is_dev(llks):
            raise ValueError("hyper_logp: H and llks must live on the same side")
        Cn = int(H.shape[0])
        if out is None:
            out = new(H, (Cn, int(llks.shape[1]) + 1))
        check(self._lib.beatamd_hyper_logp_batch(self._h, hyper_id, Cn, ptr(H), ptr(llks), ptr(out)))
        return out

    def hyper_chain_batch(self, hyper_id, n_steps, H, LL, scaling, accepted_since_tune, llks, lower, upper, kind, scales,
                          seed, step0, first_chain, tune_interval, steps_until_tune, buffer_thinning=1, trace=None,
                          n_accepted=None):
        """n_steps Metropolis steps of every chain in one launch (beatamd_hyper_chain_batch); device tensors, in place on
        H, LL, scaling, accepted_since_tune"""
        self._adopt_stream(H, LL)
        for a in (H, LL, scaling, llks, lower, upper, scales):
            as_input(a)
        check(self._lib.beatamd_hyper_chain_batch(
            self._h, hyper_id, int(H.shape[0]), int(n_steps), ptr(H), ptr(LL), ptr(scaling), ptr(accepted_since_tune),
            ptr(llks), ptr(lower), ptr(upper), int(kind), ptr(scales), int(seed) & (2 ** 64 - 1), int(step0) & 0xffffffff,
            int(first_chain), int(tune_interval), int(steps_until_tune), int(buffer_thinning),
            None if trace is None else ptr(trace), None if n_accepted is None else ptr(n_accepted)))

    # -- posterior diagnostics (csrc/summary.hip)
    def wset_quad_batch(self, wset_id, residuals, out=None):
        """residuals (C, nd, M) -> (C, nd): |W_d r|^2 per dataset of a weight set, the misfit kernels of
        ``mvn_chol_logp_batch`` (seismic.py:610-616 nom / denom with W^T W = inv(C))"""
        r, Cn, out = self._q_out(residuals, out, lambda r: (int(r.shape[1]),))
        check(self._lib.beatamd_wset_quad_batch(self._h, wset_id, Cn, ptr(r), ptr(out)))
        return out

    def ffi_obs_quads(self, model_id, ndata, out=None):
        """|W_k d_k|^2 of every dataset of the model -> (ndata,) numpy (or into the device tensor ``out``): the
        denominators of the variance reduction (seismic.py:612-616, geodetic.py:497-501), cached on the model"""
        if out is None:
            out = np.empty(int(ndata))
        else:
            self._adopt_stream(out)
        check(self._lib.beatamd_ffi_obs_quads(self._h, model_id, ptr(out)))
        return out

    def ffi_variance_reductions_batch(self, model_id, Q, ndata, out=None):
        """Q (C, nparams) -> VR (C, ndata) = 1 - |W r|^2 / |W d|^2 per dataset and draw (get_variance_reductions,
        seismic.py:564-634, geodetic.py:446-511)"""
        Q, Cn, out = self._q_out(Q, out, (int(ndata),))
        check(self._lib.beatamd_ffi_variance_reductions_batch(self._h, model_id, Cn, ptr(Q), ptr(out)))
        return out

    def ffi_geo_residuals_batch(self, model_id, Q, nobs, residuals=True, out=None):
        """Q (C, nparams) -> (C, nobs): the geodetic composite's residual (d - mu) * odw - corrections
        (geodetic.py:1072-1077) or, residuals=False, its synthetics mu"""
        Q, Cn, out = self._q_out(Q, out, (int(nobs),))
        check(self._lib.beatamd_ffi_geo_residuals_batch(self._h, model_id, Cn, ptr(Q), int(bool(residuals)), ptr(out)))
        return out

    def standardize_batch(self, S, residuals, hp=None, out=None):
        """out[c, t] = exp(-hp[c, t]) * S_t . residuals[c, t]: the standardized residuals of
        get_standardized_residuals (seismic.py:527-562) with S_t = inv(chol(C_t)).  S (T,) scalars or (T, N, N);
        residuals (C, T, N); hp (C, T) or None"""
        self._adopt_stream(residuals)
        r = as_input(residuals)
        if r.ndim != 3:
            raise ValueError("standardize_batch: residuals must be (C, T, N)")
        Cn, T, N = [int(v) for v in r.shape]
        Sc = as_input(S)
        if tuple(Sc.shape) == (T,):
            kind = _lib.W_SCALAR
        elif tuple(Sc.shape) == (T, N, N):
            kind = _lib.W_DENSE
        else:
            raise ValueError("standardize_batch: S must be (%d,) or (%d, %d, %d)" % (T, T, N, N))
        h = None
        if hp is not None:
            h = as_input(hp)
            if tuple(h.shape) != (Cn, T):
                raise ValueError("standardize_batch: hp must be (%d, %d)" % (Cn, T))
        if out is None:
            out = new(r, (Cn, T, N))
        check(self._lib.beatamd_standardize_batch(self._h, kind, ptr(Sc), T, N, Cn, ptr(r), ptr(h), ptr(out)))
        return out

    def pole_coefficients_batch(self, Q, var_off, var_fixed, earth, out=None):
        """Q (C, nparams) -> (C, npole, 4): the derived Euler-pole coefficients ``omega' p`` (slot 3 zero) of every row
        and pole, by the kernel the model launches.  var_off / var_fixed / earth: (npole, 3) offsets of (pole_lat,
        pole_lon, omega) in q (-1: the fixed value) and (radius, equator radius, oblateness)"""
        off = np.ascontiguousarray(var_off, dtype=np.int64).reshape(-1, 3)
        fix = np.ascontiguousarray(var_fixed, dtype=np.float64).reshape(-1, 3)
        ea = np.ascontiguousarray(earth, dtype=np.float64).reshape(-1, 3)
        if not (off.shape == fix.shape == ea.shape):
            raise ValueError("pole_coefficients_batch: offsets, fixed values and earth constants differ in shape")
        Q, Cn, out = self._q_out(Q, out, (off.shape[0], 4))
        check(self._lib.beatamd_pole_coefficients_batch(self._h, Cn, int(Q.shape[1]), ptr(Q), int(off.shape[0]), ptr(off), ptr(fix),
                                                        ptr(ea), ptr(out)))
        return out

    def pole_coupling_batch(self, Q, var_off, var_fixed, earth, basis, uparr_off):
        """Q (C, nparams) -> (euler_slips, coupling), each (C, P): ``euler_pole2slips`` and ``backslip2coupling``
        (ffi/fault.py:1436-1517) of every row for one pole against the patch basis (P, 3) of
        ``summary.pole_patch_basis``; uparr_off: offset of the P back-slips in q"""
        self._adopt_stream(Q)
        Q = as_input(Q)
        Cn, npar = int(Q.shape[0]), int(Q.shape[1])
        off = np.ascontiguousarray(var_off, dtype=np.int64).reshape(3)
        fix = np.ascontiguousarray(var_fixed, dtype=np.float64).reshape(3)
        ea = np.ascontiguousarray(earth, dtype=np.float64).reshape(3)
        Bp = as_input(basis)
        if Bp.ndim != 2 or Bp.shape[1] != 3 or is_dev(Bp) != is_dev(Q):
            raise ValueError("pole_coupling_batch: basis must be (P, 3) on Q's side")
        P = int(Bp.shape[0])
        es, cp = new(Q, (Cn, P)), new(Q, (Cn, P))
        check(self._lib.beatamd_pole_coupling_batch(self._h, Cn, npar, ptr(Q), ptr(off), ptr(fix), ptr(ea), P, ptr(Bp),
                                                    int(uparr_off), ptr(es), ptr(cp)))
        return es, cp

    def ensemble_moments_update(self, X, state=None, n_seen=0):
        """fold the rows of X (C, M) into the running column moments ``state`` (5, M) = (mean, M2, min, max, rows
        seen), Welford in row order: the result does not depend on how the rows are cut into calls.  state None
        (with n_seen 0) allocates one on X's side.  -> (state, n_seen + C)"""
        self._adopt_stream(X)
        x = as_input(X)
        if x.ndim != 2:
            raise ValueError("ensemble_moments_update: X must be (C, M)")
        Cn, M = int(x.shape[0]), int(x.shape[1])
        if state is None:
            if n_seen:
                raise ValueError("ensemble_moments_update: %d rows seen but no state given" % n_seen)
        state = checked(state, x, (5, M), np.float64, "ensemble_moments_update: state", of="X")
        check(self._lib.beatamd_ensemble_moments_update(self._h, Cn, M, ptr(x), ptr(state), int(n_seen)))
        return state, int(n_seen) + Cn

    def ensemble_moments_finish(self, state, n):
        """-> (mean, std, min, max), each (M,): std = sqrt(M2 / n) as numpy.std (ddof = 0)"""
        self._adopt_stream(state)
        s = as_input(state)
        M = int(s.shape[1])
        outs = [new(s, (M,)) for _ in range(4)]
        check(self._lib.beatamd_ensemble_moments_finish(self._h, M, ptr(s), int(n), *[ptr(o) for o in outs]))
        return tuple(outs)

    def trace_density_update(self, Y, tmin, deltat, extent, grid_size=(500, 500), linewidth=7, grid=None):
        """add the line images of the traces Y (E, T, N) to the density grids (T, ny, nx) of their targets -- the grid
        ``fuzzy_waveforms`` builds with ``draw_line_on_array`` (plotting/seismic.py:255-316, plotting/common.py:619-801),
        bit for bit.  Sample j of target t lies at tmin[t] + j * deltat; extent (T, 4) = (xmin, xmax, ymin, ymax) per
        target (``summary.density_extent`` gives the reference's default); grid None allocates a zeroed one on Y's side,
        a given one is added to and returned.  Traces are taken in ensemble order: cutting an ensemble into calls does
        not change the result.  TypeError: a sample or time beyond the extent's upper side (below the lower side it is
        clipped); ValueError: a non-finite sample, a bad shape."""
        return self._trace_density(Y, tmin, deltat, extent, None, grid_size, linewidth, grid)

    def trace_density_update_ranges(self, Y, tmin, deltat, extent, ranges, grid_size=(500, 500), linewidth=7, grid=None):
        """``trace_density_update`` with ranges (E, T, 2) int64 = (first sample, count) of every trace: only the stretch
        of a trace inside its own range is drawn and checked against the extent, a trace with count < 2 draws nothing --
        the grid of ``fuzzy_moment_rate`` (plotting/ffi.py:41-79), whose curves each cover their own stretch of the time
        axis (zero padding would draw segments along rate 0).  ranges None: ``trace_density_update``."""
        return self._trace_density(Y, tmin, deltat, extent, ranges, grid_size, linewidth, grid)

    def _trace_density(self, Y, tmin, deltat, extent, ranges, grid_size, linewidth, grid):
        self._adopt_stream(Y)
        y = as_input(Y)
        if y.ndim != 3:
            raise ValueError("trace_density_update: Y must be (E, T, N)")
        E, T, N = (int(v) for v in y.shape)
        ny, nx = (int(v) for v in grid_size)
        tm = on_side(tmin, y, np.float64, (T,), "trace_density_update: tmin", broadcast=True)
        ext = on_side(extent, y, np.float64, (T, 4), "trace_density_update: extent", broadcast=True)
        grid = checked(grid, y, (T, ny, nx), np.float64, "trace_density_update: grid", of="Y", zero=True)
        if ranges is None:
            check(self._lib.beatamd_trace_density_update(self._h, E, T, N, ptr(y), ptr(tm), float(deltat), ptr(ext), ny, nx,
                                                         float(linewidth), ptr(grid)))
            return grid
        rg = on_side(ranges, y, np.int64, (E, T, 2), "trace_density_update: ranges")
        check(self._lib.beatamd_trace_density_update_ranges(self._h, E, T, N, ptr(y), ptr(tm), float(deltat), ptr(ext), ptr(rg),
                                                            ny, nx, float(linewidth), ptr(grid)))
        return grid

    def halfspace_displacements_batch(self, kinds, params, east, north, nu=0.25):
        """params (C, nsrc, 10) -> (C, nsrc, nobs, 3) = (north, east, up) [m]"""
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        prm = as_input(params)
        self._adopt_stream(prm)
        Cn, nsrc = int(prm.shape[0]), int(prm.shape[1])
        if tuple(prm.shape[1:]) != (kinds.size, 10):
            raise ValueError("params must be (C, %d, 10)" % kinds.size)
        e, n = as_input(east), as_input(north)
        nobs = int(e.numel()) if is_dev(e) else int(e.size)
        out = new(prm, (Cn, nsrc, nobs, 3))
        check(self._lib.beatamd_halfspace_displacements_batch(self._h, Cn, nsrc, ptr(kinds), ptr(prm), nobs,
                                                              ptr(e), ptr(n), float(nu), ptr(out)))
        return out

    # -- geodetic FFI library and resolution-based discretization (csrc/geolib.hip, csrc/resolution.hip)
    def geo_gf_library(self, params, east, north, los, odw, nu=0.25, device=False):
        """params (nrows, 10) unit sources in the slots of halfspace_displacements_batch -> G (nrows, nobs) =
        (disp * los).sum(1) * odw of every row (ffi/base.py:804-821), all rows in one launch.  device: return a
        torch tensor on this context's GPU (inputs may be on either side)"""
        side = (bool(device) or is_dev(params), self.device)
        nrows = int(params.shape[0])
        nobs = int(odw.shape[0])
        prm = on_side(params, side, np.float64, (nrows, 10), "params")
        e = on_side(east, side, np.float64, (nobs,), "east")
        n = on_side(north, side, np.float64, (nobs,), "north")
        lo = on_side(los, side, np.float64, (nobs, 3), "los")
        w = on_side(odw, side, np.float64, (nobs,), "odw")
        self._adopt_stream(prm)
        G = new(side, (nrows, nobs))
        check(self._lib.beatamd_geo_gf_library(self._h, nrows, ptr(prm), nobs, ptr(e), ptr(n), ptr(lo), ptr(w),
                                               float(nu), ptr(G)))
        return G

    def smoothing_correlated(self, patches_coords, correlation_function="gaussian", device=False):
        """get_smoothing_operator_correlated (models/laplacian.py:261-298) on the device: coords (P, 3) [km] -> L (P, P);
        the column sums add the rows in ascending order (beat_amd.models.laplacian states the same order on the host)"""
        kinds = {"gaussian": 0, "exponential": 1}
        if correlation_function not in kinds:
            raise ValueError('Resolution based discretization does not support "nearest_neighbor" correlation function!')
        side = (bool(device) or is_dev(patches_coords), self.device)
        P = int(patches_coords.shape[0])
        c = on_side(patches_coords, side, np.float64, (P, 3), "patches_coords")
        self._adopt_stream(c)
        L = new(side, (P, P))
        check(self._lib.beatamd_smoothing_correlated(self._h, P, ptr(c), kinds[correlation_function], ptr(L)))
        return L

    def model_resolution(self, gfs, L, epsilon):
        """gfs (P, nobs) library rows, L (P, P) -> (R (P, P), diag (P,)) with R = inv(G^T G + eps^4 L^T L) . G^T G for
        G = gfs.T (ffi/fault.py:1805-1815); same side as ``gfs``; numpy.linalg.LinAlgError if the normal matrix is not
        positive definite"""
        side = (is_dev(gfs), self.device)
        P, nobs = int(gfs.shape[0]), int(gfs.shape[1])
        g = on_side(gfs, side, np.float64, (P, nobs), "gfs")
        Lm = on_side(L, side, np.float64, (P, P), "L")
        self._adopt_stream(g)
        R, d = new(side, (P, P)), new(side, (P,))
        check(self._lib.beatamd_model_resolution(self._h, P, nobs, ptr(g), ptr(Lm), float(epsilon), ptr(R), ptr(d)))
        return R, d

    def division_rating(self, widths, lengths, centers, bottom_depths, depth_penalty, data_coords, mean_R):
        """the division penalties of ffi/fault.py:1884-1929: widths, lengths (P,) [km], centers (P, 3) [km],
        bottom_depths (P,) [m] of each patch's subfault, data_coords (nobs, 2) [km] east / north, mean_R (P,) ->
        (rating (P,), patch_data_distance_mins (P,)); same side as ``mean_R``"""
        side = (is_dev(mean_R), self.device)
        P, nobs = int(mean_R.shape[0]), int(data_coords.shape[0])
        w = on_side(widths, side, np.float64, (P,), "widths")
        ln = on_side(lengths, side, np.float64, (P,), "lengths")
        c = on_side(centers, side, np.float64, (P, 3), "centers")
        b = on_side(bottom_depths, side, np.float64, (P,), "bottom_depths")
        e = on_side(data_coords, side, np.float64, (nobs, 2), "data_coords")
        m = on_side(mean_R, side, np.float64, (P,), "mean_R")
        self._adopt_stream(m)
        rating, dmin = new(side, (P,)), new(side, (P,))
        check(self._lib.beatamd_division_rating(self._h, P, nobs, ptr(w), ptr(ln), ptr(c), ptr(b), float(depth_penalty),
                                                ptr(e), ptr(m), ptr(rating), ptr(dmin)))
        return rating, dmin

    def chol_inverse_batch(self, covs):
        """covs (nd, n, n) -> (W (nd, n, n) upper triangular = cholesky(inv(C)).T, log_pdet (nd,));
        numpy or torch-cuda in, same kind out; numpy.linalg.LinAlgError if not positive definite"""
        if is_dev(covs):
            self._adopt_stream(covs)
        C = as_input(covs)
        nd, n = int(C.shape[0]), int(C.shape[1])
        W = new(C, (nd, n, n))
        lp = new(C, (nd,))
        check(self._lib.beatamd_chol_inverse_batch(self._h, nd, n, ptr(C), ptr(W), ptr(lp)))
        return W, lp

    def chol_inverse_batch_flags(self, covs):
        """like chol_inverse_batch, but a matrix that is not positive definite is reported in the
        returned int32 flags (nd,) instead of raising: -> (W, log_pdet, not_psd)"""
        if is_dev(covs):
            self._adopt_stream(covs)
        C = as_input(covs)
        nd, n = int(C.shape[0]), int(C.shape[1])
        W = new(C, (nd, n, n))
        lp = new(C, (nd,))
        bad = new(C, (nd,), np.int32)
        check(self._lib.beatamd_chol_inverse_batch_flags(self._h, nd, n, ptr(C), ptr(W), ptr(lp), ptr(bad)))
        return W, lp, bad

    def factor_compact(self, factor):
        """tall proposal factor (K, n) -> upper-triangular R (n, n) with R^T R = factor^T factor, or
        None when the Gram matrix is not numerically positive definite"""
        if is_dev(factor):
            self._adopt_stream(factor)
        F = as_input(factor)
        K, n = int(F.shape[0]), int(F.shape[1])
        R = new(F, (n, n))
        try:
            check(self._lib.beatamd_factor_compact(self._h, K, n, ptr(F), ptr(R)))
        except np.linalg.LinAlgError:
            return None
        return R

    def whitening_ratio_batch(self, W_new, W_old):
        """M (nd, n, n) = W_new . inv(W_old) for upper-triangular whitening operators"""
        Wn, Wo = as_input(W_new), as_input(W_old)
        if Wn.shape != Wo.shape or Wn.ndim != 3:
            raise ValueError("W_new and W_old must both be (nd, n, n)")
        M = new(Wn, tuple(Wn.shape))
        check(self._lib.beatamd_whitening_ratio_batch(self._h, int(Wn.shape[0]), int(Wn.shape[1]), ptr(Wn),
                                                      ptr(Wo), ptr(M)))
        return M

    def unwhiten_traces(self, W, X):
        """X (nd, n) <- inv(W[t]) . X[t] for upper-triangular W (nd, n, n), in place (back substitution)"""
        Wd = as_input(W)
        if Wd.ndim != 3 or Wd.shape[1] != Wd.shape[2] or tuple(X.shape) != (Wd.shape[0], Wd.shape[1]):
            raise ValueError("W must be (nd, n, n) and X (nd, n)")
        if not is_canonical(X):
            raise ValueError("X must be a contiguous float64 array / tensor (updated in place)")
        check(self._lib.beatamd_unwhiten_traces(self._h, int(Wd.shape[0]), int(Wd.shape[1]), ptr(Wd), ptr(X)))
        return X

    def ffi_model_update_data(self, model_id, wavemap_index, data):
        d = as_input(data)
        check(self._lib.beatamd_ffi_model_update_data(self._h, int(model_id), int(wavemap_index), ptr(d)))

    def whiten_rows_batch(self, rows, W):
        """rows (B, R, N) device tensor, in place: rows[b] <- rows[b] . W[b]^T for all datasets in one call
        (W (B, N, N) numpy or device; upper-triangular operators need no second buffer)"""
        self._adopt_stream(rows)
        if rows.dim() != 3 or not rows.is_contiguous():
            raise ValueError("whiten_rows_batch: rows must be a contiguous (B, R, N) device tensor")
        Wc = as_input(W)
        if tuple(Wc.shape) != (rows.shape[0], rows.shape[2], rows.shape[2]):
            raise ValueError("whiten_rows_batch: W must be (%d, %d, %d)" % (rows.shape[0], rows.shape[2], rows.shape[2]))
        check(self._lib.beatamd_whiten_rows_batch(self._h, ptr(rows), int(rows.shape[0]), int(rows.shape[1]),
                                                  int(rows.shape[2]), ptr(Wc)))
        return rows

    def whiten_rows(self, rows, W):
        """rows (R, N) device tensor, in place: rows <- rows . W^T"""
        self._adopt_stream(rows)
        Wc = as_input(W)
        check(self._lib.beatamd_whiten_rows(self._h, ptr(rows), int(rows.shape[0]), int(rows.shape[1]),
                                            ptr(Wc)))
        return rows


_contexts = {}


def get_context(device=None):
    """Process-wide context of a device (default: LOCAL_RANK or 0)."""
    import os
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    ctx = _contexts.get(device)
    if ctx is None or ctx._h is None:
        ctx = Context(device)
        _contexts[device] = ctx
    return ctx
