"""
Noise-covariance structures and estimators -- counterpart of beat/covariance.py (the parts
that feed the sampler's likelihood weights).  The O(n^2) estimators run on the GPU.

What is bitwise the reference and what is not (tests/test_gpu_covariance_edges.py):

- ``autocovariance[_batch]``: bitwise the reference's double loop (covariance.py:716-736) for host and
  device input alike.  The mean of a device trace is taken by the kernel in numpy's summation order;
  ``torch.mean`` sums in another order and changed about a third of the values in the last bit.
- ``scaled_toeplitz_batch``: bitwise ``toeplitz(coeffs) * stds[:, None] * stds[None, :]``.
- ``running_window_rms_batch`` (device): running sums instead of ``numpy.convolve``; equal to rounding.
- the whitening operator and log-determinant (``chol_inverse_batch[_flags]``): another factorisation
  order than the reference's ``cholesky(inv(C))``; within c n u kappa(C) (u = 2^-53, c = 4) of it.
"""
import logging

import numpy as np

from .engine import get_context
from .utility import ensure_cov_psd, running_window_rms  # noqa: F401

logger = logging.getLogger("beat_amd.covariance")


def exponential_data_covariance(n, dt, tzero):
    """covariance.py:24-51: exp(-|ti - tj| / T0), Toeplitz"""
    i = np.arange(n)
    return np.exp(-np.abs(i[:, np.newaxis] - i[np.newaxis, :]) * (dt / tzero))


def identity_data_covariance(n, dt=None, tzero=None):
    """covariance.py:54-67"""
    return np.eye(n, dtype="float64")


def ones_data_covariance(n, dt=None, tzero=None):
    """covariance.py:70-83"""
    return np.ones((n, n), dtype="float64")


NoiseStructureCatalog = {
    "variance": identity_data_covariance,
    "exponential": exponential_data_covariance,
    "import": ones_data_covariance,
    "non-toeplitz": ones_data_covariance,
}


def available_noise_structures():
    return list(NoiseStructureCatalog.keys())


def autocovariance(data):
    """covariance.py:716-736 (bitwise the reference's double loop, evaluated on the GPU)"""
    d = np.ascontiguousarray(data, dtype=np.float64).reshape(1, -1)
    return get_context().autocovariance_batch(d)[0]


def autocovariance_batch(data):
    """data (nd, n) -> (nd, n); numpy or torch-cuda"""
    return get_context().autocovariance_batch(data)


def toeplitz_covariance(data, window_size):
    """covariance.py:739-751 -> (toeplitz matrix, stds)"""
    from scipy.linalg import toeplitz
    stds = running_window_rms(data, window_size=window_size, mode="same")
    coeffs = autocovariance(data / stds)
    return toeplitz(coeffs), stds


def non_toeplitz_covariance(data, window_size):
    """covariance.py:754-771: scaled non-Toeplitz covariance for non-stationary errors"""
    return non_toeplitz_covariance_batch(np.asarray(data, dtype=np.float64).reshape(1, -1),
                                         window_size)[0]


def non_toeplitz_covariance_batch(data, window_size):
    """All datasets of a wavemap at once: data (nd, n) -> (nd, n, n).  This is what
    SeismicNoiseAnalyser.do_non_toeplitz (covariance.py:333-395) computes per trace at every
    stage when update_covariances is on."""
    data = np.ascontiguousarray(data, dtype=np.float64)
    stds = np.stack([running_window_rms(d, window_size=window_size, mode="same") for d in data])
    ctx = get_context()
    coeffs = ctx.autocovariance_batch(np.ascontiguousarray(data / stds))
    return ctx.scaled_toeplitz_batch(coeffs, stds)


def get_data_covariances(structure, scalings):
    """covariance.py:413-427: cov_d = ensure_cov_psd(scaling * structure) per dataset"""
    return [ensure_cov_psd(s * structure) for s in scalings]


def running_window_rms_batch(data, window_size):
    """utility.running_window_rms(mode="same") of every row of a torch tensor (nd, n), on its device:
    sqrt of the running mean of squares, the window centred like numpy.convolve(..., "same")"""
    import torch
    nd, n = data.shape
    w = int(window_size)
    pad = torch.zeros((nd, w - 1), dtype=data.dtype, device=data.device)
    d2 = torch.cat([pad, data * data, pad], 1)
    cs = torch.cat([torch.zeros((nd, 1), dtype=data.dtype, device=data.device), torch.cumsum(d2, 1)], 1)
    full = (cs[:, w:] - cs[:, :-w]) / float(w)          # "full" convolution with ones(w) / w: n + w - 1 values
    o = (w - 1) // 2
    return torch.sqrt(torch.clamp(full[:, o:o + n], min=0.0))


class NoiseCovarianceUpdate(object):
    """The ``update`` argument of ``smc_sample``: at the end of every stage the reference calls
    ``update.update_weights(map_pt)`` and re-evaluates the population (sampler/smc.py:492-503).
    For the seismic composite with ``noise_estimator.structure == "non-toeplitz"`` that is
    (models/seismic.py:1509-1534, covariance.py:307-325, 397-427, heart.py:211-253):

        synthetics at the MAP point -> residuals per dataset -> window = n // 5 ->
        stds = running_window_rms -> coeffs = autocovariance(res / stds) ->
        C = toeplitz(coeffs) * stds stds^T -> ensure_cov_psd -> chol_inverse, log_pdet -> weights

    Everything up to the weights stays on the device (``beatamd_ffi_synthetics_batch``,
    ``_autocovariance_batch``, ``_scaled_toeplitz_batch``, ``_chol_inverse_batch_flags``).  The
    positive-definiteness check IS the device factorisation: only matrices it flags go to the host
    for the reference's eigenvalue repair (utility.repair_covariance, utility.py:1113-1138) and are
    factored again.  ``last_ms`` / ``n_repaired`` report the last update."""

    def __init__(self, logp_func):
        self.f = logp_func
        self.last_ms, self.n_repaired, self.n_updates = 0.0, 0, 0

    def data_covariances(self, q_map, wavemap_index=0):
        """-> (covariances [T, n, n] torch-cuda, residuals [T, n]) at the point q_map"""
        import torch
        f = self.f
        dev = torch.device("cuda", f.ctx.device)
        q = torch.as_tensor(np.ascontiguousarray(q_map, dtype=np.float64).reshape(1, -1)).to(dev)
        res = f.synthetics(q, wavemap_index, residuals=True)[0]            # seismic.py:1332
        wm = f.problem.wavemaps[wavemap_index]
        if getattr(wm, "is_prewhitened", False):
            # library rows and data of a pre-whitened model hold W_old G and W_old d: the model's residuals are
            # W_old (d - s).  The reference estimates the noise on d - s (covariance.py:307-325,
            # seismic.py:1509-1534): take W_old off again, r_t = inv(W_old,t) . res_t
            res = self._unwhiten(res, wm._whitened_with, dev)
        n = int(res.shape[1])
        window = n // 5
        if window == 0:
            raise ValueError("Length of trace too short! Please widen taper in time domain or frequency bands "
                             "in spectral domain.")                     # covariance.py:317-321
        stds = running_window_rms_batch(res, window)
        coeffs = f.ctx.autocovariance_batch((res / stds).contiguous())
        return f.ctx.scaled_toeplitz_batch(coeffs, stds.contiguous()), res

    def _unwhiten(self, res, w_old, dev):
        """rows r_t = inv(W_t) res_t for upper-triangular W [T, n, n] (host or device): one back substitution per
        dataset on the device (``beatamd_unwhiten_traces``; the first version formed the 64 inverses for this)"""
        import torch
        out = res.clone().contiguous()
        wo = w_old.to(dev) if torch.is_tensor(w_old) else torch.from_numpy(np.ascontiguousarray(w_old)).to(dev)
        self.f.ctx.unwhiten_traces(wo.contiguous(), out)
        return out

    def update_weights(self, q_map):
        import time
        import torch
        from .utility import repair_covariance
        f = self.f
        f.ctx.synchronize()
        t0 = time.perf_counter()
        self.n_repaired = 0
        for i, wm in enumerate(f.problem.wavemaps):
            covs, _ = self.data_covariances(q_map, i)
            W, logdet, bad = f.ctx.chol_inverse_batch_flags(covs)
            bad_idx = torch.nonzero(bad).ravel().tolist()
            for t in bad_idx:                                           # utility.ensure_cov_psd
                fixed = repair_covariance(covs[t].cpu().numpy())
                Wt, lt = f.ctx.chol_inverse_batch(torch.from_numpy(fixed[None]).to(covs.device))
                W[t], logdet[t] = Wt[0], lt[0]
            self.n_repaired += len(bad_idx)
            f.update_weights(i, W, logdet)
        f.ctx.synchronize()
        self.last_ms = (time.perf_counter() - t0) * 1e3
        self.n_updates += 1


class VelocityModelCovarianceUpdate(object):
    """The geodetic half of the ``update`` argument of ``smc_sample``: the velocity-model prediction covariance ``C_pv``
    of every geodetic dataset from an ensemble of Green's function libraries, each computed in a perturbed crust model
    (GeodeticDistributerComposite.update_weights, geodetic.py:1130-1202; heart.py:158-253):

        mu_k = sum_var G_{k,var}.T . slip_var at the MAP point, every variant k (raw: no odw, no corrections) ->
        cov_pv = numpy.cov(mu[:, dataset], rowvar=0) -> covariance.pred_v ->
        chol_inverse, log_pdet of data + pred_g + pred_v -> weights

    on the device: ``beatamd_geo_ensemble_stack``, ``beatamd_pred_covariance_batch`` onto the resident ``data + pred_g``,
    ``beatamd_chol_inverse_batch_flags``, ``LogpForwFunc.update_geodetic_weights``.  No matrix visits the host.

    DEVIATION.  The reference passes ``cov_pv`` alone through ``utility.ensure_cov_psd`` before adding it; with fewer
    variants than points it is rank deficient, so that always ends in the eigenvalue repair, which lifts the null space
    to eps.  Here the raw sample covariance is added and the factorisation of the TOTAL decides.  A dataset whose total the
    device factorisation flags takes the reference's own route on the host: ``ensure_cov_psd(cov_pv)``, then
    ``beat_amd.heart.Covariance`` for operator and log-determinant (``n_host_route`` counts them); if that fails too,
    ``numpy.linalg.LinAlgError`` naming the dataset is raised and the model's weights are untouched -- all new operators
    are computed before any is installed.

    covariances: the datasets' ``beat_amd.heart.Covariance`` objects; their ``pred_v`` is set to the new term as a device
    tensor that is downloaded only when read, ``slog_pdet`` follows.  ``data + pred_g`` is uploaded once per pair of
    arrays (assigning a new array to ``.data`` / ``.pred_g`` is seen; after changing one in place call
    ``refresh_base()``).  With ``thresh`` (5) variants or fewer nothing is computed or installed, as in the reference
    (geodetic.py:1151-1152, 1191-1195).  ``reference_crust_ind`` names the variant the model was compiled with (its row of
    the stack is the model's mu bit for bit)."""

    thresh = 5

    def __init__(self, logp_func, ensemble, covariances, reference_crust_ind=0):
        g = logp_func.problem.geodetic
        if g is None:
            raise ValueError("the model has no geodetic composite")
        self.f, self.ensemble, self.covariances = logp_func, ensemble, list(covariances)
        if len(self.covariances) != len(g.sizes):
            raise ValueError("%d covariances for %d geodetic datasets" % (len(self.covariances), len(g.sizes)))
        if list(ensemble.varnames) != list(logp_func.problem.slip_varnames):
            raise ValueError("the ensemble's slip variables %s are not the model's %s"
                             % (list(ensemble.varnames), list(logp_func.problem.slip_varnames)))
        if ensemble.nsamples != sum(g.sizes):
            raise ValueError("the ensemble's libraries have %d observations, the datasets %d" % (ensemble.nsamples, sum(g.sizes)))
        if reference_crust_ind not in ensemble.crust_inds:
            raise ValueError("crust variant %r is not in the ensemble %s" % (reference_crust_ind, ensemble.crust_inds))
        self.reference_crust_ind = reference_crust_ind
        self._base, self._base_key = None, None
        self.last_ms, self.n_updates, self.n_host_route = 0.0, 0, 0

    def refresh_base(self):
        """forget the uploaded ``data + pred_g`` (after an in-place change of a covariance's arrays)"""
        self._base, self._base_key = None, None

    def _bases(self, dev):
        import torch
        key = [(id(c._terms["data"]), id(c._terms["pred_g"])) for c in self.covariances]
        if self._base is None or key != self._base_key:
            self._base = [torch.from_numpy(np.ascontiguousarray(c._term("data") + c._term("pred_g"), dtype=np.float64)).to(dev)
                          for c in self.covariances]
            # (_term may have replaced a missing pred_g by zeros: the key is taken afterwards)
            self._base_key = [(id(c._terms["data"]), id(c._terms["pred_g"])) for c in self.covariances]
        return self._base

    def point_slips(self, q_map):
        """the slip variables of the point, in the model's order -> (nvar * npatches,) numpy"""
        lay = self.f.problem.layout
        q = np.ascontiguousarray(q_map, dtype=np.float64).ravel()
        P = self.ensemble.npatches
        return np.concatenate([q[lay.offsets[v]:lay.offsets[v] + P] for v in self.f.problem.slip_varnames])

    def crust_synthetics(self, q_map):
        """(K, Nobs) torch-cuda: the raw synthetics of every crust variant at the point (geodetic.py:1167-1176)"""
        import torch
        dev = torch.device("cuda", self.f.ctx.device)
        self.ensemble.init_optimization(self.f.ctx)
        return self.ensemble.stack_all(torch.from_numpy(self.point_slips(q_map)).to(dev))

    def update_weights(self, q_map):
        import time
        import torch
        from .heart import Covariance
        f = self.f
        self.n_updates += 1
        K = self.ensemble.n_variations
        if K <= self.thresh:
            logger.info("Not updating geodetic velocity model-covariances because number of model variations is too low! "
                        "< %i" % self.thresh)
            self.last_ms = 0.0
            return
        f.ctx.synchronize()
        t0 = time.perf_counter()
        dev = torch.device("cuda", f.ctx.device)
        sizes = list(f.problem.geodetic.sizes)
        X = self.crust_synthetics(q_map)
        cov_pv = f.ctx.pred_covariance_batch(X, sizes)                          # the raw term, for covariance.pred_v
        total = f.ctx.pred_covariance_batch(X, sizes, base=self._bases(dev))    # data + pred_g + pred_v
        Ws, lps, pvs = [], [], []
        for i, cov in enumerate(self.covariances):
            W, lp, bad = f.ctx.chol_inverse_batch_flags(total[i].unsqueeze(0))
            pv = cov_pv[i]
            if int(bad[0]):
                self.n_host_route += 1
                pv = ensure_cov_psd(cov_pv[i].cpu().numpy())                    # geodetic.py:1189
                try:
                    host = Covariance(data=cov.data, pred_g=cov.pred_g, pred_v=pv)
                    W, lp = torch.from_numpy(host.chol_inverse).to(dev), float(host.log_pdet)
                except np.linalg.LinAlgError as e:
                    raise np.linalg.LinAlgError("geodetic dataset %d: the total covariance (data + pred_g + pred_v) is not "
                                                "positive definite: %s" % (i, e))
            else:
                W, lp = W[0], float(lp[0])
            Ws.append(W)
            lps.append(lp)
            pvs.append(pv)
        f.update_geodetic_weights(Ws, lps)
        for cov, pv, lp in zip(self.covariances, pvs, lps):
            cov.pred_v = pv
            cov.slog_pdet.set_value(np.float64(lp))
        f.ctx.synchronize()
        self.last_ms = (time.perf_counter() - t0) * 1e3


class CovarianceUpdates(object):
    """Several updates as the one ``update=`` of ``smc_sample``: ``update_weights(q)`` calls each in order, as the reference
    problem loops over its composites (a joint run: the seismic noise update, then the geodetic prediction covariance)."""

    def __init__(self, *updates):
        self.updates = list(updates)
        self.last_ms, self.n_updates = 0.0, 0

    def update_weights(self, q_map):
        self.last_ms = 0.0
        for u in self.updates:
            u.update_weights(q_map)
            self.last_ms += float(getattr(u, "last_ms", 0.0))
        self.n_updates += 1
