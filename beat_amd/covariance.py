"""
Noise-covariance structures and estimators -- counterpart of beat/covariance.py (the parts
that feed the sampler's likelihood weights).  The O(n^2) estimators run on the GPU.

What is bitwise the reference and what is not (tests/test_gpu_covariance_edges.py):

- ``autocovariance[_batch]``: bitwise the reference's double loop (covariance.py:716-736) for host and
  device input alike.  The mean of a device trace is taken by the kernel in numpy's summation order;
  ``torch.mean`` sums in another order and changed about a third of the values in the last bit.
- ``scaled_toeplitz_batch``: bitwise ``toeplitz(coeffs) * stds[:, None] * stds[None, :]``.
- ``running_window_rms_batch`` (device): running sums instead of ``numpy.convolve``; equal to rounding.
- ``k_nearest_neighbor_rms`` / ``non_toeplitz_covariance_2d[_batch]`` (csrc/noise2d.hip): the radius and the neighbour sets
  are the reference's bit for bit (exact ties included); the KD-tree returns a point's neighbours in no defined order, so
  the reference's last bits of ``stds`` are not defined either -- the kernel sums in ONE stated order that depends on the
  point and the scene size alone (tests/noise2d_ref.py restates it bit for bit), within (count + 3) 2^-53 of the reference.
- the whitening operator and log-determinant (``chol_inverse_batch[_flags]``): another factorisation
  order than the reference's ``cholesky(inv(C))``; within c n u kappa(C) (u = 2^-53, c = 4) of it.
"""
import logging

import numpy as np

from ._marshal import upload
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


def k_nearest_neighbor_rms(coords, data, k=None, max_dist_perc=0.2):
    """covariance.py:774-811: running rms on irregularly sampled 2-d data -- per point the sample standard deviation
    (ddof = 1) of the data over all points within ``max_dist_perc`` of the largest point distance.  coords (n, 2), data (n,);
    numpy or torch-cuda, same kind out.  Only the ``max_dist_perc`` branch runs here (``beatamd_ball_rms_batch``); the
    ``k`` nearest neighbours branch is not offered."""
    if k and max_dist_perc:
        raise ValueError("Either k or max_dist_perc should be defined!")
    if k is not None:
        raise NotImplementedError("k_nearest_neighbor_rms: the k nearest neighbours branch is not implemented, "
                                  "use max_dist_perc")
    if max_dist_perc is None:
        raise ValueError("Either k or max_dist_perc should be defined!")
    n = int(data.shape[0])
    return get_context().ball_rms_batch(coords, data, [n], max_dist_perc)[2]


def toeplitz_covariance_2d(coords, data, max_dist_perc=0.2):
    """covariance.py:814-828 -> (toeplitz matrix, stds); host arrays"""
    from scipy.linalg import toeplitz
    coords, data = np.ascontiguousarray(coords, dtype=np.float64), np.ascontiguousarray(data, dtype=np.float64)
    stds = k_nearest_neighbor_rms(coords=coords, data=data, max_dist_perc=max_dist_perc)
    with np.errstate(invalid="ignore", divide="ignore"):
        coeffs = autocovariance(data / stds)
    return toeplitz(coeffs), stds


def non_toeplitz_covariance_2d(coords, data, max_dist_perc):
    """covariance.py:831-848: scaled non-Toeplitz covariance for non-stationary errors of 2-d geospatial data"""
    coords, data = np.ascontiguousarray(coords, dtype=np.float64), np.ascontiguousarray(data, dtype=np.float64)
    return non_toeplitz_covariance_2d_batch(coords, data, [data.size], max_dist_perc)[0]


def non_toeplitz_covariance_2d_batch(coords, data, sizes, max_dist_perc, stds=None):
    """All scenes of a geodetic composite: coords (Ntot, 2) and data (Ntot,) concatenated over datasets of ``sizes``
    points -> list of (n_i, n_i) matrices ``toeplitz(autocovariance(data_i / stds_i)) * stds_i stds_i^T``; numpy or
    torch-cuda in, same kind out.  One launch group for the neighbourhood statistic of all scenes, then the existing
    autocovariance and scaled-Toeplitz kernels per scene (their batches share one length).  A scene with a point that has
    no neighbour comes back with NaN, as in the reference.  stds: the statistic where the caller has it already."""
    ctx = get_context()
    if stds is None:
        stds = ctx.ball_rms_batch(coords, data, sizes, max_dist_perc)[2]
    out, o = [], 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for n in (int(n) for n in sizes):
            s = stds[o:o + n].reshape(1, n)
            coeffs = ctx.autocovariance_batch((data[o:o + n].reshape(1, n) / s))
            out.append(ctx.scaled_toeplitz_batch(coeffs, s)[0])
            o += n
    return out


NoiseStructureCatalog2d = {
    "import": ones_data_covariance,
    "non-toeplitz": ones_data_covariance,
}


def available_noise_structures_2d():
    return list(NoiseStructureCatalog2d.keys())


class GeodeticNoiseAnalyser(object):
    """covariance.py:154-233: the data covariance of a geodetic dataset by ``config.structure`` ("import": the dataset's
    own, "non-toeplitz": estimated from the residual of ``result`` for SAR scenes; any other dataset type keeps its
    ``covariance.data``).

    config: anything with ``structure`` and ``max_dist_perc``.  dataset: ``typ``, ``id``, ``ncoords``, ``covariance``,
    ``east_shifts`` / ``north_shifts`` [m]; where it has ``update_local_coords`` (pyrocko's projection about the event) it
    is called with ``events[0]`` as in the reference, otherwise the shifts are taken as they are."""

    def __init__(self, config, events=None):
        avail = available_noise_structures_2d()
        if config.structure not in avail:
            raise AttributeError('Selected noise structure "%s" not supported! Implemented'
                                 " noise structures: %s" % (config.structure, ", ".join(avail)))
        self.events = events
        self.config = config

    def get_structure(self, dataset):
        return NoiseStructureCatalog2d[self.config.structure](dataset.ncoords)

    def do_import(self, dataset):
        if dataset.covariance.data is not None:
            return dataset.covariance.data
        raise ValueError("Data covariance for dataset %s needs to be defined!" % dataset.id)

    def do_non_toeplitz(self, dataset, result):
        if dataset.typ == "SAR":
            if hasattr(dataset, "update_local_coords"):
                dataset.update_local_coords(self.events[0])
            coords = np.vstack([dataset.east_shifts, dataset.north_shifts]).T
            scaling = non_toeplitz_covariance_2d(coords, result.processed_res, max_dist_perc=self.config.max_dist_perc)
        else:
            scaling = dataset.covariance.data
        if np.isnan(scaling).any():
            raise ValueError("Estimated Non-Toeplitz covariance matrix for dataset %s contains Nan! "
                             "Please increase 'max_dist_perc'!" % dataset.id)
        return scaling

    def get_data_covariance(self, dataset, result=None):
        covariance_structure = self.get_structure(dataset)
        if self.config.structure == "import":
            scaling = self.do_import(dataset)
        elif self.config.structure == "non-toeplitz":
            scaling = self.do_non_toeplitz(dataset, result)
        return ensure_cov_psd(scaling * covariance_structure)


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
        from .models.problem import refuse_spectrum_wavemaps
        refuse_spectrum_wavemaps(getattr(logp_func, "problem", None), "NoiseCovarianceUpdate")
        self.f = logp_func
        self.last_ms, self.n_repaired, self.n_updates = 0.0, 0, 0

    def data_covariances(self, q_map, wavemap_index=0):
        """-> (covariances [T, n, n] torch-cuda, residuals [T, n]) at the point q_map"""
        import torch
        f = self.f
        dev = torch.device("cuda", f.ctx.device)
        q = upload(np.asarray(q_map, dtype=np.float64).reshape(1, -1), dev)
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
        wo = w_old.to(dev) if torch.is_tensor(w_old) else upload(w_old, dev)
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

    @staticmethod
    def _base_of(c, t, dev):
        """``data + pred_g`` of one dataset on the device; t: a device-resident data term to take instead of ``c``'s.  A data
        term that already lives on the device is the base as it is (``pred_g`` missing) or takes the uploaded ``pred_g``
        there: no host round trip.  Host arrays are summed on the host and uploaded."""
        if t is None and hasattr(c._terms["data"], "is_cuda"):
            t = c._terms["data"]
        if t is None:
            return upload(c._term("data") + c._term("pred_g"), dev, np.float64)
        g = c._terms["pred_g"]
        if g is None:
            return t
        return t + (g.to(dev) if hasattr(g, "is_cuda") else upload(g, dev, np.float64))

    def _bases(self, dev, data_terms=None):
        """the datasets' ``data + pred_g`` on the device: kept from call to call per pair of arrays of the Covariance
        objects; formed anew where the caller hands the data terms over (``data_terms``: one device tensor or None each)"""
        if data_terms is not None:
            return [self._base_of(c, t, dev) for c, t in zip(self.covariances, data_terms)]
        key = [(id(c._terms["data"]), id(c._terms["pred_g"])) for c in self.covariances]
        if self._base is None or key != self._base_key:
            self._base = [self._base_of(c, None, dev) for c in self.covariances]
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

    def compute(self, q_map, data_terms=None):
        """everything up to the installation -> (operators, log-determinants, pred_v terms, repaired data terms or None).
        data_terms: device tensors to take for the datasets' ``data`` instead of the Covariance objects' (the noise update
        hands its new estimates over before anything is installed)"""
        import torch
        from .heart import Covariance
        f = self.f
        dev = torch.device("cuda", f.ctx.device)
        sizes = list(f.problem.geodetic.sizes)
        X = self.crust_synthetics(q_map)
        cov_pv = f.ctx.pred_covariance_batch(X, sizes)                          # the raw term, for covariance.pred_v
        total = f.ctx.pred_covariance_batch(X, sizes, base=self._bases(dev, data_terms))    # data + pred_g + pred_v
        Ws, lps, pvs, datas = [], [], [], []
        for i, cov in enumerate(self.covariances):
            W, lp, bad = f.ctx.chol_inverse_batch_flags(total[i].unsqueeze(0))
            pv, data = cov_pv[i], None
            if int(bad[0]):
                self.n_host_route += 1
                pv = ensure_cov_psd(cov_pv[i].cpu().numpy())                    # geodetic.py:1189
                try:
                    if data_terms is not None and data_terms[i] is not None:
                        data = ensure_cov_psd(data_terms[i].cpu().numpy())      # covariance.py:233
                    host = Covariance(data=cov.data if data is None else data, pred_g=cov.pred_g, pred_v=pv)
                    W, lp = torch.from_numpy(host.chol_inverse).to(dev), float(host.log_pdet)
                except np.linalg.LinAlgError as e:
                    raise np.linalg.LinAlgError("geodetic dataset %d: the total covariance (data + pred_g + pred_v) is not "
                                                "positive definite: %s" % (i, e))
            else:
                W, lp = W[0], float(lp[0])
            Ws.append(W)
            lps.append(lp)
            pvs.append(pv)
            datas.append(data)
        return Ws, lps, pvs, datas

    def update_weights(self, q_map):
        import time
        f = self.f
        self.n_updates += 1
        if self.ensemble.n_variations <= self.thresh:
            logger.info("Not updating geodetic velocity model-covariances because number of model variations is too low! "
                        "< %i" % self.thresh)
            self.last_ms = 0.0
            return
        f.ctx.synchronize()
        t0 = time.perf_counter()
        Ws, lps, pvs, _ = self.compute(q_map)
        f.update_geodetic_weights(Ws, lps)
        for cov, pv, lp in zip(self.covariances, pvs, lps):
            cov.pred_v = pv
            cov.slog_pdet.set_value(np.float64(lp))
        f.ctx.synchronize()
        self.last_ms = (time.perf_counter() - t0) * 1e3


class GeodeticNoiseCovarianceUpdate(object):
    """The data half of the geodetic ``update`` of ``smc_sample``: with ``noise_estimator.structure == "non-toeplitz"``
    the reference re-estimates every SAR scene's DATA covariance from the residual at the stage's MAP point before it adds
    the prediction covariances and factorises (GeodeticDistributerComposite.update_weights, geodetic.py:1130-1202 ->
    analyse_noise :143-174 -> GeodeticNoiseAnalyser.do_non_toeplitz, covariance.py:193-210 -> non_toeplitz_covariance_2d
    :831-848 -> toeplitz_covariance_2d :814-828 -> k_nearest_neighbor_rms :774-811):

        res = d - mu - sum of corrections at the point (no odw factor: assemble_results :201-232, get_synthetics :1086-1128)
        stds = k_nearest_neighbor_rms(coords, res, max_dist_perc) -> coeffs = autocovariance(res / stds) ->
        C_d = toeplitz(coeffs) * stds stds^T -> covariance.data -> chol_inverse, log_pdet of data + pred_g + pred_v -> weights

    on the device: ``beatamd_ffi_geo_residuals_batch`` (the model's own mu), ``beatamd_ball_rms_batch``,
    ``beatamd_autocovariance_batch``, ``beatamd_scaled_toeplitz_batch``, the sum of the terms,
    ``beatamd_chol_inverse_batch_flags``, ``LogpForwFunc.update_geodetic_weights``.  No matrix visits the host.

    THE RESIDUAL.  ``mu`` is ``geodetic_residuals(q, residuals=False)``, the likelihood's own synthetics bit for bit.  The
    data and every correction's basis columns are uploaded once; per update ``res = d - mu`` and then, term by term in the
    order the model subtracts them (``corrections.correction_tables``), ``res_i = res_i - corr`` with ``corr = B[:, 0] *
    c_0`` and ``corr = corr + B[:, k] * c_k`` for the further columns, the coefficients read from the point (or the
    problem's fixed values): one IEEE operation per element and step, so numpy gives the same bits.

    DEVIATION.  The reference passes the DATA term alone through ``utility.ensure_cov_psd`` (covariance.py:233) before the
    prediction terms are added.  Here the factorisation of the TOTAL decides: a dataset whose total the device
    factorisation flags takes the reference's route on the host -- ``ensure_cov_psd(C_d)``, then
    ``beat_amd.heart.Covariance`` for operator and log-determinant (``n_host_route`` counts them); if that fails too,
    ``numpy.linalg.LinAlgError`` naming the dataset is raised.  Whatever is raised -- that, or the reference's ValueError
    for a scene whose estimate contains NaN (a point without a neighbour, or a neighbourhood of equal values) -- the
    model's weights and the Covariance objects are untouched: everything is computed before anything is installed.

    coords: one (n_i, 2) array of local east / north shifts [m] per dataset (the caller's: the reference derives them with
    pyrocko's ``update_local_coords``).  covariances: the datasets' ``beat_amd.heart.Covariance`` objects; ``data`` becomes
    the new term as a device tensor that is downloaded only when read, ``slog_pdet`` follows.  typs: the datasets' types,
    default all "SAR"; any other type keeps its data term (covariance.py:201-202).  velocity: a
    ``VelocityModelCovarianceUpdate`` of the same model and Covariance objects -- the update then runs in the reference's
    order, data term first, ``pred_v`` from the ensemble at the same point next, and ONE factorisation per dataset of the
    final total; the result is bit for bit that of ``CovarianceUpdates(noise, velocity)``, which factorises twice."""

    def __init__(self, logp_func, coords, covariances, max_dist_perc, typs=None, velocity=None):
        g = logp_func.problem.geodetic
        if g is None:
            raise ValueError("the model has no geodetic composite")
        if not hasattr(logp_func, "geodetic_residuals"):
            raise NotImplementedError("the geodetic noise update needs the whole geodetic composite in one compiled model")
        nd = len(g.sizes)
        self.f, self.covariances = logp_func, list(covariances)
        if len(self.covariances) != nd:
            raise ValueError("%d covariances for %d geodetic datasets" % (len(self.covariances), nd))
        coords = [np.ascontiguousarray(c, dtype=np.float64) for c in coords]
        if len(coords) != nd:
            raise ValueError("%d coordinate arrays for %d geodetic datasets" % (len(coords), nd))
        for i, (c, n) in enumerate(zip(coords, g.sizes)):
            if c.shape != (n, 2):
                raise ValueError("geodetic dataset %d: coordinates of shape %s, expected (%d, 2)" % (i, c.shape, n))
        self.typs = ["SAR"] * nd if typs is None else list(typs)
        if len(self.typs) != nd:
            raise ValueError("%d dataset types for %d geodetic datasets" % (len(self.typs), nd))
        if not np.isfinite(max_dist_perc):
            raise ValueError("max_dist_perc must be finite")
        if velocity is not None and (velocity.f is not logp_func or
                                     any(a is not b for a, b in zip(velocity.covariances, self.covariances))):
            raise ValueError("the velocity update must act on the same model and Covariance objects")
        self.coords, self.max_dist_perc, self.velocity = coords, float(max_dist_perc), velocity
        self.sar = [i for i, t in enumerate(self.typs) if t == "SAR"]
        self._dev = None
        self.last_ms, self.n_updates, self.n_host_route = 0.0, 0, 0

    def _resident(self):
        """what is uploaded once: the data, the SAR scenes' coordinates, the correction terms' basis columns"""
        import torch
        from .models.corrections import correction_tables
        if self._dev is None:
            f = self.f
            g = f.problem.geodetic
            dev = torch.device("cuda", f.ctx.device)
            up = lambda a: upload(a, dev, np.float64)   # noqa: E731
            ds, ncol, basis, offs, fixs, kind, earth = correction_tables(g.corrections, g.sizes, f.problem.layout, g.fixed,
                                                                         kinds=True)
            self._dev = dict(dev=dev, data=up(g.data),
                             terms=list(zip(ds, [up(B.T) for B in basis], offs, fixs, kind, earth)),
                             coords=up(np.concatenate([self.coords[i] for i in self.sar])) if self.sar else None)
        return self._dev

    def residuals(self, q_map):
        """(Nobs,) torch-cuda: ``d - mu - sum of corrections`` at the point, without the odw factor (the class docstring
        says how)"""
        import torch
        from .models.corrections import KIND_EULER_POLE, EarthModel, pole_coefficients
        r = self._resident()
        g = self.f.problem.geodetic
        q = np.ascontiguousarray(q_map, dtype=np.float64).ravel()
        mu = self.f.geodetic_residuals(torch.from_numpy(q.reshape(1, -1)).to(r["dev"]), residuals=False)[0]
        res = r["data"] - mu
        starts = np.concatenate([[0], np.cumsum(g.sizes)])
        for d, Bt, off, fix, kind, earth in r["terms"]:
            coef = [float(q[o]) if o >= 0 else float(v) for o, v in zip(off, fix)]
            if kind == KIND_EULER_POLE:     # (pole_lat, pole_lon, omega) -> omega' p, the host statement of k_pole_coef
                coef = [float(v) for v in pole_coefficients(coef[0], coef[1], coef[2], EarthModel(*earth))]
            corr = Bt[0] * coef[0]
            for k in range(1, len(coef)):
                corr = corr + Bt[k] * coef[k]
            a, b = int(starts[d]), int(starts[d + 1])
            res[a:b] = res[a:b] - corr
        return res

    def data_covariances(self, q_map):
        """-> (one (n_i, n_i) torch-cuda matrix per dataset, None where the dataset is no SAR scene; residuals (Nobs,);
        stds of the SAR scenes, concatenated).  Raises the reference's ValueError where an estimate contains NaN."""
        import torch
        f = self.f
        g = f.problem.geodetic
        r = self._resident()
        res = self.residuals(q_map)
        out = [None] * len(g.sizes)
        if not self.sar:
            return out, res, None
        starts = np.concatenate([[0], np.cumsum(g.sizes)])
        sizes = [g.sizes[i] for i in self.sar]
        if len(self.sar) == len(g.sizes):
            rs = res
        else:
            rs = torch.cat([res[int(starts[i]):int(starts[i + 1])] for i in self.sar])
        rs = rs.contiguous()
        _, _, stds = f.ctx.ball_rms_batch(r["coords"], rs, sizes, self.max_dist_perc)
        # a NaN or a zero among the stds is a NaN in the matrix (0 / 0 on the diagonal at the latest): one read of one flag
        bad = ~torch.isfinite(stds) | (stds == 0.0)
        if bool(bad.any()):
            o = np.concatenate([[0], np.cumsum(sizes)])
            first = int(torch.nonzero(bad)[0, 0])
            d = self.sar[int(np.searchsorted(o, first, side="right")) - 1]
            raise ValueError("Estimated Non-Toeplitz covariance matrix for dataset %s contains Nan! "
                             "Please increase 'max_dist_perc'!" % d)                  # covariance.py:204-208
        for i, C in zip(self.sar, non_toeplitz_covariance_2d_batch(None, rs, sizes, None, stds=stds)):
            out[i] = C
        return out, res, stds

    def update_weights(self, q_map):
        import time
        import torch
        from .heart import Covariance
        f = self.f
        f.ctx.synchronize()
        t0 = time.perf_counter()
        dev = torch.device("cuda", f.ctx.device)
        Cd, _, _ = self.data_covariances(q_map)
        vel = self.velocity
        if vel is not None and vel.ensemble.n_variations <= vel.thresh:
            logger.info("Not updating geodetic velocity model-covariances because number of model variations is too low! "
                        "< %i" % vel.thresh)
            vel.n_updates += 1
            vel.last_ms = 0.0
            vel = None
        if vel is not None:
            # the reference's order: data term, pred_v at the same point, ONE factorisation of the final total
            routed = vel.n_host_route
            Ws, lps, pvs, datas = vel.compute(q_map, data_terms=Cd)
            self.n_host_route += vel.n_host_route - routed
            vel.n_updates += 1
        else:
            Ws, lps, pvs, datas = [], [], None, []
            for i, cov in enumerate(self.covariances):
                total, data = VelocityModelCovarianceUpdate._base_of(cov, Cd[i], dev), None
                pv = cov._terms["pred_v"]
                if pv is not None:
                    total = total + (pv.to(dev) if hasattr(pv, "is_cuda") else upload(pv, dev, np.float64))
                W, lp, bad = f.ctx.chol_inverse_batch_flags(total.unsqueeze(0))
                if int(bad[0]):
                    self.n_host_route += 1
                    try:
                        data = ensure_cov_psd(cov.data if Cd[i] is None else Cd[i].cpu().numpy())    # covariance.py:233
                        host = Covariance(data=data, pred_g=cov.pred_g, pred_v=cov.pred_v)
                        W, lp = torch.from_numpy(host.chol_inverse).to(dev), float(host.log_pdet)
                    except np.linalg.LinAlgError as e:
                        raise np.linalg.LinAlgError("geodetic dataset %d: the total covariance (data + pred_g + pred_v) is "
                                                    "not positive definite: %s" % (i, e))
                else:
                    W, lp = W[0], float(lp[0])
                Ws.append(W)
                lps.append(lp)
                datas.append(data)
        f.update_geodetic_weights(Ws, lps)
        for i, (cov, lp) in enumerate(zip(self.covariances, lps)):
            if datas[i] is not None:
                cov.data = datas[i]
            elif Cd[i] is not None:
                cov.data = Cd[i]
            if pvs is not None:
                cov.pred_v = pvs[i]
            cov.slog_pdet.set_value(np.float64(lp))
        f.ctx.synchronize()
        self.last_ms = (time.perf_counter() - t0) * 1e3
        if self.velocity is not None and vel is not None:
            vel.last_ms = self.last_ms
        self.n_updates += 1


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
