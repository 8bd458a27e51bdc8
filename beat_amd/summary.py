"""
Posterior diagnostics of a whole stage population on the device -- what the reference computes with one forward model
per draw on one core:

  beat/models/seismic.py:564-634, geodetic.py:446-511    get_variance_reductions(point)
  beat/plotting/seismic.py:395-451                       form_result_ensemble: an ensemble of draws, their variance
                                                         reductions and synthetics (also plotting/geodetic.py:194-227,
                                                         580-610; station_variance_reductions, `beat summarize`)

Here a batch of draws is one call of the compiled model (``LogpForwFunc.variance_reductions`` / ``.synthetics``), and
the synthetics of an ensemble are reduced to mean / std / envelope where they are produced
(``Context.ensemble_moments_update``): an ensemble of [E, T, N] doubles never travels to the host unless asked for.
The functions take arrays (a population (n, nparams) in the order of the model's parameter vector), not stage
directories.  There is no CPU fallback: without a GPU they raise.
"""
import numpy as np

from .engine import get_context


def ensemble_indices(n, nensemble):
    """which of n draws make up an ensemble of ``nensemble``: the reference's
    ``floor(arange(0, n, float(n) / nensemble)).astype("int32")`` (plotting/seismic.py:400-402).

    DEVIATION: ``arange`` with a fractional step can come out one element longer than nensemble, the last one equal
    to n (n = 530, nensemble = 7 gives a trailing 530), which the reference would then fail to look up in its trace.
    Entries >= n are dropped here."""
    n, nensemble = int(n), int(nensemble)
    if n <= 0 or nensemble <= 0:
        return np.zeros(0, dtype=np.int32)
    raw = np.floor(np.arange(0, n, float(n) / nensemble)).astype("int32")
    return raw[raw < n]


def _ctx_of(f):
    ctx = getattr(f, "ctx", None)
    return ctx if ctx is not None else get_context()      # (raises without the library or a GPU)


def _is_tensor(a):
    return hasattr(a, "data_ptr") and not isinstance(a, np.ndarray)


def _to_device(ctx, a):
    import torch
    if _is_tensor(a):
        return a
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:%d" % ctx.device)


def posterior_variance_reductions(f, population, batch=512):
    """variance reduction of every dataset at every draw: population (n, nparams) -> (n, ndata), columns
    ``f.dataset_names``, as a fraction.  The draws go through the device in batches of ``batch``; numpy in -> numpy
    out, torch-cuda in -> tensor."""
    ctx = _ctx_of(f)
    n = int(population.shape[0])
    batch = max(int(batch), 1)
    if _is_tensor(population):
        import torch
        out = torch.empty((n, f.ndata), dtype=torch.float64, device=population.device)
        for a in range(0, n, batch):
            f.variance_reductions(population[a:a + batch].contiguous(), out=out[a:a + batch])
        return out
    population = np.ascontiguousarray(population, dtype=np.float64)
    out = np.empty((n, f.ndata))
    for a in range(0, n, batch):
        out[a:a + batch] = f.variance_reductions(_to_device(ctx, population[a:a + batch])).cpu().numpy()
    return out


def density_extent(mn, mx, tmin, deltat):
    """the default extent of ``fuzzy_waveforms`` (plotting/seismic.py:282-291) per target, from the envelope (T, N) that
    ``ensemble_moments_finish`` returns: [tmin, tmin + (N - 1) deltat, -a, a], a = max(|min|, |max|) over the target's
    samples.  numpy or torch-cuda in -> numpy (T, 4)."""
    if _is_tensor(mn):
        mn = mn.cpu().numpy()
    if _is_tensor(mx):
        mx = mx.cpu().numpy()
    mn, mx = np.asarray(mn, dtype=np.float64), np.asarray(mx, dtype=np.float64)
    T, N = mn.shape
    tmin = np.broadcast_to(np.asarray(tmin, dtype=np.float64), (T,))
    a = np.maximum(np.abs(mn.min(axis=1)), np.abs(mx.max(axis=1)))
    return np.stack([tmin, tmin + float(N - 1) * float(deltat), -a, a], axis=1)


def trace_density(Y, tmin, deltat, extent, grid_size=(500, 500), linewidth=7, grid=None, ctx=None):
    """density grid (T, ny, nx) of the traces Y (E, T, N): ``Context.trace_density_update`` on the default context"""
    ctx = ctx if ctx is not None else get_context()
    return ctx.trace_density_update(Y, tmin, deltat, extent, grid_size, linewidth, grid)


def result_ensemble(f, population, best, nensemble, wavemap_index=0, batch=512, keep_synthetics=False, density=None,
                    linewidth=7, tmin=0.0, deltat=1.0):
    """``form_result_ensemble`` (plotting/seismic.py:395-451) on arrays: ``nensemble`` draws of ``population``
    (n, nparams) picked by ``ensemble_indices`` next to the point ``best`` (nparams,).  Returns

      indices          (E,) int32
      var_reductions   (E + 1, ndata) in percent, the best point first (the reference's ordering, :437-450)
      moments          dict wavemap index -> dict(mean, std, min, max: (T, N) numpy) over the ENSEMBLE's synthetics of
                       that wavemap (std as numpy.std, ddof = 0), accumulated on the device from the output of
                       ``f.synthetics``; with ``keep_synthetics`` also ``synthetics`` (E, T, N) on the host.
                       wavemap_index: an index, a list of them, or None for every wavemap of the model.
                       density = (ny, nx): also ``density`` (T, ny, nx), the fuzzy-waveform grid of the ensemble at
                       ``linewidth`` (``Context.trace_density_update``), and its ``extent`` (T, 4) =
                       ``density_extent(min, max, tmin, deltat)``; tmin a scalar or (T,), the time of sample 0.  The
                       extent needs the whole ensemble's envelope, so the batches go through ``f.synthetics`` a second
                       time."""
    ctx = _ctx_of(f)
    idx = ensemble_indices(int(population.shape[0]), nensemble)
    batch = max(int(batch), 1)
    if _is_tensor(population):
        import torch
        ens = population[torch.as_tensor(idx.astype(np.int64), device=population.device)].contiguous()
        best_d = _to_device(ctx, best).reshape(1, -1).to(ens.device)
    else:
        ens = _to_device(ctx, np.asarray(population, dtype=np.float64)[idx])
        best_d = _to_device(ctx, np.asarray(best, dtype=np.float64).reshape(1, -1))
    import torch
    points = torch.cat([best_d, ens]).contiguous()
    var_reductions = posterior_variance_reductions(f, points, batch).cpu().numpy() * 100.0

    nwm = len(f.problem.wavemaps)
    if wavemap_index is None:
        which = list(range(nwm))
    elif np.ndim(wavemap_index) == 0:
        which = [int(wavemap_index)] if nwm else []
    else:
        which = [int(w) for w in wavemap_index]
    moments = {}
    E = int(ens.shape[0])
    for wi in which:
        T, N = f.problem.wavemaps[wi].data.shape
        state, seen, kept = None, 0, []
        for a in range(0, E, batch):
            syn = f.synthetics(ens[a:a + batch], wi)                      # (e, T, N) on the device
            state, seen = ctx.ensemble_moments_update(syn.view(-1, T * N), state, seen)
            if keep_synthetics:
                kept.append(syn.cpu().numpy())
        entry = {}
        if E:
            mean, std, mn, mx = ctx.ensemble_moments_finish(state, seen)
            entry = dict(mean=mean.cpu().numpy().reshape(T, N), std=std.cpu().numpy().reshape(T, N),
                         min=mn.cpu().numpy().reshape(T, N), max=mx.cpu().numpy().reshape(T, N))
            if density is not None:
                extent = density_extent(entry["min"], entry["max"], tmin, deltat)
                ext_d, tmin_d = _to_device(ctx, extent), _to_device(ctx, extent[:, 0])
                grid = None
                for a in range(0, E, batch):
                    syn = f.synthetics(ens[a:a + batch], wi)
                    grid = ctx.trace_density_update(syn, tmin_d, deltat, ext_d, density, linewidth, grid)
                entry["density"], entry["extent"] = grid.cpu().numpy(), extent
        if keep_synthetics:
            entry["synthetics"] = np.concatenate(kept) if kept else np.zeros((0, T, N))
        moments[wi] = entry
    return idx, var_reductions, moments


def pole_patch_basis(patch_lats, patch_lons, strikevectors_enu, earth=None):
    """(P, 3) basis of the Euler-pole slip along strike of fault patches (``euler_pole2slips``, ffi/fault.py:1436-1497):
    the strike vectors go ENU -> NEU as fault.py:1478-1480 swaps them (the third component is left at zero there), and
    then stand where a dataset's line of sight stands in ``EulerPoleCorrection.basis()``:
    ``euler_slips = |basis @ coefficients|``.  The patch centres' lats / lons [deg] are the caller's (the reference
    derives them with pyrocko's ``ne_to_latlon``); earth: ``EarthModel`` (None: the defaults)."""
    from .models.corrections import EulerPoleConfig
    sv = np.asarray(strikevectors_enu, dtype=np.float64)
    neu = np.zeros_like(sv)
    neu[:, 0] = sv[:, 1]
    neu[:, 1] = sv[:, 0]
    corr = EulerPoleConfig(dataset_names=["patches"], enabled=True).init_correction()
    corr.setup_correction(patch_lats, patch_lons, neu, np.zeros(neu.shape[0], dtype=bool), "patches", earth=earth)
    return corr.basis()


def coupling_ensemble(f, Q, basis, pole_names, earth=None, batch=512):
    """coupling maps of a batch of draws: ``backslip2coupling(point, euler_pole2slips(point, ...))``
    (ffi/fault.py:1436-1517) for every row of Q (n, nparams) against the patch basis (P, 3) of ``pole_patch_basis``.
    pole_names: the (pole_lat, pole_lon, omega) variables of ONE pole -- the reference takes the first of several too;
    each is looked up in the model's layout, else in the geodetic composite's fixed values.  earth: the EarthModel
    the basis was built with (None: the defaults).  The back-slip is the layout's ``uparr``.
    -> dict(coupling (n, P) [percent], euler_slips (n, P), mean, std (P,) of the coupling over the draws, NaN where a
    draw's ratio is 0 / 0), through ``ensemble_moments``; numpy in -> numpy out, torch-cuda in -> tensors."""
    from .models.corrections import EarthModel
    ctx = _ctx_of(f)
    lay = f.problem.layout
    fixed = getattr(getattr(f.problem, "geodetic", None), "fixed", None) or {}
    off, fix = [], []
    for name in pole_names:
        if name in lay.offsets:
            off.append(lay.offset(name, 0))
            fix.append(0.0)
        elif name in fixed:
            off.append(-1)
            fix.append(float(np.ravel(fixed[name])[0]))
        else:
            raise KeyError("pole variable %s is neither sampled nor fixed" % name)
    if len(off) != 3:
        raise ValueError("coupling_ensemble: pole_names = (pole_lat, pole_lon, omega) of one pole")
    earth = (earth if earth is not None else EarthModel()).as_tuple()
    tensor_in = _is_tensor(Q)
    Bp = _to_device(ctx, basis)
    P = int(Bp.shape[0])
    if lay.varsizes["uparr"] != P:
        raise ValueError("coupling_ensemble: %d patches in the basis, %d back-slips in the layout" % (P, lay.varsizes["uparr"]))
    n, batch = int(Q.shape[0]), max(int(batch), 1)
    es_all, cp_all, state, seen = [], [], None, 0
    for a in range(0, max(n, 1), batch):          # (an empty population still gives its (0, P) arrays)
        q = _to_device(ctx, Q[a:a + batch]).contiguous()
        es, cp = ctx.pole_coupling_batch(q, off, fix, earth, Bp, lay.offset("uparr", 0))
        state, seen = ctx.ensemble_moments_update(cp, state, seen)
        es_all.append(es)
        cp_all.append(cp)
    import torch
    out = dict(euler_slips=torch.cat(es_all), coupling=torch.cat(cp_all))
    if seen:
        out["mean"], out["std"] = ctx.ensemble_moments_finish(state, seen)[:2]
    if not tensor_in:
        out = dict((k, v.cpu().numpy()) for k, v in out.items())
    return out
