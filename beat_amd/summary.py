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

from ._marshal import upload
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
    return a if _is_tensor(a) else upload(a, "cuda:%d" % ctx.device, np.float64)


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
        N = getattr(f.problem.wavemaps[wi], "nsamples", N)      # (a spectrum wavemap's synthetics are (e, T, M) spectra)
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


def derived_parameters(f, population, moment_per_slip, batch=512, coupling=None):
    """``FaultGeometry.get_derived_parameters`` (ffi/fault.py:945-954) for every row of ``population`` (n, nparams):
    (n, 1 + P_coupling) = hstack([moment magnitude, coupling]).  The magnitude is ``f.magnitudes`` over all slip
    variables of the model (get_magnitude -> get_total_slip(components=None)); moment_per_slip (npatches,): the moment of
    every patch at unit slip.  coupling: None (no pole: the magnitude alone, (n, 1)) or a dict of the arguments of
    ``coupling_ensemble`` after (f, Q): basis, pole_names and optionally earth.  numpy in -> numpy out, torch-cuda in ->
    tensor."""
    ctx = _ctx_of(f)
    tensor_in = _is_tensor(population)
    n, batch = int(population.shape[0]), max(int(batch), 1)
    import torch
    mags = []
    for a in range(0, n, batch):
        q = _to_device(ctx, population[a:a + batch]).contiguous()
        mags.append(f.magnitudes(q, moment_per_slip)[1])
    mw = torch.cat(mags) if mags else torch.zeros(0, dtype=torch.float64, device="cuda:%d" % ctx.device)
    cols = [mw.reshape(n, 1)]
    if coupling is not None:
        cp = coupling_ensemble(f, _to_device(ctx, population), batch=batch, **coupling)["coupling"]
        cols.append(cp.reshape(n, -1))
    out = torch.cat(cols, dim=1)
    return out if tensor_in else out.cpu().numpy()


def moment_rate_extent(rates, spans, kbase, deltat):
    """the extent of ``fuzzy_moment_rate`` (plotting/ffi.py:62-67) on arrays: rates (E, NT) on the index grid from
    ``kbase``, spans (E, 2) = (first index, count) of every curve's own stretch -> (min_times, max_times, min_rates,
    max_rates) over those stretches only (a curve's zeros outside its span do not count); curves with count < 1 are left
    out.  numpy arrays."""
    rates, spans = np.asarray(rates, dtype=np.float64), np.asarray(spans, dtype=np.int64)
    first, count = spans[:, 0], spans[:, 1]
    keep = count > 0
    if not keep.any():
        raise ValueError("moment_rate_extent: no curve with a sample")
    j = np.arange(rates.shape[1], dtype=np.int64)[None, :] + int(kbase)
    own = (j >= first[:, None]) & (j < (first + count)[:, None]) & keep[:, None]
    lo = np.where(own, rates, np.inf).min()
    hi = np.where(own, rates, -np.inf).max()
    return (float(first[keep].min()) * float(deltat), float((first + count - 1)[keep].max()) * float(deltat), float(lo),
            float(hi))


def truncate_density(grid, nrates):
    """``grid[grid > nrates / 2] = nrates / 2`` (plotting/ffi.py:75-77), in place; returns grid"""
    truncate = nrates / 2
    grid[grid > truncate] = truncate
    return grid


def moment_rate_ensemble(f, population, best, nensemble, moment_per_slip, deltat, individual=False, density=(500, 500),
                         linewidth=7, batch=512):
    """``draw_moment_rate`` (plotting/ffi.py:84-181) on arrays: the moment-rate functions of ``nensemble`` draws of
    ``population`` (n, nparams) picked by ``ensemble_indices``, and of the point ``best`` (nparams,).  R = 1 curve per
    draw, the total -- or with ``individual`` R = nsubfaults + 1: every subfault, then the total (the reference's
    "individual" projection draws one figure per subfault).  Returns a dict of numpy arrays:

      indices        (E,) int32
      best           dict(rates (R, NTb), times (NTb,), kbase): the best point's curves on their own grid
      times, kbase   (NT,), int: the ensemble's common grid, times = (kbase + arange(NT)) * deltat
      spans          (E, R, 2) int64: every curve's own stretch (first index, count)
      mean, std, min, max   (R, NT) over the ensemble through ``ensemble_moments`` (outside a draw's span its rate is 0)
      density        (R, ny, nx): the ``fuzzy_moment_rate`` grid -- every curve drawn over its own stretch only
                     (``trace_density_update_ranges``), then truncated at E / 2 (plotting/ffi.py:75-77); None for
                     ``density=None``
      extent         (R, 4) = (min_times, max_times, min_rates, max_rates) over the draws' own stretches (:62-67)"""
    import torch
    ctx = _ctx_of(f)
    idx = ensemble_indices(int(population.shape[0]), nensemble)
    batch = max(int(batch), 1)
    if _is_tensor(population):
        ens = population[torch.as_tensor(idx.astype(np.int64), device=population.device)].contiguous()
    else:
        ens = _to_device(ctx, np.asarray(population, dtype=np.float64)[idx])
    best_d = _to_device(ctx, best).reshape(1, -1).to(ens.device).contiguous()
    prob = f.problem
    nsub, P, E = len(prob.n_patch_dip), prob.npatches, int(ens.shape[0])
    rows = slice(0, nsub + 1) if individual else slice(nsub, nsub + 1)
    b = f.moment_rates(best_d, moment_per_slip, deltat, individual=True)
    out = dict(indices=idx, best=dict(rates=b["rates"][0, rows].cpu().numpy(), times=b["times"].cpu().numpy(),
                                      kbase=b["kbase"]))
    if E == 0:
        return out
    off = f._slip_offsets([v for v in ("uparr", "uperp") if v in prob.slip_varnames], "moment_rate_ensemble")
    k_d = _to_device(ctx, moment_per_slip)
    starts, spans = [], []
    for a in range(0, E, batch):                       # the onsets and spans of every batch: the common grid needs all
        st = f.start_times(ens[a:a + batch])
        starts.append(st)
        spans.append(ctx.ffi_moment_rate_spans_batch(f.model_id, ens[a:a + batch], nsub, P, deltat, start_times=st))
    spans = torch.cat(spans)
    kbase = int(spans[:, nsub, 0].min())
    NT = int((spans[:, nsub, 0] + spans[:, nsub, 1]).max()) - kbase
    rates = torch.empty((E, nsub + 1, NT), dtype=torch.float64, device=ens.device)
    for i, a in enumerate(range(0, E, batch)):
        ctx.ffi_moment_rates_batch(f.model_id, ens[a:a + batch], k_d, nsub, P, deltat, kbase, NT, comp_off=off,
                                   start_times=starts[i], out=rates[a:a + batch])
    Y = rates[:, rows].contiguous()
    R = int(Y.shape[1])
    state, seen = ctx.ensemble_moments_update(Y.view(E, R * NT))
    mean, std, mn, mx = (v.cpu().numpy().reshape(R, NT) for v in ctx.ensemble_moments_finish(state, seen))
    sp = spans[:, rows].contiguous()
    sp_h, Y_h = sp.cpu().numpy(), Y.cpu().numpy()
    extent = np.array([moment_rate_extent(Y_h[:, r], sp_h[:, r], kbase, deltat) for r in range(R)])
    out.update(times=(float(kbase) + np.arange(NT, dtype=np.float64)) * float(deltat), kbase=kbase, spans=sp_h, mean=mean,
               std=std, min=mn, max=mx, extent=extent, density=None)
    if density is not None:
        ranges = sp.clone()
        ranges[:, :, 0] -= kbase
        tmin = _to_device(ctx, np.full(R, float(kbase) * float(deltat)))
        grid = ctx.trace_density_update_ranges(Y, tmin, deltat, _to_device(ctx, extent), ranges.contiguous(), density,
                                               linewidth)
        out["density"] = truncate_density(grid.cpu().numpy(), E)
    return out
