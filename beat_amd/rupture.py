"""
The arrays behind ``beat plot slip_dist`` of a distributed-slip (FFI) run, computed on the device from a stage
population -- what the reference computes with one Python sweep, one matplotlib contour call and a Python loop over
every contour segment per draw:

  beat/plotting/ffi.py:401-762    fault_slip_distribution: per subfault the rupture-front contours of ``nensemble`` draws
                                  (:599-611, ``dummy_ax.contour(xgr, ygr, sts)`` with automatic levels), the reference
                                  point's contours and hypocentre (:645-667), the mean-slip quivers and the 2-sigma
                                  ellipses of the slip vectors (:674-753)
  beat/plotting/ffi.py:338-398    fuzzy_rupture_fronts: every contour line drawn by ``draw_line_on_array(linewidth=7)`` into
                                  a grid of 25 pixels per km, truncated at half the number of draws

What is NOT here: figures, colour maps, ``clabel``, ``draw_patches`` and the 3-d GMT plot.  The contour lines come from
marching squares on the device (csrc/rupture.hip) with the decisions of contourpy's ``mpl2014`` algorithm -- a node is above
iff ``z > level``, a saddle is split by the mean of its four corners -- and agree with it in topology and, within a few
roundings, in every vertex.  DEVIATION: the order of the lines of a level, where a closed line starts and the direction of
a line are this package's own canonical ones (above on the left in (j, i) index space, an open line from its boundary edge,
a closed one from its segment with the smallest (cell, slot) key, lines by the key of their first segment), not contourpy's
trace order.  ``draw_line_on_array`` lets a later segment of a polyline overwrite an earlier one, so the density grid may
differ from the reference route in pixels where a line crosses its own earlier part; the count of lines per pixel
(``coverage``) does not depend on any order.  On given polylines ``polyline_density`` equals ``draw_line_on_array`` bit for
bit.

The functions take arrays, not stage directories; numpy in -> numpy out, torch-cuda in -> tensors.  There is no CPU
fallback: without a GPU the device functions raise.  ``auto_levels`` and ``slip_vector_geometry`` are host arithmetic.
"""
import math

import numpy as np

from . import rupture_binding as rb
from .summary import _ctx_of, _is_tensor, _to_device, ensemble_indices
from .utility import positions2idxs

LMAX = rb.LMAX
R2D, D2R = 180.0 / np.pi, np.pi / 180.0

# matplotlib.ticker.MaxNLocator's default staircase, extended as ``_staircase`` extends it
_STEPS = np.array([1, 1.5, 2, 2.5, 3, 4, 5, 6, 8, 10])
_EXTENDED_STEPS = np.concatenate([0.1 * _STEPS[:-1], _STEPS, [10 * _STEPS[1]]])


def _nonsingular(vmin, vmax, expander=1e-13, tiny=1e-14):
    """matplotlib.transforms.nonsingular as ``MaxNLocator.tick_values`` calls it"""
    if (not np.isfinite(vmin)) or (not np.isfinite(vmax)):
        return -expander, expander
    if vmax < vmin:
        vmin, vmax = vmax, vmin
    vmin, vmax = float(vmin), float(vmax)
    maxabsvalue = max(abs(vmin), abs(vmax))
    if maxabsvalue < (1e6 / tiny) * np.finfo(float).tiny:
        vmin, vmax = -expander, expander
    elif vmax - vmin <= maxabsvalue * tiny:
        if vmax == 0 and vmin == 0:
            vmin, vmax = -expander, expander
        else:
            vmin -= expander * abs(vmin)
            vmax += expander * abs(vmax)
    return vmin, vmax


def _closeto(step, offset, ms, edge):
    """matplotlib.ticker._Edge_integer.closeto"""
    if offset > 0:
        digits = np.log10(offset / step)
        tol = max(1e-10, 10 ** (digits - 12))
        tol = min(0.4999, tol)
    else:
        tol = 1e-10
    return abs(ms - edge) < tol


def auto_levels(zmin, zmax, nbins=8):
    """The contour levels matplotlib picks for ``ax.contour(x, y, z)`` without a ``levels`` argument, from the extremes of z:
    ``MaxNLocator(nbins=7 + 1, min_n_ticks=1).tick_values(zmin, zmax)`` (matplotlib/ticker.py: ``scale_range``, the default
    staircase [1, 1.5, 2, 2.5, 3, 4, 5, 6, 8, 10], ``_Edge_integer.le`` / ``ge``; ``axes.autolimit_mode`` "data") and then
    ``ContourSet._autolev``'s trim: from the last level below zmin to the first above zmax inclusive, the whole list when
    fewer than three remain.  Python / numpy floats in matplotlib's own order of operations (log10, floor division, power):
    equal to ``ax.contour(z).levels`` bit for bit on the pairs of tests/golden/rupture_fronts.npz.  -> float64 array"""
    vmin, vmax = _nonsingular(zmin, zmax)
    # scale_range
    dv = abs(vmax - vmin)
    meanv = (vmax + vmin) / 2
    if abs(meanv) / dv < 100:
        offset = 0
    else:
        offset = math.copysign(10 ** (math.log10(abs(meanv)) // 1), meanv)
    scale = 10 ** (math.log10(dv / nbins) // 1)
    # MaxNLocator._raw_ticks
    _vmin, _vmax = vmin - offset, vmax - offset
    steps = _EXTENDED_STEPS * scale
    raw_step = (_vmax - _vmin) / nbins
    large_steps = steps >= raw_step
    istep = np.nonzero(large_steps)[0][0] if any(large_steps) else len(steps) - 1
    ticks = None
    for step in steps[:istep + 1][::-1]:
        best_vmin = (_vmin // step) * step
        d, m = divmod(_vmin - best_vmin, step)                      # _Edge_integer.le
        low = d + 1 if _closeto(step, abs(offset), m / step, 1) else d
        d, m = divmod(_vmax - best_vmin, step)                      # _Edge_integer.ge
        high = d if _closeto(step, abs(offset), m / step, 0) else d + 1
        ticks = np.arange(low, high + 1) * step + best_vmin
        if ((ticks <= _vmax) & (ticks >= _vmin)).sum() >= 1:
            break
    lev = ticks + offset
    # ContourSet._autolev (line contours, extend="neither")
    zmin, zmax = float(zmin), float(zmax)
    under = np.nonzero(lev < zmin)[0]
    i0 = under[-1] if len(under) else 0
    over = np.nonzero(lev > zmax)[0]
    i1 = over[0] + 1 if len(over) else len(lev)
    if i1 - i0 < 3:
        i0, i1 = 0, len(lev)
    return np.asarray(lev[i0:i1], dtype=np.float64)


def _level_tables(levels, E, nsub, minmax=None):
    """levels (E, nsub, LMAX) and nlevels (E, nsub) from the caller's ``levels`` -- None: ``auto_levels`` of every (draw,
    subfault); one list for all draws; or one list per draw"""
    lv = np.zeros((E, nsub, LMAX))
    nl = np.zeros((E, nsub), dtype=np.int32)

    def put(e, s, vals):
        vals = np.asarray(vals, dtype=np.float64).reshape(-1)
        if vals.size > LMAX:
            raise ValueError("rupture contours: %d levels for draw %d, at most %d" % (vals.size, e, LMAX))
        if vals.size > 1 and np.min(np.diff(vals)) <= 0.0:
            raise ValueError("Contour levels must be increasing")        # matplotlib's text
        lv[e, s, :vals.size], nl[e, s] = vals, vals.size

    if levels is None:
        for e in range(E):
            for s in range(nsub):
                put(e, s, auto_levels(minmax[e, s, 0], minmax[e, s, 1]))
        return lv, nl
    per_draw = len(levels) > 0 and np.ndim(levels[0]) > 0
    if per_draw and len(levels) != E:
        raise ValueError("rupture contours: %d lists of levels for %d draws" % (len(levels), E))
    for e in range(E):
        for s in range(nsub):
            put(e, s, levels[e] if per_draw else levels)
    return lv, nl


def start_time_contours(sts, n_dip, n_strike, x, y, levels=None, ctx=None):
    """Contour lines of start times that are at hand: sts (E, npatches) in the subfault blocks of ``f.start_times`` (a
    subfault's patches row-major ``i * n_strike + j``), n_dip / n_strike per subfault, x / y the centre coordinates along
    strike (n_strike,) / dip (n_dip,) of every subfault (a list of arrays; one array for a single subfault), rectilinear
    and strictly monotone in either direction.  levels: None (matplotlib's automatic levels of every draw and subfault,
    ``auto_levels`` of its minimum and maximum, which a small kernel reduces on the device), one list for all draws, or one
    list per draw; at most 16 levels.  Returns a dict:

      vertices       (V, 2) = (x, y), and
      line_offsets   (nlines + 1,) int64 into them, on the side of sts; a closed line repeats its first vertex
      level_offsets  (E, nsub, 17) int64 into the lines: level l of (draw e, subfault s) owns the lines
                     ``level_offsets[e, s, l] ... level_offsets[e, s, l + 1]`` (numpy)
      levels, nlevels   (E, nsub, 16) float64 and (E, nsub) int32 (numpy)

    ValueError names a draw with a start time or level that is not finite.  A subfault with fewer than two rows or columns
    yields no lines (matplotlib raises there).  The largest subfault is 2304 patches (48 x 48): the start times and the
    link tables of a subfault live in LDS."""
    from .engine import get_context
    ctx = ctx if ctx is not None else get_context()
    subs = rb.subfault_table(n_dip, n_strike)
    xs, ys = rb.check_coordinates(x, y, subs)
    sts, E, _ = rb.check_start_times(sts, subs)
    nsub = int(subs.shape[0])
    minmax = rb.rupture_minmax(ctx, sts, subs)             # (raises on a non-finite start time)
    lv, nl = _level_tables(levels, E, nsub, minmax)
    vertices, line_offsets, level_offsets = rb.contour_lines(ctx, sts, subs, xs, ys, lv, nl)
    return dict(vertices=vertices, line_offsets=line_offsets, level_offsets=level_offsets, levels=lv, nlevels=nl)


def _concat_contours(parts):
    """the results of consecutive batches of draws as one"""
    if len(parts) == 1:
        return parts[0]
    voff = np.cumsum([0] + [int(p["vertices"].shape[0]) for p in parts])
    loff = np.cumsum([0] + [int(p["line_offsets"].shape[0]) - 1 for p in parts])
    if _is_tensor(parts[0]["vertices"]):
        import torch
        cat = torch.cat
    else:
        cat = np.concatenate
    lo = [p["line_offsets"][:-1] + int(voff[k]) for k, p in enumerate(parts)] + [parts[-1]["line_offsets"][-1:] + int(voff[-2])]
    return dict(vertices=cat([p["vertices"] for p in parts]), line_offsets=cat(lo),
                level_offsets=np.concatenate([p["level_offsets"] + loff[k] for k, p in enumerate(parts)]),
                levels=np.concatenate([p["levels"] for p in parts]), nlevels=np.concatenate([p["nlevels"] for p in parts]))


def rupture_contours(f, Q, x, y, levels=None, batch=512):
    """Rupture-front contours of the draws Q (n, nparams) of the compiled model ``f``: ``f.start_times`` and
    ``start_time_contours`` per batch of ``batch`` draws, joined (the result does not depend on the cut).  x, y, levels and
    the returned dict as in ``start_time_contours``; the subfaults are the model's.  Use it with ``Q = best[None]`` for the
    reference point's labelled contours (plotting/ffi.py:645-648)."""
    ctx = _ctx_of(f)
    prob = f.problem
    n, batch = int(Q.shape[0]), max(int(batch), 1)
    tensor_in = _is_tensor(Q)
    per_draw = levels is not None and len(levels) > 0 and np.ndim(levels[0]) > 0
    parts = []
    for a in range(0, max(n, 1), batch):
        q = _to_device(ctx, Q[a:a + batch]).contiguous()
        sts = f.start_times(q)
        parts.append(start_time_contours(sts, prob.n_patch_dip, prob.n_patch_strike, x, y,
                                         levels[a:a + batch] if per_draw else levels, ctx=ctx))
    out = _concat_contours(parts)
    if not tensor_in:
        out["vertices"], out["line_offsets"] = out["vertices"].cpu().numpy(), out["line_offsets"].cpu().numpy()
    return out


def allsegs(contours, draw=0, subfault=0):
    """The lines of one draw and subfault as matplotlib's ``ContourSet.allsegs``: a list over the levels of lists of
    (n, 2) numpy arrays."""
    v, lo = contours["vertices"], contours["line_offsets"]
    if _is_tensor(v):
        v, lo = v.cpu().numpy(), lo.cpu().numpy()
    lvl = contours["level_offsets"][draw, subfault]
    return [[v[lo[k]:lo[k + 1]] for k in range(int(lvl[l]), int(lvl[l + 1]))]
            for l in range(int(contours["nlevels"][draw, subfault]))]


def subfault_lines(contours, subfault):
    """the indices of every line of one subfault, draw by draw, level by level -- the order ``fuzzy_rupture_fronts`` draws in"""
    lvl = contours["level_offsets"][:, subfault]
    if lvl.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate([np.arange(int(r[0]), int(r[LMAX]), dtype=np.int64) for r in lvl] + [np.zeros(0, dtype=np.int64)])


def polyline_density(vertices, line_offsets, extent, grid_size, linewidth=7, grid=None, coverage=None, lines=None, ctx=None):
    """Density grid of polylines: every polyline ``vertices[line_offsets[k]:line_offsets[k + 1]]`` ((x, y) rows) is drawn
    into an image of its own, as ``draw_line_on_array`` (plotting/common.py:700-801) draws a line -- inside a polyline a
    later segment overwrites an earlier one --, and the images are added to ``grid`` (ny, nx) float64 in polyline order;
    ``coverage`` (ny, nx) int32 gets 1 per polyline wherever its image is positive.  extent = (xmin, xmax, ymin, ymax),
    grid_size = (ny, nx), each 2 ... 4096; linewidth in (0, 64]; grid / coverage: arrays to continue (None: zeros); lines:
    indices of the polylines to draw, in order (None: all).  On given polylines the grid equals the reference's bit for
    bit, whatever the cut into calls.  TypeError: a vertex outside the grid (``check_line_in_grid``); ValueError: a vertex
    or extent that is not finite.  -> (grid, coverage) on the side of vertices."""
    from .engine import get_context
    ctx = ctx if ctx is not None else get_context()
    return rb.polyline_density(ctx, vertices, line_offsets, extent, grid_size, linewidth, grid, coverage, lines)


def front_grid(x, y, res_km=25):
    """extent and grid shape of ``fuzzy_rupture_fronts`` (plotting/ffi.py:359-372) from the centre coordinates of a subfault:
    extent = (xmin, xmax, ymin, ymax), shape = (int((|ymax| - |ymin|) res_km), int((|xmax| - |xmin|) res_km)), restated as
    written (the absolute values included).  ValueError when a side comes out below 2 or above 4096 pixels."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    xmin, xmax, ymin, ymax = x.min(), x.max(), y.min(), y.max()
    shape = (int((np.abs(ymax) - np.abs(ymin)) * res_km), int((np.abs(xmax) - np.abs(xmin)) * res_km))
    if min(shape) < rb.GRID_MIN or max(shape) > rb.GRID_MAX:
        raise ValueError("rupture fronts: the centres x in [%g, %g], y in [%g, %g] at %g pixels per km give a grid of %d x %d "
                         "pixels; the device draws into %d ... %d a side" % (xmin, xmax, ymin, ymax, res_km, shape[0], shape[1],
                                                                           rb.GRID_MIN, rb.GRID_MAX))
    return (float(xmin), float(xmax), float(ymin), float(ymax)), shape


def hypocentre_marker(nucleation_dip, nucleation_strike, patch_size, n_dip):
    """where ``fault_slip_distribution`` puts the star (plotting/ffi.py:650-667): the centre of the patch the nucleation
    point falls into, ``(strike_idx psize + psize / 2, width - (dip_idx psize + psize / 2))`` with the indices of
    ``positions2idxs`` and width = n_dip * psize -> (x, y)"""
    psize = float(patch_size)
    dip_idx = positions2idxs(np.asarray(nucleation_dip, dtype=np.float64), psize)
    strike_idx = positions2idxs(np.asarray(nucleation_strike, dtype=np.float64), psize)
    return (float(strike_idx * psize + (psize / 2.0)), float(n_dip * psize - (dip_idx * psize + (psize / 2.0))))


def rupture_front_ensemble(f, population, best, nensemble, x, y, res_km=25, linewidth=7, batch=512):
    """``fault_slip_distribution``:599-615 with ``fuzzy_rupture_fronts`` on arrays: the rupture fronts of ``nensemble`` draws
    of ``population`` (n, nparams), picked by ``summary.ensemble_indices``, contoured at matplotlib's automatic levels and
    drawn at ``linewidth`` into a grid of ``res_km`` pixels per km, next to the contours of the point ``best`` (nparams,).
    x / y: centre coordinates per subfault as in ``start_time_contours``.  Returns ``indices`` (E,) int32 and
    ``subfaults``, a list with one dict per subfault (numpy arrays):

      extent       (xmin, xmax, ymin, ymax) of the centres, and the grid's
      shape        (ny, nx) (``front_grid``)
      density      (ny, nx): the images of every contour line of every draw added up, truncated at E / 2 (:387-389)
      coverage     (ny, nx) int32: how many lines touch a pixel; independent of any order
      best_contours   ``allsegs`` of the best point, with best_levels, and
      best_start_times  (n_dip, n_strike)
      hypocentre   (x, y) of the star (``hypocentre_marker``), None when the model samples no nucleation point"""
    import torch
    ctx = _ctx_of(f)
    prob = f.problem
    idx = ensemble_indices(int(population.shape[0]), nensemble)
    batch = max(int(batch), 1)
    if _is_tensor(population):
        ens = population[torch.as_tensor(idx.astype(np.int64), device=population.device)].contiguous()
    else:
        ens = _to_device(ctx, np.asarray(population, dtype=np.float64)[idx])
    best_h = best.cpu().numpy() if _is_tensor(best) else np.asarray(best, dtype=np.float64)
    best_d = _to_device(ctx, best_h).reshape(1, -1).contiguous()
    nd, ns = prob.n_patch_dip, prob.n_patch_strike
    nsub, E = len(nd), int(ens.shape[0])
    subs = rb.subfault_table(nd, ns)
    xs, ys = rb.check_coordinates(x, y, subs)
    grids = []
    for s in range(nsub):
        grids.append(front_grid(xs[subs[s, 3]:subs[s, 3] + ns[s]], ys[subs[s, 4]:subs[s, 4] + nd[s]], res_km) + (None, None))
    xl = [xs[subs[s, 3]:subs[s, 3] + ns[s]] for s in range(nsub)]
    yl = [ys[subs[s, 4]:subs[s, 4] + nd[s]] for s in range(nsub)]
    for a in range(0, E, batch):
        c = start_time_contours(f.start_times(ens[a:a + batch]), nd, ns, xl, yl, ctx=ctx)
        for s in range(nsub):
            extent, shape, g, cov = grids[s]
            g, cov = rb.polyline_density(ctx, c["vertices"], c["line_offsets"], extent, shape, linewidth, g, cov,
                                         subfault_lines(c, s))
            grids[s] = (extent, shape, g, cov)
    st_best = f.start_times(best_d)
    cb = start_time_contours(st_best, nd, ns, xl, yl, ctx=ctx)
    st_best = st_best.cpu().numpy()
    lay = prob.layout
    out = []
    for s in range(nsub):
        extent, shape, g, cov = grids[s]
        density = np.zeros(shape) if g is None else g.cpu().numpy()
        truncate = E / 2
        density[density > truncate] = truncate
        hypo = None
        if "nucleation_dip" in lay.offsets and "nucleation_strike" in lay.offsets:
            hypo = hypocentre_marker(best_h[lay.offset("nucleation_dip", s)], best_h[lay.offset("nucleation_strike", s)],
                                     prob.patch_sizes[s], nd[s])
        o = int(subs[s, 2])
        out.append(dict(extent=extent, shape=shape, density=density,
                        coverage=np.zeros(shape, dtype=np.int32) if cov is None else cov.cpu().numpy(),
                        best_contours=allsegs(cb, 0, s), best_levels=cb["levels"][0, s, :cb["nlevels"][0, s]].copy(),
                        best_start_times=st_best[0, o:o + nd[s] * ns[s]].reshape(nd[s], ns[s]), hypocentre=hypo))
    return dict(indices=idx, subfaults=out)


def euler_rotation_z(gamma):
    """pyrocko.moment_tensor.euler_to_matrix(0, 0, gamma) -- RESTATED FROM MEMORY, UNVERIFIED (pyrocko is not in the
    tree): with alpha = beta = 0 the matrix is the rotation about z [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]]"""
    c, s = np.cos(gamma), np.sin(gamma)
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


def slip_vector_geometry(mean, std, utens_max, reference_slip_max, rake, xgr, ygr, reference=None):
    """The host part of plotting/ffi.py:687-753 for one subfault.  mean / std: dicts of (P,) arrays for "uparr", "uperp",
    "utens" over the population (std with ddof = 0); utens_max: the largest tensile slip of the population on this
    subfault; reference_slip_max: the largest total slip of the reference point over the whole fault (``slip_bounds[1]``);
    rake [deg] of the subfault; xgr / ygr (P,): the patch centres; reference: dict of (P,) "uparr" / "uperp" of the
    reference point, or None.  Returns a dict:

      normalisation   reference_slip_max / 3 (shear) or utens_max (tensile branch)
      quivers         (P, 2) = (U, V), components of the mean slip vectors from ``arctan2(-uperp, uparr) r2d + rake``, over
                      the normalisation; None in the tensile branch ("not drawing quivers")
      ellipses        (P, 100, 2): the 2-sigma ellipses, rotated by ``euler_rotation_z(rake d2r)`` (unverified, see there)
                      and shifted to the patch centre and by the quiver
      reference_quivers  (P, 2) of the reference point with the same normalisation, None where its uparr.mean() is 0

    ValueError where neither the mean uparr nor the mean utens sums to a non-zero value (the reference fails there with
    an unbound name)."""
    upa_m, upe_m, ute_m = (np.asarray(mean[k], dtype=np.float64) for k in ("uparr", "uperp", "utens"))
    xgr, ygr = np.asarray(xgr, dtype=np.float64).ravel(), np.asarray(ygr, dtype=np.float64).ravel()

    def quivers(uperp, uparr, normalisation):
        angles = np.arctan2(-uperp, uparr) * R2D + rake
        slips = np.sqrt((uperp ** 2 + uparr ** 2)).ravel()
        slips /= normalisation
        return np.stack([np.cos(angles * D2R) * slips, np.sin(angles * D2R) * slips], axis=1)

    if upa_m.sum() != 0.0:
        normalisation = reference_slip_max / 3
        uv = quivers(upe_m, upa_m, normalisation)
        uparrstd = np.asarray(std["uparr"], dtype=np.float64) / normalisation
        uperpstd = np.asarray(std["uperp"], dtype=np.float64) / normalisation
    elif ute_m.sum() != 0:
        uperpstd = uparrstd = np.asarray(std["utens"], dtype=np.float64)
        normalisation = utens_max
        uv = None
    else:
        raise ValueError("slip vectors: the mean slip is zero in uparr and in utens")
    rot = euler_rotation_z(rake * D2R)
    circle = np.linspace(0, 2 * np.pi, 100)
    ellipses = np.empty((xgr.size, 100, 2))
    for i, (upe, upa) in enumerate(zip(uperpstd, uparrstd)):
        ellipse_x = 2 * upa * np.cos(circle)
        ellipse_y = 2 * upe * np.sin(circle)
        ellipse = np.vstack([ellipse_x, ellipse_y, np.zeros_like(ellipse_x)]).T
        rot_ellipse = ellipse.dot(rot)
        xcoords = xgr[i] + rot_ellipse[:, 0]
        ycoords = ygr[i] + rot_ellipse[:, 1]
        if uv is not None:
            xcoords += uv[i, 0]
            ycoords += uv[i, 1]
        ellipses[i, :, 0], ellipses[i, :, 1] = xcoords, ycoords
    ref_uv = None
    if reference is not None:
        r_upa, r_upe = np.asarray(reference["uparr"], dtype=np.float64), np.asarray(reference["uperp"], dtype=np.float64)
        if r_upa.mean() != 0.0:
            ref_uv = quivers(r_upe, r_upa, normalisation)
    return dict(normalisation=normalisation, quivers=uv, ellipses=ellipses, reference_quivers=ref_uv)


def slip_vector_statistics(f, population, reference, rakes, x, y, batch=512):
    """plotting/ffi.py:674-753 on arrays: per-patch mean and std (``numpy.std``, ddof = 0) of the slip variables over the
    WHOLE ``population`` (n, nparams), accumulated on the device in batches of ``batch`` rows
    (``Context.ensemble_moments_update`` / ``_finish``: only (nparams,) results leave the device), then per subfault the
    host arithmetic of ``slip_vector_geometry``.  reference (nparams,): the reference point (its total slip over the slip
    variables of the model gives the normalisation, its uparr / uperp the black quivers); rakes: the rake [deg] of every
    subfault; x / y: centre coordinates per subfault as in ``start_time_contours``.  A slip variable the model does not
    sample counts as zero.  Returns a list with one dict per subfault: ``mean`` / ``std`` (dicts of (P,) arrays) and the
    entries of ``slip_vector_geometry``."""
    ctx = _ctx_of(f)
    prob = f.problem
    lay = prob.layout
    n, batch = int(population.shape[0]), max(int(batch), 1)
    if n < 1:
        raise ValueError("slip_vector_statistics: an empty population")
    state, seen = None, 0
    for a in range(0, n, batch):
        q = _to_device(ctx, population[a:a + batch]).contiguous()
        state, seen = ctx.ensemble_moments_update(q, state, seen)
    mean, std, _, mx = (v.cpu().numpy() for v in ctx.ensemble_moments_finish(state, seen))
    ref = reference.cpu().numpy() if _is_tensor(reference) else np.asarray(reference, dtype=np.float64)
    nd, ns = prob.n_patch_dip, prob.n_patch_strike
    subs = rb.subfault_table(nd, ns)
    xs, ys = rb.check_coordinates(x, y, subs)
    P = prob.npatches
    rakes = np.broadcast_to(np.asarray(rakes, dtype=np.float64), (len(nd),))

    def column(vec, name, fill=0.0):
        if name in lay.offsets:
            o = lay.offset(name, 0)
            return vec[o:o + P]
        return np.full(P, fill)

    total = np.zeros(P)
    for comp in prob.slip_varnames:
        total += column(ref, comp) ** 2
    slip_max = np.sqrt(total).max()
    out = []
    for s in range(len(nd)):
        o, cnt = int(subs[s, 2]), nd[s] * ns[s]
        sl = slice(o, o + cnt)
        m = dict((k, column(mean, k)[sl]) for k in ("uparr", "uperp", "utens"))
        sd = dict((k, column(std, k)[sl]) for k in ("uparr", "uperp", "utens"))
        xg, yg = np.meshgrid(xs[subs[s, 3]:subs[s, 3] + ns[s]], ys[subs[s, 4]:subs[s, 4] + nd[s]])
        geo = slip_vector_geometry(m, sd, column(mx, "utens")[sl].max(), slip_max, float(rakes[s]), xg, yg,
                                   dict(uparr=column(ref, "uparr")[sl], uperp=column(ref, "uperp")[sl]))
        geo.update(mean=m, std=sd)
        out.append(geo)
    return out
