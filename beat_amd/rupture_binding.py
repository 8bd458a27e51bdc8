"""
The Python binding of the rupture-front entries of ``libbeat_amd.so`` (``beatamd_rupture_minmax``, ``beatamd_contour_count``,
``beatamd_contour_fill``, ``beatamd_polyline_density``; csrc/rupture.hip) as functions of a ``Context`` (``ctx``,
beat_amd.engine).  The argument rules that need no device are checked here ahead of the call (the library checks them
again); results live on the side of the first array argument.  ``beat_amd.rupture`` is the public interface on top.
"""
import numpy as np

from ._lib import check, ptr
from ._marshal import as_input, checked, is_dev, on_side

LMAX = 16                      # csrc/kernels.hpp CT_LMAX
MAX_NODES = 2304               # csrc/kernels.hpp CT_MAX_NODES
SUB_FIELDS = 5                 # csrc/kernels.hpp CT_SUB_FIELDS
GRID_MIN, GRID_MAX, LINEWIDTH_MAX = 2, 4096, 64.0


def _host(a):
    return a.cpu().numpy() if is_dev(a) else np.asarray(a)


def subfault_table(n_dip, n_strike):
    """(nsub, 5) int64 = (n_dip, n_strike, first patch, first x, first y) of subfaults that stand one after the other in
    the start times, in x (strike) and in y (dip); ValueError for a subfault beyond the LDS layout of the contour kernels"""
    nd = np.atleast_1d(np.asarray(n_dip, dtype=np.int64))
    ns = np.atleast_1d(np.asarray(n_strike, dtype=np.int64))
    if nd.ndim != 1 or nd.shape != ns.shape or nd.size < 1 or np.any(nd < 1) or np.any(ns < 1):
        raise ValueError("subfaults: n_dip %s and n_strike %s must be equally many positive counts" % (nd.tolist(), ns.tolist()))
    if np.any(nd * ns > MAX_NODES):
        k = int(np.argmax(nd * ns > MAX_NODES))
        raise ValueError("subfault %d has %d x %d = %d patches; the contour kernels keep a subfault's start times and link "
                         "tables in LDS and take at most %d (48 x 48)" % (k, nd[k], ns[k], nd[k] * ns[k], MAX_NODES))
    subs = np.zeros((nd.size, SUB_FIELDS), dtype=np.int64)
    subs[:, 0], subs[:, 1] = nd, ns
    subs[1:, 2] = np.cumsum(nd * ns)[:-1]
    subs[1:, 3] = np.cumsum(ns)[:-1]
    subs[1:, 4] = np.cumsum(nd)[:-1]
    return subs


def check_start_times(sts, subs):
    """sts as the library reads it, (E, ncells_total) with the subfaults' blocks inside -> (sts, E, ncells_total)"""
    sts = as_input(sts)
    if len(sts.shape) != 2:
        raise ValueError("start times must be (E, npatches), got %s" % (tuple(sts.shape),))
    need = int((subs[:, 2] + subs[:, 0] * subs[:, 1]).max())
    if int(sts.shape[1]) < need:
        raise ValueError("start times of %d patches, the subfaults take %d" % (int(sts.shape[1]), need))
    return sts, int(sts.shape[0]), int(sts.shape[1])


def check_coordinates(x, y, subs):
    """the centre coordinates along strike / dip of every subfault (one array each for a single subfault, else a sequence
    of arrays) -> the concatenated float64 vectors; every array finite and strictly monotone (either direction)"""
    nsub = subs.shape[0]

    def one(v, counts, what):
        if not isinstance(v, (list, tuple)) or (len(v) and np.ndim(v[0]) == 0):
            v = [v]                                     # one array: a single subfault
        if len(v) != nsub:
            raise ValueError("%s: %d coordinate arrays for %d subfaults" % (what, len(v), nsub))
        out = []
        for k, (a, n) in enumerate(zip(v, counts)):
            a = np.ascontiguousarray(_host(a), dtype=np.float64)
            if a.shape != (int(n),):
                raise ValueError("%s of subfault %d must be (%d,), got %s" % (what, k, n, a.shape))
            d = np.diff(a)
            if not np.all(np.isfinite(a)) or not (np.all(d > 0) or np.all(d < 0)):
                raise ValueError("%s of subfault %d must be finite and strictly monotone" % (what, k))
            out.append(a)
        return np.concatenate(out)

    return one(x, subs[:, 1], "x"), one(y, subs[:, 0], "y")


def check_levels(levels, nlevels, E, nsub):
    lv = np.ascontiguousarray(_host(levels), dtype=np.float64)
    nl = np.ascontiguousarray(_host(nlevels), dtype=np.int32)
    if lv.shape != (E, nsub, LMAX) or nl.shape != (E, nsub):
        raise ValueError("levels must be (%d, %d, %d) and nlevels (%d, %d), got %s and %s"
                         % (E, nsub, LMAX, E, nsub, lv.shape, nl.shape))
    if np.any(nl < 0) or np.any(nl > LMAX):
        raise ValueError("at most %d levels per draw and subfault, got %d" % (LMAX, int(nl.max())))
    used = np.arange(LMAX)[None, None, :] < nl[:, :, None]
    if not np.all(np.isfinite(lv[used])):
        e = int(np.argwhere(used & ~np.isfinite(lv))[0][0])
        raise ValueError("a contour level of draw %d is not finite" % e)
    return np.where(used, lv, 0.0), nl


def rupture_minmax(ctx, sts, subs):
    """sts (E, npatches) -> (E, nsub, 2) = (min, max) of every draw's subfaults, on the host.  ValueError names the first
    draw with a non-finite start time."""
    ctx._adopt_stream(sts)
    sts, E, ncells = check_start_times(sts, subs)
    out = np.empty((E, subs.shape[0], 2))
    check(ctx._lib.beatamd_rupture_minmax(ctx._h, E, ncells, ptr(sts), int(subs.shape[0]), ptr(subs), ptr(out)))
    bad = np.isnan(out).any(axis=(1, 2))
    if bad.any():
        raise ValueError("rupture contours: draw %d holds a start time that is not finite" % int(np.argmax(bad)))
    return out


def contour_lines(ctx, sts, subs, x, y, levels, nlevels):
    """The contour lines of E draws: sts (E, npatches), subs from ``subfault_table``, x / y from ``check_coordinates``,
    levels (E, nsub, LMAX) with nlevels (E, nsub) -> (vertices (V, 2), line_offsets (nlines + 1,) int64) on the side of sts
    and level_offsets (E, nsub, LMAX + 1) int64 on the host: the lines of level l of (e, s) are
    ``level_offsets[e, s, l] ... level_offsets[e, s, l + 1]``."""
    ctx._adopt_stream(sts)
    sts, E, ncells = check_start_times(sts, subs)
    nsub = int(subs.shape[0])
    lv, nl = check_levels(levels, nlevels, E, nsub)
    counts = np.zeros((E, nsub, LMAX, 2), dtype=np.int32)
    if E:
        check(ctx._lib.beatamd_contour_count(ctx._h, E, ncells, ptr(sts), nsub, ptr(subs), ptr(lv), ptr(nl), ptr(counts)))
    # the exclusive scans: where the lines and the vertices of every (draw, subfault, level) begin
    flat = counts.reshape(-1, 2).astype(np.int64)
    ends = np.cumsum(flat, axis=0)
    base = np.ascontiguousarray(ends - flat)
    nlines, nverts = (int(ends[-1, 0]), int(ends[-1, 1])) if E else (0, 0)
    line_base, vert_base = np.ascontiguousarray(base[:, 0]), np.ascontiguousarray(base[:, 1])
    level_offsets = np.empty((E, nsub, LMAX + 1), dtype=np.int64)
    level_offsets[:, :, :LMAX] = line_base.reshape(E, nsub, LMAX)
    level_offsets[:, :, LMAX] = ends[:, 0].reshape(E, nsub, LMAX)[:, :, LMAX - 1] if E else 0
    vertices = checked(None, sts, (nverts, 2), np.float64, "vertices", of="sts")
    line_offsets = checked(None, sts, (nlines + 1,), np.int64, "line_offsets", of="sts", zero=True)
    line_offsets[nlines:] = nverts
    if nlines:
        check(ctx._lib.beatamd_contour_fill(ctx._h, E, ncells, ptr(sts), nsub, ptr(subs), int(x.size), ptr(x), int(y.size),
                                            ptr(y), ptr(lv), ptr(nl), ptr(line_base), ptr(vert_base), nlines, nverts,
                                            ptr(vertices), ptr(line_offsets)))
    return vertices, line_offsets, level_offsets


def check_grid_size(grid_size):
    ny, nx = (int(v) for v in grid_size)
    if not (GRID_MIN <= ny <= GRID_MAX and GRID_MIN <= nx <= GRID_MAX):
        raise ValueError("polyline_density: a grid of %d x %d pixels (%d ... %d each)" % (ny, nx, GRID_MIN, GRID_MAX))
    return ny, nx


def polyline_density(ctx, vertices, line_offsets, extent, grid_size, linewidth=7, grid=None, coverage=None, lines=None):
    """grid (ny, nx) float64 += the image of every polyline, coverage (ny, nx) int32 += 1 per polyline where its image is
    positive; vertices (V, 2) = (x, y), line_offsets (nlines + 1,), extent = (xmin, xmax, ymin, ymax) on the host, lines: the
    polylines to draw, in order (None: all).  -> (grid, coverage) on the side of vertices.  TypeError for a vertex outside
    the grid, ValueError for one that is not finite."""
    ctx._adopt_stream(vertices)
    vertices = as_input(vertices)
    if len(vertices.shape) != 2 or vertices.shape[1] != 2:
        raise ValueError("polyline_density: vertices must be (V, 2), got %s" % (tuple(vertices.shape),))
    V = int(vertices.shape[0])
    if is_dev(line_offsets) == is_dev(vertices):
        lo = as_input(line_offsets, np.int64)
    else:
        lo = np.ascontiguousarray(_host(line_offsets), dtype=np.int64)
    if len(lo.shape) != 1 or lo.shape[0] < 1:
        raise ValueError("polyline_density: line_offsets must be (nlines + 1,)")
    nlines = int(lo.shape[0]) - 1
    ny, nx = check_grid_size(grid_size)
    lw = float(linewidth)
    if not (0.0 < lw <= LINEWIDTH_MAX):
        raise ValueError("polyline_density: linewidth %g outside (0, %g]" % (lw, LINEWIDTH_MAX))
    ext = np.ascontiguousarray(_host(extent), dtype=np.float64).reshape(-1)
    if ext.shape != (4,):
        raise ValueError("polyline_density: extent = (xmin, xmax, ymin, ymax)")
    sel, nsel = None, nlines
    if lines is not None:
        sel = np.ascontiguousarray(_host(lines), dtype=np.int64).reshape(-1)
        nsel = int(sel.size)
        if nsel and (sel.min() < 0 or sel.max() >= nlines):
            raise IndexError("polyline_density: polylines %d ... %d of %d" % (int(sel.min()), int(sel.max()), nlines))
    grid = checked(grid, vertices, (ny, nx), np.float64, "polyline_density: grid", of="vertices", zero=True)
    coverage = checked(coverage, vertices, (ny, nx), np.int32, "polyline_density: coverage", of="vertices", zero=True)
    check(ctx._lib.beatamd_polyline_density(ctx._h, V, ptr(vertices) if V else None, nlines, ptr(lo), nsel, ptr(sel), ptr(ext),
                                            ny, nx, lw, ptr(grid), ptr(coverage)))
    return grid, coverage
