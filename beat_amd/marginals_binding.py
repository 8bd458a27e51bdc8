"""
The Python binding of the marginals entries of ``libbeat_amd.so`` (``beatamd_column_sort``, ``beatamd_column_percentiles``,
``beatamd_column_histograms``, ``beatamd_pair_hist2d``, ``beatamd_pair_kde2d``, ``beatamd_unit_vector_sum``,
``beatamd_spherical_kde``; csrc/marginals.hip) as functions of a ``Context`` (``ctx``, beat_amd.engine).  The argument rules
that need no device are checked here ahead of the call (the library checks them again); results live on the side of the
first array argument.  ``beat_amd.marginals`` is the public interface on top.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr
from ._marshal import as_input, checked, is_dev, on_side

HIST2D_MAX_CELLS, HIST2D_MAX_SIDE = 128 * 128, 4096    # csrc/kernels.hpp MG_HIST2D_*
SORT_MAX_N = 1 << 24                                   # csrc/kernels.hpp MG_SORT_MAX_N
KDE_MAX_POINTS = 1 << 24


def _host(a):
    return a.cpu().numpy() if is_dev(a) else np.asarray(a)


def check_population(X, what="X"):
    """X as the library reads it: a contiguous float64 (n, V) array with n >= 1, V >= 1 -> (X, n, V)"""
    X = as_input(X)
    if len(X.shape) != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("%s must be a (n, V) array with n, V >= 1, got %s" % (what, tuple(X.shape)))
    return X, int(X.shape[0]), int(X.shape[1])


def check_columns(cols, V, what="cols"):
    """K column indices of a population of V columns (None: all, in order): int64 (K,), each in [0, V) (IndexError);
    any order, repeats allowed"""
    if cols is None:
        return np.arange(V, dtype=np.int64)
    c = np.asarray(_host(cols))
    if c.ndim != 1 or (c.size and not np.issubdtype(c.dtype, np.integer)):
        raise ValueError("%s must be a vector of integer column indices, got %s %s" % (what, c.dtype, c.shape))
    c = np.ascontiguousarray(c, dtype=np.int64)
    if np.any(c < 0) or np.any(c >= V):
        raise IndexError("%s %s outside a population of %d columns" % (what, c[(c < 0) | (c >= V)].tolist(), V))
    return c


def check_pairs(pairs, V):
    """(P, 2) column indices, each in [0, V) (IndexError) -> int64 (P, 2)"""
    p = np.asarray(_host(pairs))
    if p.ndim != 2 or p.shape[1] != 2 or (p.size and not np.issubdtype(p.dtype, np.integer)):
        raise ValueError("pairs must be (P, 2) integer column indices, got %s %s" % (p.dtype, p.shape))
    return check_columns(p.ravel(), V, "pairs").reshape(-1, 2)


def check_edges(edges, rows, what="edges"):
    """(rows, m + 1) bin edges, m >= 1, every row finite and non-decreasing (numpy: "bins must increase monotonically")
    -> host float64 array"""
    e = np.ascontiguousarray(_host(edges), dtype=np.float64)
    if e.ndim != 2 or e.shape[0] != rows or e.shape[1] < 2:
        raise ValueError("%s must be (%d, nbins + 1) with nbins >= 1, got %s" % (what, rows, e.shape))
    if not np.all(np.isfinite(e)):
        raise ValueError("%s must be finite" % what)
    if np.any(e[:, :-1] > e[:, 1:]):
        raise ValueError("%s must increase monotonically (row %d does not)"
                         % (what, int(np.argmax(np.any(e[:, :-1] > e[:, 1:], axis=1)))))
    return e


def check_hist2d_bins(bx, by):
    bx, by = int(bx), int(by)
    if bx < 1 or by < 1:
        raise ValueError("hist2d needs at least one bin a side, got %d x %d" % (bx, by))
    if bx * by > HIST2D_MAX_CELLS or bx > HIST2D_MAX_SIDE or by > HIST2D_MAX_SIDE:
        raise ValueError("hist2d: a grid of %d x %d bins; the device keeps at most %d cells (128 x 128) and %d bins a side"
                         % (bx, by, HIST2D_MAX_CELLS, HIST2D_MAX_SIDE))
    return bx, by


def check_grid(grid):
    """an int or (gx, gy) -> (gx, gy), both >= 1"""
    gx, gy = (grid, grid) if np.ndim(grid) == 0 else grid
    gx, gy = int(gx), int(gy)
    if gx < 1 or gy < 1 or gx * gy > KDE_MAX_POINTS:
        raise ValueError("kde2d: a grid of %d x %d points (each >= 1, at most 2^24 in all)" % (gx, gy))
    return gx, gy


SHAPES = {None: 0, "wide": 1, "narrow": 2}      # the launch shapes of the two KDE kernels (csrc/marginals.hip)


def check_shape(shape):
    if shape not in SHAPES:
        raise ValueError("unknown launch shape %r (None, 'wide' or 'narrow')" % (shape,))
    return SHAPES[shape]


def check_percents(q):
    q = np.ascontiguousarray(np.atleast_1d(np.asarray(_host(q), dtype=np.float64)))
    if q.ndim != 1:
        raise ValueError("q must be a vector of percentages, got %s" % (q.shape,))
    if not np.all((q >= 0.0) & (q <= 100.0)):     # (also catches NaN)
        raise ValueError("Percentiles must be in the range [0, 100]")
    return q


def _nonfinite(rc, bad, who):
    """ValueError naming the column for BEATAMD_ENAN, the usual mapping otherwise"""
    if rc == _lib.ENAN:
        raise ValueError("%s: column %d holds a non-finite sample (numpy would sort NaN last and return NaN; here it is an "
                         "error)" % (who, bad.value))
    check(rc)


def column_sort(ctx, X, cols=None, out=None):
    """X (n, V), cols (K,) -> (K, n): the selected columns ascending.  ValueError names a column with a non-finite sample."""
    ctx._adopt_stream(X)
    X, n, V = check_population(X)
    if n > SORT_MAX_N:
        raise ValueError("column_sort: %d samples, at most 2^24" % n)
    c = check_columns(cols, V)
    out = checked(out, X, (c.size, n), np.float64, "out", of="X")
    bad = C.c_int64(-1)
    _nonfinite(ctx._lib.beatamd_column_sort(ctx._h, n, V, ptr(X), int(c.size), ptr(c), ptr(out), C.byref(bad)), bad,
               "column_sort")
    return out


def column_percentiles(ctx, S, q, out=None):
    """S (K, n) ascending rows, q (Q,) in [0, 100] -> (K, Q), bit for bit ``numpy.percentile(S, q, axis=1).T``"""
    ctx._adopt_stream(S)
    S, K, n = check_population(S, "sorted")
    q = check_percents(q)
    out = checked(out, S, (K, q.size), np.float64, "out", of="sorted")
    check(ctx._lib.beatamd_column_percentiles(ctx._h, K, n, ptr(S), int(q.size), ptr(q), ptr(out)))
    return out


def column_histograms(ctx, S, edges, out=None):
    """S (K, n) ascending rows, edges (K, nb + 1) -> int64 counts (K, nb): ``numpy.histogram(S[k], edges[k])[0]``"""
    ctx._adopt_stream(S)
    S, K, n = check_population(S, "sorted")
    e = check_edges(edges, K)
    nb = int(e.shape[1]) - 1
    out = checked(out, S, (K, nb), np.int64, "out", of="sorted")
    check(ctx._lib.beatamd_column_histograms(ctx._h, K, n, ptr(S), nb, ptr(e), ptr(out)))
    return out


def pair_hist2d(ctx, X, pairs, xedges, yedges, out=None):
    """X (n, V), pairs (P, 2), xedges (P, bx + 1), yedges (P, by + 1) -> int64 counts (P, bx, by):
    ``numpy.histogram2d(X[:, i], X[:, j], bins=(xedges[p], yedges[p]))[0]``"""
    ctx._adopt_stream(X)
    X, n, V = check_population(X)
    p = check_pairs(pairs, V)
    P = int(p.shape[0])
    ex, ey = check_edges(xedges, P, "xedges"), check_edges(yedges, P, "yedges")
    bx, by = check_hist2d_bins(ex.shape[1] - 1, ey.shape[1] - 1)
    out = checked(out, X, (P, bx, by), np.int64, "out", of="X")
    bad = C.c_int64(-1)
    _nonfinite(ctx._lib.beatamd_pair_hist2d(ctx._h, n, V, ptr(X), P, ptr(p), bx, by, ptr(ex), ptr(ey), ptr(out),
                                            C.byref(bad)), bad, "pair_hist2d")
    return out


def pair_kde2d(ctx, X, pairs, grid=200, skip_blocks=True, shape=None):
    """X (n, V), pairs (P, 2) -> (Z (P, gx, gy), extents (P, 4) = (xmin, xmax, ymin, ymax), flags int32 (P,)) on X's side.
    Nothing is raised for flagged pairs here (their Z is NaN); ``beat_amd.marginals.kde2d`` raises."""
    ctx._adopt_stream(X)
    X, n, V = check_population(X)
    p = check_pairs(pairs, V)
    P = int(p.shape[0])
    gx, gy = check_grid(grid)
    shape = check_shape(shape)
    Z = checked(None, X, (P, gx, gy), np.float64, "Z", of="X")
    ext = checked(None, X, (P, 4), np.float64, "extents", of="X")
    flags = checked(None, X, (P,), np.int32, "flags", of="X", zero=True)
    bad = C.c_int64(-1)
    rc = ctx._lib.beatamd_pair_kde2d(ctx._h, n, V, ptr(X), P, ptr(p), gx, gy, int(bool(skip_blocks)), shape, ptr(Z), ptr(ext),
                                     ptr(flags), C.byref(bad))
    if rc != _lib.ENOTPSD:
        _nonfinite(rc, bad, "pair_kde2d")
    return Z, ext, flags


def unit_vector_sum(ctx, lats, lons, transform=False):
    """sum of the unit vectors of (lats, lons) [deg] -> host (3,); transform: 90 - lat and mod(lon, 360) first"""
    ctx._adopt_stream(lats)
    lats = as_input(lats)
    lons = on_side(lons, lats, np.float64, tuple(lats.shape), "lons")
    n = int(np.prod(tuple(lats.shape)))
    if n < 1:
        raise ValueError("unit_vector_sum: no samples")
    S = np.empty(3)
    check(ctx._lib.beatamd_unit_vector_sum(ctx._h, n, ptr(lats), ptr(lons), int(bool(transform)), ptr(S)))
    return S


def spherical_kde(ctx, lats0, lons0, lats, lons, norm, sigma2, shape=None):
    """sum_i exp(norm + (x . x0_i) / sigma2) at the points (lats, lons) over the samples (lats0, lons0), all [deg] -> an
    array of the shape of ``lats`` on the side of ``lats0``"""
    ctx._adopt_stream(lats0)
    lats0 = as_input(lats0)
    n = int(np.prod(tuple(lats0.shape)))
    if n < 1:
        raise ValueError("spherical_kde: no samples")
    lons0 = on_side(lons0, lats0, np.float64, tuple(lats0.shape), "lons0")
    dims = tuple(np.shape(_host(lats))) if not is_dev(lats) else tuple(lats.shape)
    lats = on_side(lats, lats0, np.float64, dims, "lats")
    lons = on_side(lons, lats0, np.float64, dims, "lons")
    m = int(np.prod(dims))
    if not (np.isfinite(norm) and np.isfinite(sigma2) and sigma2 > 0.0):
        raise ValueError("spherical_kde: sigma^2 = %r gives the norm %r" % (sigma2, norm))
    out = checked(None, lats0, dims, np.float64, "kde", of="lats0")
    check(ctx._lib.beatamd_spherical_kde(ctx._h, n, ptr(lats0), ptr(lons0), m, ptr(lats), ptr(lons), float(norm), float(sigma2),
                                         check_shape(shape), ptr(out)))
    return out
