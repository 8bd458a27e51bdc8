"""
The arrays behind the marginal-posterior plots of a finished stage, computed on the device from the population or trace
itself -- what the reference computes per variable (pair) on one core:

  beat/plotting/marginals.py:131-507    traceplot (``beat plot stage_posteriors``): ``make_bins`` (:207-215) and
  beat/plotting/common.py:248-397       ``histplot_op`` / ``hist_binning``: percentiles, bin edges, histograms
  beat/plotting/common.py:400-415       ``hist2d_plot_op`` -> ``numpy.histogram2d(density=True)``
  beat/plotting/marginals.py:510-851    ``correlation_plot`` / ``correlation_plot_hist``: ``kde2plot_op``
  beat/plotting/common.py:445-461       (a ``scipy.stats.gaussian_kde`` on a grid) once per variable pair
  beat/plotting/common.py:471-523       ``spherical_kde_op`` with ``vonmises_fisher`` / ``vonmises_std``
  beat/plotting/seismic.py:2707-2729    (beat/models/distributions.py:245-337) for ``draw_lune_kde``
  beat/utility.py:1334-1352             ``get_fit_indexes``

``X`` is a population or trace (n, V), float64, row-major: a numpy array (results are numpy) or a torch-cuda tensor (results
are tensors on its device).  ``cols`` selects K columns (None: all), ``pairs`` is (P, 2) column indices; any order, repeats
allowed.  Plotting itself, and the variable transforms (``get_transform``), stay with the caller.  There is no CPU fallback:
without a GPU the device functions raise ``BeatAmdError``.

Deviations from the reference, all stated where they apply:
  * a non-finite sample in a used column raises ``ValueError`` naming the column (numpy sorts NaN last and returns NaN);
  * the device returns integer counts; the densities are formed from them on the host with numpy's own expressions;
  * ``kde2d`` flags singular pairs one by one and raises ``numpy.linalg.LinAlgError`` after the call;
  * ``spherical_kde`` adds the samples in ascending order (the reference adds its remainder chunk first);
  * ``lune_kde`` adds no jitter to a nearly fixed variable: it raises ``ValueError`` and the caller adds it.
"""
import numpy as np

from . import marginals_binding as mb
from ._marshal import is_dev, upload
from .engine import get_context


# ------------------------------------------------------------------------------------------------ host functions
def hist_binning(mind, maxd, nbins=40):
    """the number of histogram bins of a data range (plotting/common.py:248-258): the range over its ``nbins``-th, rounded
    up -- ``nbins`` but for rounding --, 10 for an empty range"""
    mind, maxd = np.float64(mind), np.float64(maxd)
    step = np.float64((maxd - mind) / nbins)
    if step == 0:
        step = np.finfo(np.float64).eps
    bins = int(np.ceil((maxd - mind) / step))
    return bins if bins != 0 else 10


def get_fit_indexes(llk):
    """indexes of the draws whose likelihood is closest to the mean, the minimum and the maximum of ``llk``
    (utility.py:1334-1352) -> {"mean", "min", "max"}"""
    llk = np.asarray(llk)
    return dict((name, np.abs(llk - ref).argmin()) for name, ref in (("mean", llk.mean()), ("min", llk.min()),
                                                                    ("max", llk.max())))


def histogram_heights(counts, edges, cumulative=False):
    """what ``ax.hist(d, bins=edges, density=True[, cumulative=True])`` draws, from integer counts (K, nb) and edges
    (K, nb + 1): ``numpy.histogram``'s ``n / db / n.sum()``, and matplotlib's ``(tops * diff(bins)).cumsum()`` on top"""
    counts, edges = np.asarray(counts), np.asarray(edges, dtype=np.float64)
    out = np.empty(counts.shape, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(counts.shape[0]):
            db = np.array(np.diff(edges[k]), float)
            tops = counts[k] / db / counts[k].sum()
            out[k] = (tops * np.diff(edges[k])).cumsum() if cumulative else tops
    return out


def hist2d_density(counts, xedges, yedges):
    """``numpy.histogram2d(density=True)`` from integer counts (P, bx, by): histogramdd's division by the edge widths of
    each axis in turn, then by the sum"""
    counts = np.asarray(counts)
    out = np.empty(counts.shape, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in range(counts.shape[0]):
            hist = counts[p].astype(float)
            s = hist.sum()
            hist = hist / np.diff(xedges[p]).reshape(-1, 1)
            hist = hist / np.diff(yedges[p]).reshape(1, -1)
            out[p] = hist / s
    return out


def _outer_edges(lo, hi, bins):
    """numpy's edges of ``bins`` equal bins over [lo, hi] (an empty range is widened by 0.5 on both sides)"""
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    e = np.linspace(lo, hi, bins + 1)
    if np.any(e[:-1] >= e[1:]):
        raise ValueError("Too many bins for data range. Cannot create %d finite-sized bins." % bins)      # numpy's
    return e


# ------------------------------------------------------------------------------------------------ sorted columns
class SortedColumns(object):
    """the selected columns of a population, ascending, resident on the device: ``sorted`` (K, n) torch-cuda tensor;
    ``cols`` the column indices; ``host``: the population was a numpy array (results come back as numpy).
    ``percentiles``, ``make_bins`` and ``histograms`` accept it in place of ``X`` (then without ``cols``)."""

    def __init__(self, ctx, sorted_, cols, host):
        self.ctx, self.sorted, self.cols, self.host = ctx, sorted_, cols, host
        self.K, self.n = int(sorted_.shape[0]), int(sorted_.shape[1])

    def result(self, a):
        """a host array on the side the population came from"""
        return a if self.host else upload(a, self.sorted.device)


def _device_columns(X, cols):
    """-> (ctx, device tensor, the indices of ``cols`` in it, host?).  The argument rules are checked before the device
    is touched; of a host population only the used columns go up."""
    if is_dev(X):
        Xd, n, V = mb.check_population(X.contiguous())
        return get_context(X.device.index), Xd, mb.check_columns(cols, V), False
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be a (n, V) array with n, V >= 1, got %s" % (X.shape,))
    c = mb.check_columns(cols, X.shape[1])
    used, inv = np.unique(c, return_inverse=True)
    ctx = get_context()      # (raises without the library or a GPU)
    if used.size == 0:
        used = np.zeros(1, dtype=np.int64)
    return ctx, upload(X[:, used], "cuda:%d" % ctx.device, np.float64), inv.astype(np.int64).reshape(c.shape), True


def sort_columns(X, cols=None):
    """the columns ``cols`` of X, each sorted ascending on the device -> ``SortedColumns`` (K, n).  A non-finite sample
    raises ``ValueError`` naming the column (DEVIATION: numpy sorts NaN last)."""
    if isinstance(X, SortedColumns):
        if cols is not None:
            raise ValueError("a SortedColumns handle has its columns already: pass cols=None")
        return X
    c = None if cols is None else np.asarray(cols)
    ctx, Xd, idx, host = _device_columns(X, cols)
    try:
        S = mb.column_sort(ctx, Xd, idx)
    except ValueError as e:
        raise _renamed(e, idx, c, host, X)
    return SortedColumns(ctx, S, mb.check_columns(cols, int(np.shape(X)[1])), host)


def _renamed(e, idx, cols, host, X):
    """the library names a column of the array it was given; of a host population only the used columns went up"""
    import re
    m = re.search(r"column (\d+) holds", str(e))
    if not (host and m):
        return e
    used = np.unique(mb.check_columns(cols, int(np.shape(X)[1])))
    return ValueError(str(e).replace("column %s holds" % m.group(1), "column %d holds" % used[int(m.group(1))]))


def percentiles(X, q, cols=None):
    """(K, Q), ``array_equal`` to ``numpy.percentile(X[:, cols], q, axis=0).T`` (num.percentile of common.py:303, 361 and
    marginals.py:210): numpy's "linear" method restated operation for operation on the sorted columns"""
    h = sort_columns(X, cols)
    out = mb.column_percentiles(h.ctx, h.sorted, q)
    return out.cpu().numpy() if h.host else out


def _host_percentiles(h, q):
    return mb.column_percentiles(h.ctx, h.sorted, q).cpu().numpy()


def make_bins(X, nbins=40, qlist=None, cols=None):
    """(K, nbins) edges ``linspace(mind, maxd, nbins)`` per column, (mind, maxd) the first and last of the percentiles
    ``qlist`` or, for None, the minimum and maximum (``make_bins``, marginals.py:207-215).  That is nbins - 1 bins: the
    reference's quirk, kept."""
    h = sort_columns(X, cols)
    qu = _host_percentiles(h, [0.0, 100.0] if qlist is None else qlist)
    return h.result(np.array([np.linspace(qu[k, 0], qu[k, -1], int(nbins)) for k in range(h.K)]).reshape(h.K, int(nbins)))


def histograms(X, edges=None, bins=None, cols=None, cumulative=False):
    """-> (counts int64 (K, nb), edges (K, nb + 1), heights (K, nb)) of the selected columns: ``numpy.histogram`` as
    ``ax.hist(d, bins=..., density=True[, cumulative=True])`` calls it.  ``edges``: (K, nb + 1), or (nb + 1,) shared by all
    columns; ``edges=None, bins=int``: numpy's ``linspace(min, max, bins + 1)`` per column (a constant column gets
    min - 0.5, max + 0.5, as in numpy).  Bin i counts ``edges[i] <= x < edges[i + 1]``, the last bin is closed on the
    right; samples outside the edges are not counted.  The counts come from the device, exact; the heights are formed
    from them on the host (``histogram_heights``)."""
    if (edges is None) == (bins is None):
        raise ValueError("histograms: give either edges or an integer bins")
    if edges is None and (np.ndim(bins) != 0 or int(bins) < 1):
        raise ValueError("histograms: bins must be an integer >= 1, got %r" % (bins,))
    h = sort_columns(X, cols)
    if edges is None:
        mm = _host_percentiles(h, [0.0, 100.0])
        e = np.array([_outer_edges(mm[k, 0], mm[k, 1], int(bins)) for k in range(h.K)]).reshape(h.K, int(bins) + 1)
    else:
        e = np.asarray(mb._host(edges), dtype=np.float64)
        if e.ndim == 1:
            e = np.broadcast_to(e, (h.K, e.size))
        e = mb.check_edges(e, h.K)
    counts = mb.column_histograms(h.ctx, h.sorted, e)
    heights = histogram_heights(counts.cpu().numpy(), e, cumulative)
    return (counts.cpu().numpy() if h.host else counts), h.result(e), h.result(heights)


# ------------------------------------------------------------------------------------------------ pairs
def _device_pairs(X, pairs):
    """-> (ctx, device tensor, the pairs as indices into it, the pairs as given (P, 2), host?)"""
    V = int(np.shape(X)[1]) if len(np.shape(X)) == 2 else 0
    p = mb.check_pairs(pairs, max(V, 1))
    ctx, Xd, idx, host = _device_columns(X, p.ravel())
    return ctx, Xd, idx.reshape(-1, 2), p, host


def hist2d(X, pairs, bins=(None, None)):
    """-> (counts int64 (P, bx, by), xedges (P, bx + 1), yedges (P, by + 1), density (P, bx, by)):
    ``numpy.histogram2d(X[:, i], X[:, j], bins=bins, density=True)`` of every pair (i, j) (``hist2d_plot_op``,
    common.py:400-415).  A ``None`` in ``bins`` is ``hist_binning`` of the column's range; all pairs of a call must arrive
    at the same (bx, by) (``ValueError`` otherwise: call per pair).  Bin = ``searchsorted(edges, x, 'right') - 1``, a
    value on the last edge goes to the last bin.  bx * by <= 128 * 128."""
    if len(bins) != 2:
        raise ValueError("hist2d: bins must be (bx, by)")
    mb.check_hist2d_bins(*[1 if b is None else b for b in bins])
    ctx, Xd, idx, p, host = _device_pairs(X, pairs)
    P = int(p.shape[0])
    used = np.unique(idx)
    try:
        S = mb.column_sort(ctx, Xd, used)
    except ValueError as e:
        raise _renamed(e, None, p.ravel(), host, X)
    mm = mb.column_percentiles(ctx, S, [0.0, 100.0]).cpu().numpy()
    mm = dict((int(c), mm[k]) for k, c in enumerate(used))
    nb = [[hist_binning(mm[int(c)][0], mm[int(c)][1], nbins=40) if b is None else int(b) for c in idx[:, a]]
          for a, b in enumerate(bins)]
    if P and (len(set(nb[0])) > 1 or len(set(nb[1])) > 1):
        raise ValueError("hist2d: hist_binning gives the pairs different bin counts (%s x %s): call per pair"
                         % (sorted(set(nb[0])), sorted(set(nb[1]))))
    bx, by = mb.check_hist2d_bins(nb[0][0] if P else (bins[0] or 40), nb[1][0] if P else (bins[1] or 40))
    ex = np.array([_outer_edges(mm[int(c)][0], mm[int(c)][1], bx) for c in idx[:, 0]]).reshape(P, bx + 1)
    ey = np.array([_outer_edges(mm[int(c)][0], mm[int(c)][1], by) for c in idx[:, 1]]).reshape(P, by + 1)
    counts = mb.pair_hist2d(ctx, Xd, idx, ex, ey)
    dens = hist2d_density(counts.cpu().numpy(), ex, ey)
    if host:
        return counts.cpu().numpy(), ex, ey, dens
    return counts, upload(ex, Xd.device), upload(ey, Xd.device), upload(dens, Xd.device)


def kde2d(X, pairs, grid=200, skip_blocks=True, shape=None):
    """-> (Z (P, gx, gy), extents (P, 4) = (xmin, xmax, ymin, ymax), pairs (P, 2)): ``Z[p, a, b]`` is the gaussian kernel
    density estimate of the pair's two columns at ``(linspace(xmin, xmax, gx)[a], linspace(ymin, ymax, gy)[b])``
    (``kde2plot_op``, common.py:445-461, which draws ``imshow(rot90(Z), extent=extents[p])``): scipy's ``gaussian_kde`` with
    Scott's factor n^(-1/6), the full sample covariance (bias=False) and 1 / (2 pi n sqrt(det)).  ``grid``: an int or
    (gx, gy).  Every Z[p, a, b] has one accumulator and takes the samples in ascending order: it does not depend on the
    other pairs of the call; ``skip_blocks=False`` also adds the blocks of samples whose terms are exact zeros (the same
    bits).  ``shape``: None lets the launcher choose between "wide" (four grid points per lane, workgroups of 256) and
    "narrow" (one per lane, workgroups of 64, where the tiles of the wide one would not fill the device); the same bits.

    DEVIATION: a pair whose scaled covariance has no Cholesky factor (a constant column, a column paired with itself, n < 3;
    scipy raises for each such pair) is flagged; after the call a ``numpy.linalg.LinAlgError`` names those pairs, and its
    attributes ``Z``, ``extents``, ``pairs``, ``flags`` hold the results of the others (NaN in the flagged pairs)."""
    mb.check_grid(grid), mb.check_shape(shape)
    ctx, Xd, idx, p, host = _device_pairs(X, pairs)
    try:
        Z, ext, flags = mb.pair_kde2d(ctx, Xd, idx, grid, skip_blocks, shape)
    except ValueError as e:
        raise _renamed(e, None, p.ravel(), host, X)
    fl = flags.cpu().numpy()
    if host:
        Z, ext = Z.cpu().numpy(), ext.cpu().numpy()
    if fl.any():
        bad = [tuple(int(v) for v in p[k]) for k in np.nonzero(fl)[0]]
        err = np.linalg.LinAlgError("kde2d: the pairs %s have a scaled covariance without a Cholesky factor (a constant column, "
                                    "a column paired with itself or fewer than 3 samples): the data lie in a lower-dimensional "
                                    "subspace; the other pairs of the call hold their results" % (bad,))
        err.Z, err.extents, err.pairs, err.flags = Z, ext, p, fl
        raise err
    return Z, ext, p


def correlation_pairs(cols):
    """the pairs of ``correlation_plot``'s loop (marginals.py:578-587): (cols[k], cols[l]) for k < l, k outermost"""
    cols = [int(c) for c in cols]
    return np.array([(cols[k], cols[l]) for k in range(len(cols) - 1) for l in range(k + 1, len(cols))],
                    dtype=np.int64).reshape(-1, 2)


def correlation_kdes(X, cols, grid=200):
    """``kde2d`` of every pair of ``cols`` in the order of ``correlation_plot``'s loop (``correlation_pairs``)"""
    return kde2d(X, correlation_pairs(cols), grid)


# ------------------------------------------------------------------------------------------------ spherical
def vonmises_std(lons, lats, ctx=None):
    """``vonmises_std`` (distributions.py:302-337) with the unit-vector sum taken on the device in a fixed order: the
    solution kappa of 1 / tanh(kappa) - 1 / kappa = |sum x_i| / n, as sigma = kappa^-0.5.  The angles are used as they
    come: phi = deg2rad(lons), theta = deg2rad(lats)."""
    from scipy.optimize import brentq
    ctx = ctx or (get_context(lats.device.index) if is_dev(lats) else get_context())
    n = int(np.prod(tuple(lats.shape)))
    S = mb.unit_vector_sum(ctx, _flat(lats), _flat(lons), transform=False)
    R = S.dot(S) ** 0.5 / n

    def f(s):
        return 1.0 / np.tanh(s) - 1.0 / s - R

    return brentq(f, 1e-8, 1e8) ** -0.5


def _flat(a):
    return a.contiguous().reshape(-1) if is_dev(a) else np.ascontiguousarray(a, dtype=np.float64).ravel()


def vmf_norm(sigma):
    """the constant of ``vonmises_fisher`` (distributions.py:274-298) as the reference writes it"""
    x = 1.0 / sigma ** 2
    logsinh = x + np.log(1.0 - np.exp(-2.0 * x)) - np.log(2.0)
    return -np.log(4.0 * np.pi * sigma ** 2) - logsinh


def spherical_kde(lats0, lons0, lats=None, lons=None, grid_size=(200, 200), sigma=None, shape=None):
    """-> (kde, lats, lons): the sum of von Mises-Fisher kernels of width ``sigma`` centred on the samples (lats0, lons0)
    [deg] at the points (lats, lons) [deg], (grid_size) of them (``spherical_kde_op``, common.py:471-523; default grid:
    lats ``linspace(-90, 90)`` x lons ``linspace(-180, 180)``).  The reference's formula with both its quirks:
    ``sigma=None`` is 1.06 sigmahat n^-0.2 with sigmahat = ``vonmises_std`` called on (lons0, lats0) WITHOUT the 90 - lat
    transform.  The kde lives on the side of ``lats0``; the grid comes back as given (numpy for the default).  ``shape``: the
    launch shape as in ``kde2d`` (the same bits in both).

    DEVIATION: one accumulator per point, the samples added in ascending order; the reference adds its remainder chunk
    first and sums chunks of 500 pairwise -- a difference of rounding only."""
    mb.check_shape(shape)
    n = int(np.prod(tuple(lats0.shape)))
    if n < 1 or tuple(lons0.shape) != tuple(lats0.shape):
        raise ValueError("spherical_kde: lats0 and lons0 must be two arrays of one shape, at least one sample")
    grid_size = (int(grid_size[0]), int(grid_size[1]))
    if lats is None and lons is None:
        lons, lats = np.meshgrid(np.linspace(-180.0, 180, grid_size[1]), np.linspace(-90.0, 90, grid_size[0]))
    if lats is None or lons is None or int(np.prod(tuple(lats.shape))) != int(np.prod(tuple(lons.shape))) \
            or int(np.prod(tuple(lats.shape))) != grid_size[0] * grid_size[1]:
        raise ValueError("spherical_kde: lats and lons must both be given, of grid_size %s points each" % (grid_size,))
    ctx = get_context(lats0.device.index) if is_dev(lats0) else get_context()
    if sigma is None:
        sigma = 1.06 * vonmises_std(lats=lats0, lons=lons0, ctx=ctx) * n ** -0.2
    sigma = float(sigma)
    kde = mb.spherical_kde(ctx, _flat(lats0), _flat(lons0), _flat(lats), _flat(lons), vmf_norm(sigma), sigma ** 2, shape)
    return kde.reshape(grid_size), lats, lons


def lune_kde(v, w, grid_size=(200, 200), sigma=None):
    """-> (kde, lats, lons): ``spherical_kde`` of the lune coordinates (latitude delta = rad2deg(w_to_delta(w)), longitude
    gamma = rad2deg(v_to_gamma(v))) of MTQT draws on lats ``linspace(-90, 90, grid_size[0])`` x lons
    ``linspace(-30, 30, grid_size[1])`` (``draw_lune_kde``, seismic.py:2707-2729).  v, w: host arrays (n,).

    DEVIATION: the reference perturbs a variable whose spread is below 0.1 degrees with ``num.random.normal(0, 0.05)`` so
    that a width can be estimated; nothing random is added here: such a variable raises ``ValueError`` and the caller
    adds the jitter."""
    from .sources import v_to_gamma, w_to_delta
    gamma = np.rad2deg(v_to_gamma(np.asarray(mb._host(v), dtype=np.float64)))
    delta = np.rad2deg(w_to_delta(np.asarray(mb._host(w), dtype=np.float64)))
    for a, name in ((gamma, "v"), (delta, "w")):
        if a.std() < 0.1:
            raise ValueError('lune_kde: the spread of variable "%s" is %g degrees, below the 0.1 needed to estimate a spherical '
                             "kde; the reference adds normal jitter of scale 0.05 here, lune_kde adds none: add it to the "
                             "draws and call again" % (name, a.std()))
    lons, lats = np.meshgrid(np.linspace(-30.0, 30.0, int(grid_size[1])), np.linspace(-90.0, 90.0, int(grid_size[0])))
    return spherical_kde(delta, gamma, lats=lats, lons=lons, grid_size=grid_size, sigma=sigma)
