"""numpy restatement of csrc/marginals.hip for the tests: the same rules written from the kernels' comments, so that the
CPU tests can pin them to numpy / scipy / the reference's fixture and the GPU tests can compare the device against them."""
import numpy as np


def sort_columns(X, cols=None):
    X = np.asarray(X, dtype=np.float64)
    cols = np.arange(X.shape[1]) if cols is None else np.asarray(cols)
    return np.sort(X[:, cols], axis=0).T.copy()


def percentiles(S, q):
    """k_col_percentiles on sorted rows S (K, n): virtual index (n - 1) * (q / 100), neighbours floor and floor + 1
    (clipped), a + (b - a) t, replaced by b - (b - a) (1 - t) where t >= 0.5"""
    S = np.asarray(S, dtype=np.float64)
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    n = S.shape[1]
    vi = np.float64(n - 1) * (q / 100.0)
    lo = np.floor(vi).astype(np.int64)
    t = vi - lo
    hi = lo + 1
    above, below = vi >= n - 1, vi < 0
    lo = np.where(above, n - 1, np.where(below, 0, lo))
    hi = np.where(above, n - 1, np.where(below, 0, hi))
    a, b = S[:, lo], S[:, hi]
    d = b - a
    return np.where(t >= 0.5, b - d * (1.0 - t), a + d * t)


def hist_counts(S, edges):
    """k_col_hist: positions of the edges in the sorted rows (left; the last edge right), counts their differences"""
    out = np.empty((S.shape[0], edges.shape[1] - 1), dtype=np.int64)
    for k in range(S.shape[0]):
        pos = np.concatenate([np.searchsorted(S[k], edges[k, :-1], "left"), np.searchsorted(S[k], edges[k, -1:], "right")])
        out[k] = np.diff(pos)
    return out


def hist2d_counts(x, y, ex, ey):
    """k_pair_hist2d: bin = searchsorted(edges, v, 'right') - 1, a value on the last edge in the last bin, outside dropped"""
    def bins(v, e):
        b = np.searchsorted(e, v, "right") - 1
        b[v == e[-1]] = e.size - 2
        b[(v < e[0]) | (v > e[-1])] = -1
        return b
    a, b = bins(x, ex), bins(y, ey)
    ok = (a >= 0) & (b >= 0)
    out = np.zeros((ex.size - 1, ey.size - 1), dtype=np.int64)
    np.add.at(out, (a[ok], b[ok]), 1)
    return out


def outer_edges(lo, hi, bins):
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return np.linspace(lo, hi, bins + 1)


def kde2d(x, y, gx, gy):
    """k_pair_moments + the host factor + k_pair_kde2d: samples and grid centred on the column means, whitened by the lower
    Cholesky factor of cov * n^(-1/3); one sum per grid point over the samples in ascending order"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.size
    mx, my = x.sum() / n, y.sum() / n
    a, b = x - mx, y - my
    f2 = np.float64(n) ** (-1.0 / 6.0) * np.float64(n) ** (-1.0 / 6.0)
    c11, c12, c22 = (a * a).sum() / (n - 1) * f2, (a * b).sum() / (n - 1) * f2, (b * b).sum() / (n - 1) * f2
    l11 = np.sqrt(c11)
    l21 = c12 / l11
    l22 = np.sqrt(c22 - l21 * l21)
    scale = 1.0 / (2.0 * np.pi * n * (l11 * l22))
    u = a / l11
    v = (b - l21 * u) / l22
    gxs, gys = np.linspace(x.min(), x.max(), gx), np.linspace(y.min(), y.max(), gy)
    gu = (gxs - mx) / l11                                            # (gx,)
    gv = ((gys - my)[None, :] - l21 * gu[:, None]) / l22             # (gx, gy)
    Z = np.zeros((gx, gy))
    for i in range(n):
        du, dv = gu[:, None] - u[i], gv - v[i]
        Z += np.exp(-(du * du + dv * dv) / 2.0)
    return Z * scale


def unit_vectors(lats, lons, transform=True):
    lats, lons = np.asarray(lats, dtype=np.float64).ravel(), np.asarray(lons, dtype=np.float64).ravel()
    if transform:
        lats, lons = 90.0 - lats, np.mod(lons, 360.0)
    t, p = np.deg2rad(lats), np.deg2rad(lons)
    return np.array([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)])


def vmf_norm(sigma):
    x = 1.0 / sigma ** 2
    return -np.log(4.0 * np.pi * sigma ** 2) - (x + np.log(1.0 - np.exp(-2.0 * x)) - np.log(2.0))


def spherical_kde(lats0, lons0, lats, lons, sigma):
    """k_sph_kde: one sum per point of exp(norm + x . x0 / sigma^2) over the samples in ascending order"""
    U0, Ug = unit_vectors(lats0, lons0), unit_vectors(lats, lons)
    norm, s2 = vmf_norm(sigma), sigma ** 2
    out = np.zeros(Ug.shape[1])
    for i in range(U0.shape[1]):
        dot = (Ug[0] * U0[0, i] + Ug[1] * U0[1, i]) + Ug[2] * U0[2, i]
        out += np.exp(norm + dot / s2)
    return out.reshape(np.shape(lats))


def vonmises_std(lons, lats):
    from scipy.optimize import brentq
    U = unit_vectors(lats, lons, transform=False)
    S = U.sum(axis=-1)
    R = S.dot(S) ** 0.5 / U.shape[-1]
    return brentq(lambda s: 1.0 / np.tanh(s) - 1.0 / s - R, 1e-8, 1e8) ** -0.5
