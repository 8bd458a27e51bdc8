"""TEST INFRASTRUCTURE ONLY.  The numpy restatement of csrc/noise2d.hip (k_ball_maxd2, k_ball_radius, k_ball_rms),
operation by operation in the kernels' one stated order (every numpy operation below is one IEEE operation per element: no
fused multiply-add, no pairwise summation), so the device result can be compared with ``array_equal``:

    d2(i,j) = dx*dx + dy*dy
    radius  = sqrt(max d2) * max_dist_perc;  j neighbours i iff d2(i,j) <= radius*radius
    a sum over the neighbours of i: partial l of 64 takes the neighbours j == l (mod 64), j ascending, from 0; then
    partial[l] += partial[l + h] for l < h, h = 32, 16, 8, 4, 2, 1
    mean = sum(x_j) / count;  std = sqrt(sum((x_j - mean)^2) / (count - 1));  count < 2: NaN

Adding 0.0 for a point that is no neighbour leaves a partial's bits as they are (a partial starts at +0.0 and can never
become -0.0), so the restatement adds masked terms where the kernel skips them.

Also the pieces that follow the statistic in the reference's composition (covariance.py:716-736, 814-848), on the host."""
import numpy as np

NB_TILE, NB_WAVES, LANES = 1024, 4, 64     # k_ball_rms's LDS tile, points per block, partials per point


def _lane_sum(terms):
    """terms (m, n): row-wise sum in the kernel's order -> (m,)"""
    m, n = terms.shape
    pad = (-n) % LANES
    t = np.concatenate([terms, np.zeros((m, pad))], axis=1).reshape(m, -1, LANES)
    p = np.zeros((m, LANES))
    for k in range(t.shape[1]):
        p = p + t[:, k, :]
    h = LANES // 2
    while h >= 1:
        p = p[:, :h] + p[:, h:2 * h]
        h //= 2
    return p[:, 0]


def ball_rms(coords, data, max_dist_perc, chunk=512):
    """one dataset: coords (n, 2), data (n,) -> (radius, counts (n,) int32, stds (n,))"""
    c = np.asarray(coords, dtype=np.float64)
    x = np.asarray(data, dtype=np.float64)
    n = x.size

    def d2rows(a, b):
        dx = c[a:b, 0][:, None] - c[None, :, 0]
        dy = c[a:b, 1][:, None] - c[None, :, 1]
        return dx * dx + dy * dy

    m = 0.0
    for a in range(0, n, chunk):
        m = max(m, float(d2rows(a, min(n, a + chunk)).max()))
    radius = np.sqrt(np.float64(m)) * np.float64(max_dist_perc)
    r2 = radius * radius
    counts, stds = np.zeros(n, dtype=np.int32), np.zeros(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in range(0, n, chunk):
            b = min(n, a + chunk)
            nb = d2rows(a, b) <= r2
            cnt = nb.sum(axis=1)
            mean = _lane_sum(np.where(nb, x[None, :], 0.0)) / cnt.astype(np.float64)
            e = x[None, :] - mean[:, None]
            q = _lane_sum(np.where(nb, e * e, 0.0))
            counts[a:b] = cnt
            stds[a:b] = np.where(cnt < 2, np.nan, np.sqrt(q / (cnt - 1).astype(np.float64)))
    return radius, counts, stds


def ball_rms_batch(coords, data, sizes, max_dist_perc):
    """the C entry's shape: concatenated datasets -> (radius (nd,), counts (Ntot,), stds (Ntot,))"""
    rad, cnt, std, o = [], [], [], 0
    for n in sizes:
        r, k, s = ball_rms(coords[o:o + n], data[o:o + n], max_dist_perc)
        rad.append(r)
        cnt.append(k)
        std.append(s)
        o += n
    return np.array(rad), np.concatenate(cnt), np.concatenate(std)


def autocovariance(data):
    """covariance.py:716-736, the reference's term order (ascending k, from 0)"""
    d = np.asarray(data, dtype=np.float64)
    n = d.size
    c = d - d.mean()
    out = np.zeros(n)
    for j in range(n):
        acc = 0.0
        for v in c[j:] * c[:n - j]:
            acc += v
        out[j] = acc
    return out / n


def scaled_toeplitz(coeffs, stds):
    """covariance.py:847-848: toeplitz(coeffs) * stds[:, None] * stds[None, :]"""
    n = coeffs.size
    i = np.arange(n)
    return coeffs[np.abs(i[:, None] - i[None, :])] * stds[:, None] * stds[None, :]


def non_toeplitz_covariance_2d(coords, data, max_dist_perc):
    """the host composition of the restatement: -> (C_d, stds)"""
    _, _, stds = ball_rms(coords, data, max_dist_perc)
    return scaled_toeplitz(autocovariance(data / stds), stds), stds
