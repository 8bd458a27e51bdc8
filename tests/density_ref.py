"""numpy restatement of the density grid of an ensemble of traces (k_trace_density in beat_amd/csrc/summary.hip), pinned
bit for bit to the reference's own numbers by tests/test_density_host.py (tests/golden/trace_density.npz) and used as the
expectation of tests/test_gpu_density.py.  TEST INFRASTRUCTURE ONLY.

What it restates (one trace into one grid):
  beat/plotting/common.py:700-801    draw_line_on_array: cell indices of the samples, one line per segment drawn into an
                                     image of the trace in segment order (a later segment overwrites), image added
  beat/plotting/common.py:619-697    _weighted_line: the anti-aliased line of one segment
  beat/utility.py:1556               positions2idxs: round((pos - min - cell / 2) / cell), half to even
  beat/plotting/seismic.py:282-291   fuzzy_waveforms: the default extent, amplitudes symmetric about zero

Every operation is IEEE double arithmetic in the order written here; the kernel keeps the same order."""
import math

import numpy as np

INDEX_MIN = -32768      # below: TypeError here and in the kernel (the reference's int32 products overflow from there on)


def steps(extent, ny, nx):
    xmin, xmax, ymin, ymax = (float(v) for v in extent)
    return (xmax - xmin) / (nx - 1), (ymax - ymin) / (ny - 1)


def cell_indices(pos, lo, step, nmax, axis):
    """-> int64 indices; ValueError on a non-finite one, TypeError on one above nmax or below INDEX_MIN"""
    with np.errstate(all="ignore"):
        q = np.rint((np.asarray(pos, dtype=np.float64) - lo - step / 2.0) / step)
    if not np.all(np.isfinite(q)):
        raise ValueError("trace_density: non-finite sample or extent (axis %s)" % axis)
    if q.max() > nmax or q.min() < INDEX_MIN:
        raise TypeError("Line endpoint outside of given grid Axis \"%s\"!" % axis)
    return q.astype(np.int64)


def draw_segment(img, r0, c0, r1, c1, linewidth, rmax, cmax):
    """segment (r0, c0) -> (r1, c1) into img (which is indexed [row, col]); rows < rmax and cols < cmax are written"""
    if r0 == r1 and c0 == c1:
        return
    transposed = abs(c1 - c0) < abs(r1 - r0)
    if transposed:                                  # rows and columns change roles, limits included
        r0, c0, r1, c1, rmax, cmax = c0, r0, c1, r1, cmax, rmax
    if c0 > c1:
        r0, c0, r1, c1 = r1, c1, r0, c0
    slope = float(r1 - r0) / float(c1 - c0)
    w = linewidth * math.sqrt(1.0 + abs(slope)) / 2.0
    b = float(c1 * r0 - c0 * r1) / float(c1 - c0)
    th = math.ceil(w / 2.0)
    x = np.arange(c0, c1 + 1, dtype=np.float64)[:, None]
    yv = x * slope + b
    yy = np.floor(yv) + np.arange(-th - 1, th + 2, dtype=np.float64)[None, :]
    v = np.clip(np.minimum(yy + 1.0 + w / 2.0 - yv, -yy + 1.0 + w / 2.0 + yv), 0.0, 1.0)
    xx = np.broadcast_to(x, yy.shape)
    keep = (v > 0.0) & (yy >= 0.0) & (yy < rmax) & (xx >= 0.0) & (xx < cmax)
    a, c = yy[keep].astype(np.int64), xx[keep].astype(np.int64)
    if transposed:
        img[c, a] = v[keep]
    else:
        img[a, c] = v[keep]


def trace_image(y, tmin, deltat, extent, ny, nx, linewidth):
    """the image of one trace (ny, nx)"""
    y = np.asarray(y, dtype=np.float64)
    xmin, _, ymin, _ = (float(v) for v in extent)
    xstep, ystep = steps(extent, ny, nx)
    X = float(tmin) + np.arange(y.size, dtype=np.float64) * float(deltat)
    cols = cell_indices(X, xmin, xstep, nx - 1, "x")
    rows = cell_indices(y, ymin, ystep, ny - 1, "y")
    img = np.zeros((ny, nx))
    for i in range(1, y.size):
        draw_segment(img, int(rows[i - 1]), int(cols[i - 1]), int(rows[i]), int(cols[i]), float(linewidth), ny - 1, nx - 1)
    return img


def trace_density(Y, tmin, deltat, extent, grid_size, linewidth, grid=None):
    """Y (E, T, N), tmin (T,), extent (T, 4) -> grid (T, ny, nx): the traces added in ensemble order"""
    Y = np.asarray(Y, dtype=np.float64)
    E, T, _ = Y.shape
    ny, nx = grid_size
    grid = np.zeros((T, ny, nx)) if grid is None else np.array(grid, dtype=np.float64)
    tmin = np.broadcast_to(np.asarray(tmin, dtype=np.float64), (T,))
    extent = np.asarray(extent, dtype=np.float64).reshape(T, 4)
    for t in range(T):
        for e in range(E):
            grid[t] += trace_image(Y[e, t], tmin[t], deltat, extent[t], ny, nx, linewidth)
    return grid


def density_extent(mn, mx, tmin, deltat):
    """per target [tmin, tmin + (N - 1) deltat, -a, a], a = max(|min|, |max|) over the target's envelope"""
    mn, mx = np.asarray(mn, dtype=np.float64), np.asarray(mx, dtype=np.float64)
    T, N = mn.shape
    tmin = np.broadcast_to(np.asarray(tmin, dtype=np.float64), (T,))
    a = np.maximum(np.abs(mn.min(axis=1)), np.abs(mx.max(axis=1)))
    return np.stack([tmin, tmin + float(N - 1) * float(deltat), -a, a], axis=1)
