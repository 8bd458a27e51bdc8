"""numpy restatement of the contour kernels and the polyline rasteriser (beat_amd/csrc/rupture.hip), pinned to contourpy's
``mpl2014`` lines and to the reference's own ``draw_line_on_array`` by tests/test_rupture_host.py
(tests/golden/rupture_fronts.npz) and used as the expectation of tests/test_gpu_rupture.py.  TEST INFRASTRUCTURE ONLY.

What it restates:
  matplotlib's ``ax.contour(x, y, z)`` at given levels (beat/plotting/ffi.py:610, :646) by marching squares with the
  decisions of contourpy's ``mpl2014``: a node is above iff z > level, a saddle is split by
  0.25 (((za + zb) + zc) + zd) > level, a vertex on an edge with below-node p and above-node q is
  f = (zq - level) / (zq - zp), x = xp f + xq (1 - f), the same for y
  beat/plotting/ffi.py:374-385 with beat/plotting/common.py:700-801: every line drawn into an image of its own through
  density_ref.cell_indices / draw_segment, the images added in line order

The canonical order (this package's, not contourpy's): the cell (i, j) has the corners 0 = (i, j), 1 = (i, j + 1),
2 = (i + 1, j + 1), 3 = (i + 1, j), side k joins the corners k and k + 1; a segment enters through a side whose corner k
is above and corner k + 1 is not and leaves through one where it is the other way round (the above side on its left in
(j, i) index space); in a saddle the segment entering through side s leaves through s + 1 if the centre is above, else
s + 3, and the lower entry side is slot 0.  An open line starts at its boundary edge, a closed one at its segment with the
smallest key 2 cell + slot, the lines of a level are ordered by the key of their first segment; a closed line repeats
its first vertex."""
import numpy as np

import density_ref as dref

LMAX = 16
_CORNER = ((0, 0), (0, 1), (1, 1), (1, 0))


def cell_segments(z, i, j, level):
    """-> [(entry side, exit side)] of cell (i, j), slot order"""
    zc = [z[i + di, j + dj] for di, dj in _CORNER]
    above = [v > level for v in zc]
    ent = [k for k in range(4) if above[k] and not above[(k + 1) % 4]]
    ext = [k for k in range(4) if not above[k] and above[(k + 1) % 4]]
    if not ent:
        return []
    if len(ent) == 1:
        return [(ent[0], ext[0])]
    turn = 1 if 0.25 * (((zc[0] + zc[1]) + zc[2]) + zc[3]) > level else 3
    return [(e, (e + turn) % 4) for e in ent]


def edge_vertex(z, x, y, i, j, side, level):
    (di0, dj0), (di1, dj1) = _CORNER[side], _CORNER[(side + 1) % 4]
    p, q = (i + di0, j + dj0), (i + di1, j + dj1)
    if z[p] > level:
        p, q = q, p
    f = (z[q] - level) / (z[q] - z[p])
    return x[p[1]] * f + x[q[1]] * (1.0 - f), y[p[0]] * f + y[q[0]] * (1.0 - f)


def _neighbour(i, j, side):
    return i + (side == 2) - (side == 0), j + (side == 1) - (side == 3)


def edge_scale(x, y, i, j, side):
    """(max(|x_p|, |x_q|), max(|y_p|, |y_q|)) of the edge: what a vertex's rounding error scales with"""
    (di0, dj0), (di1, dj1) = _CORNER[side], _CORNER[(side + 1) % 4]
    return (max(abs(x[j + dj0]), abs(x[j + dj1])), max(abs(y[i + di0]), abs(y[i + di1])))


def level_lines(z, x, y, level, scales=None):
    """the lines of one level in canonical order: a list of (n, 2) arrays; scales: a list that gets ``edge_scale`` of
    every vertex, line by line"""
    z = np.asarray(z, dtype=np.float64)
    nd, ns = z.shape
    if nd < 2 or ns < 2:
        return []
    segs = {}                                              # key -> (i, j, entry, exit)
    for i in range(nd - 1):
        for j in range(ns - 1):
            for slot, (en, ex) in enumerate(cell_segments(z, i, j, level)):
                segs[2 * (i * (ns - 1) + j) + slot] = (i, j, en, ex)
    by_entry = dict(((i, j, en), k) for k, (i, j, en, ex) in segs.items())
    by_exit = dict(((i, j, ex), k) for k, (i, j, en, ex) in segs.items())
    succ, pred = {}, {}
    for k, (i, j, en, ex) in segs.items():
        ni, nj = _neighbour(i, j, ex)
        succ[k] = by_entry.get((ni, nj, (ex + 2) % 4), -1)
        pi, pj = _neighbour(i, j, en)
        pred[k] = by_exit.get((pi, pj, (en + 2) % 4), -1)
    lines, seen = [], set()
    for k in sorted(segs):
        if k in seen:
            continue
        cur = k                                            # walk back to the start of k's line
        while pred[cur] >= 0 and pred[cur] != k:
            cur = pred[cur]
        if pred[cur] >= 0:                                 # closed: k is the smallest key of its loop (keys ascend)
            cur = k
        start, keys = cur, []
        while True:
            keys.append(cur)
            seen.add(cur)
            cur = succ[cur]
            if cur < 0 or cur == start:
                break
        lines.append((start, keys))
    out = []
    for start, keys in sorted(lines):
        pts = [edge_vertex(z, x, y, segs[k][0], segs[k][1], segs[k][2], level) for k in keys]
        last = segs[keys[-1]]
        pts.append(edge_vertex(z, x, y, last[0], last[1], last[3], level))
        out.append(np.array(pts, dtype=np.float64).reshape(-1, 2))
        if scales is not None:
            sc = [edge_scale(x, y, segs[k][0], segs[k][1], segs[k][2]) for k in keys]
            sc.append(edge_scale(x, y, last[0], last[1], last[3]))
            scales.append(np.array(sc, dtype=np.float64).reshape(-1, 2))
    return out


def contours(sts, n_dip, n_strike, x, y, levels):
    """sts (E, npatches); x / y: lists of arrays per subfault; levels[e][s]: the levels of draw e on subfault s -> the
    arrays of ``beat_amd.rupture.start_time_contours``: vertices (V, 2), line_offsets, level_offsets (E, nsub, LMAX + 1)"""
    sts = np.asarray(sts, dtype=np.float64)
    E, nsub = sts.shape[0], len(n_dip)
    off = np.concatenate([[0], np.cumsum(np.asarray(n_dip) * np.asarray(n_strike))])
    verts, lo, lvl = [], [0], np.zeros((E, nsub, LMAX + 1), dtype=np.int64)
    nlines = 0
    for e in range(E):
        for s in range(nsub):
            z = sts[e, off[s]:off[s + 1]].reshape(n_dip[s], n_strike[s])
            for l in range(LMAX):
                lvl[e, s, l] = nlines
                if l < len(levels[e][s]):
                    for line in level_lines(z, x[s], y[s], float(levels[e][s][l])):
                        verts.append(line)
                        lo.append(lo[-1] + line.shape[0])
                        nlines += 1
            lvl[e, s, LMAX] = nlines
    vertices = np.concatenate(verts) if verts else np.zeros((0, 2))
    return vertices, np.array(lo, dtype=np.int64), lvl


def line_image(line, extent, ny, nx, linewidth):
    """the image of one polyline (ny, nx): draw_line_on_array's ``new_grid``"""
    line = np.asarray(line, dtype=np.float64).reshape(-1, 2)
    xmin, _, ymin, _ = (float(v) for v in extent)
    xstep, ystep = dref.steps(extent, ny, nx)
    img = np.zeros((ny, nx))
    if line.shape[0] == 0:
        return img
    cols = dref.cell_indices(line[:, 0], xmin, xstep, nx - 1, "x")
    rows = dref.cell_indices(line[:, 1], ymin, ystep, ny - 1, "y")
    for i in range(1, line.shape[0]):
        dref.draw_segment(img, int(rows[i - 1]), int(cols[i - 1]), int(rows[i]), int(cols[i]), float(linewidth), ny - 1, nx - 1)
    return img


def polyline_density(vertices, line_offsets, extent, grid_size, linewidth=7, grid=None, coverage=None, lines=None):
    """-> (grid, coverage): the images added in line order; coverage counts the lines whose image is positive"""
    ny, nx = grid_size
    grid = np.zeros((ny, nx)) if grid is None else np.array(grid, dtype=np.float64)
    coverage = np.zeros((ny, nx), dtype=np.int32) if coverage is None else np.array(coverage, dtype=np.int32)
    vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
    for k in (range(len(line_offsets) - 1) if lines is None else lines):
        img = line_image(vertices[line_offsets[k]:line_offsets[k + 1]], extent, ny, nx, linewidth)
        grid += img
        coverage += img > 0
    return grid, coverage


def load_cases(path):
    """tests/golden/rupture_fronts.npz -> {name: case}; a case holds the fixture's arrays of that name and n_dip, n_strike
    (lists), xs, ys (lists of the subfaults' coordinate arrays), level_lists ([e][s] arrays of the levels in use)"""
    g = np.load(path, allow_pickle=False)
    cases = {}
    for name in (str(k) for k in g["keys"]):
        pre = name + "_"
        c = dict((k[len(pre):], g[k]) for k in g.files if k.startswith(pre))
        nd, ns = [int(v) for v in c["shape"][:, 0]], [int(v) for v in c["shape"][:, 1]]
        xo, yo = np.concatenate([[0], np.cumsum(ns)]), np.concatenate([[0], np.cumsum(nd)])
        c["n_dip"], c["n_strike"] = nd, ns
        c["xs"] = [c["x"][xo[s]:xo[s + 1]] for s in range(len(nd))]
        c["ys"] = [c["y"][yo[s]:yo[s + 1]] for s in range(len(nd))]
        E = c["sts"].shape[0]
        c["level_lists"] = [[c["levels"][e, s, :c["nlevels"][e, s]] for s in range(len(nd))] for e in range(E)]
        cases[name] = c
    return cases, g


def subfault_lines(level_offsets, s):
    """the lines of subfault s, draw by draw and level by level"""
    return np.concatenate([np.arange(r[0], r[LMAX], dtype=np.int64) for r in level_offsets[:, s]])
