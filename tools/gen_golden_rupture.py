"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/rupture_fronts.npz: matplotlib's automatic contour levels, contourpy's ``mpl2014`` contour lines of
seeded start-time grids, and the density grids of the REFERENCE's own ``fuzzy_rupture_fronts`` / ``draw_line_on_array`` on
those lines.  Needs the reference tree (oracle/ref_import.py finds it; its sweep extension built in place by
``make -C oracle``), matplotlib and contourpy, so it runs where that tree is mounted; the fixture it writes is data (inputs
and expected outputs, none of the reference's text).

    python tools/gen_golden_rupture.py

Reference entry points exercised:
  beat/plotting/ffi.py:338-398      fuzzy_rupture_fronts(ax, rupture_fronts, xgrid, ygrid, linewidth=7): extent, grid shape
                                    at 25 pixels per km, the loop over draws / levels / lines, the truncation at E / 2
  beat/plotting/common.py:700-801   draw_line_on_array, once per line on one grid (the untruncated sum) and once per line on
                                    a grid of its own (the coverage count: how many lines have a positive pixel there)
  beat/plotting/ffi.py:610          ``ax.contour(xgr, ygr, sts)``: matplotlib's call, made here on the same arrays

Content:
  lev_pairs (n, 2), lev_values (n, 16), lev_counts (n,)   (zmin, zmax) -> ``ax.contour(z).levels``; half with zmin = 0
  keys                                                    the cases; per case "<key>_":
    shape (nsub, 2) = (n_dip, n_strike); sts (E, npatches); x, y: the centre coordinates of the subfaults, concatenated;
    levels (E, nsub, 16), nlevels (E, nsub): what matplotlib chose (or what the case sets)
    cp_vertices (V, 2), cp_line_offsets, cp_level_offsets (E, nsub, 17): contourpy's lines (empty ones left out)
    s<k>_extent (4,), s<k>_grid (ny, nx): fuzzy_rupture_fronts' grid of subfault k (truncated), s<k>_raw: the untruncated
    sum, s<k>_coverage (ny, nx) int32
  the case "model" also: Q (n, nparams), a population of a two-subfault model in the layout MODEL_NAMES with layout_sizes,
    all_sts (n, npatches), its start times as beat/models/seismic.py:1253-1272 forms them, idx: the draws of the
    ensemble (plotting/ffi.py:602-603), whose start times are sts; psize: the patch sizes

Every kept case is checked here: the numpy restatement tests/rupture_ref.py (marching squares in the canonical order, drawn
through density_ref) must give EXACTLY the recorded coverage.  A seeded case where a last-bit difference between a
restated and a contourpy vertex moves a pixel index is drawn again with the next seed; the count is printed (this run: 2
of the 8 seeded cases: the 2 x 2 grid on its 25 x 25 pixels, where one moved index shifts a whole diagonal line, and the
model case once).
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import ref_import  # noqa: E402

ref_import.install()
import matplotlib  # noqa: E402

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402

# beat/plotting/__init__ imports every plotting module: an empty package with the directory as its path lets the two
# modules be imported on their own
_pkg = types.ModuleType("beat.plotting")
_pkg.__path__ = [os.path.join(ref_import.REFERENCE_ROOT, "beat", "plotting")]
sys.modules["beat.plotting"] = _pkg
common = importlib.import_module("beat.plotting.common")
ffi = importlib.import_module("beat.plotting.ffi")
import fast_sweep_ext  # noqa: E402  (oracle/_ref, the reference's C built in place)
import rupture_ref as rref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
LMAX = 16
LINEWIDTH = 7


class _Axes(object):
    """stands where fuzzy_rupture_fronts expects an axes: keeps what imshow is given"""

    def imshow(self, grid, **kwargs):
        self.grid, self.extent = np.array(grid), kwargs["extent"]


def _sweep(rng, nd, ns, psize):
    """start times of a random slowness field from a random hypocentre (the reference's sweep)"""
    slow = 1.0 / rng.uniform(2.0, 4.0, nd * ns)
    hd, hs = int(rng.integers(0, nd)), int(rng.integers(0, ns))
    return np.asarray(fast_sweep_ext.fast_sweep(np.ascontiguousarray(slow), float(psize), hd, hs, nd, ns), dtype=np.float64)


def _contour(ax, xgr, ygr, z, levels):
    cs = ax.contour(xgr, ygr, z) if levels is None else ax.contour(xgr, ygr, z, levels=levels)
    segs = [[np.asarray(line, dtype=np.float64) for line in level if len(line) > 0] for level in cs.allsegs]
    return np.asarray(cs.levels, dtype=np.float64), segs


def build_case(shapes, sts, xs, ys, levels=None):
    """shapes [(nd, ns)], sts (E, npatches), xs / ys per subfault; levels: None or [e][s] lists -> the case's arrays"""
    E, nsub = sts.shape[0], len(shapes)
    off = np.concatenate([[0], np.cumsum([nd * ns for nd, ns in shapes])])
    out = dict(shape=np.array(shapes, dtype=np.int64), sts=sts, x=np.concatenate(xs), y=np.concatenate(ys))
    lv, nl = np.zeros((E, nsub, LMAX)), np.zeros((E, nsub), dtype=np.int32)
    fig, ax = plt.subplots()
    fronts = [[None] * E for _ in range(nsub)]
    for e in range(E):
        for s, (nd, ns) in enumerate(shapes):
            xgr, ygr = np.meshgrid(xs[s], ys[s])
            z = sts[e, off[s]:off[s + 1]].reshape(nd, ns)
            levs, segs = _contour(ax, xgr, ygr, z, None if levels is None else levels[e][s])
            assert len(levs) <= LMAX
            lv[e, s, :len(levs)], nl[e, s] = levs, len(levs)
            fronts[s][e] = segs
    plt.close(fig)
    verts, lo, lvl = [], [0], np.zeros((E, nsub, LMAX + 1), dtype=np.int64)
    for e in range(E):
        for s in range(nsub):
            for l in range(LMAX):
                lvl[e, s, l] = len(lo) - 1
                if l < nl[e, s]:
                    for line in fronts[s][e][l]:
                        verts.append(line)
                        lo.append(lo[-1] + len(line))
            lvl[e, s, LMAX] = len(lo) - 1
    out.update(levels=lv, nlevels=nl, cp_vertices=np.concatenate(verts) if verts else np.zeros((0, 2)),
               cp_line_offsets=np.array(lo, dtype=np.int64), cp_level_offsets=lvl)
    for s, (nd, ns) in enumerate(shapes):
        xgr, ygr = np.meshgrid(xs[s], ys[s])
        ax_ = _Axes()
        ffi.fuzzy_rupture_fronts(ax_, fronts[s], xgr, ygr, linewidth=LINEWIDTH)
        extent, shape = [float(v) for v in ax_.extent], ax_.grid.shape
        raw, cov = np.zeros(shape), np.zeros(shape, dtype=np.int32)
        for front in fronts[s]:
            for level in front:
                for line in level:
                    common.draw_line_on_array(line[:, 0], line[:, 1], grid=raw, extent=extent, grid_resolution=shape,
                                              linewidth=LINEWIDTH)
                    own = np.zeros(shape)
                    common.draw_line_on_array(line[:, 0], line[:, 1], grid=own, extent=extent, grid_resolution=shape,
                                              linewidth=LINEWIDTH)
                    cov += own > 0
        trunc = raw.copy()
        trunc[trunc > len(fronts[s]) / 2] = len(fronts[s]) / 2
        assert np.array_equal(trunc, ax_.grid)
        out["s%d_extent" % s], out["s%d_grid" % s], out["s%d_raw" % s], out["s%d_coverage" % s] = \
            np.array(extent), ax_.grid, raw, cov
    return out


def restated_coverage_equal(case):
    """the restatement on the case's start times and levels gives the recorded coverage exactly"""
    shapes = [tuple(int(v) for v in r) for r in case["shape"]]
    nd, ns = [r[0] for r in shapes], [r[1] for r in shapes]
    xo, yo = np.concatenate([[0], np.cumsum(ns)]), np.concatenate([[0], np.cumsum(nd)])
    xs = [case["x"][xo[s]:xo[s + 1]] for s in range(len(shapes))]
    ys = [case["y"][yo[s]:yo[s + 1]] for s in range(len(shapes))]
    E = case["sts"].shape[0]
    levels = [[case["levels"][e, s, :case["nlevels"][e, s]] for s in range(len(shapes))] for e in range(E)]
    v, lo, lvl = rref.contours(case["sts"], nd, ns, xs, ys, levels)
    for s in range(len(shapes)):
        lines = np.concatenate([np.arange(r[0], r[LMAX]) for r in lvl[:, s]])
        _, cov = rref.polyline_density(v, lo, case["s%d_extent" % s], case["s%d_grid" % s].shape, LINEWIDTH, lines=lines)
        if not np.array_equal(cov, case["s%d_coverage" % s]):
            return False
    return True


def _axis(n, step, reverse=False):
    a = step / 2.0 + step * np.arange(n, dtype=np.float64)
    return a[::-1].copy() if reverse else a


def sweep_case(seed, shapes, step, E, reverse_y=False):
    """seeded; drawn again with the next seed until the restatement's coverage is the recorded one -> (case, redraws)"""
    for redraw in range(20):
        rng = np.random.default_rng(seed + 1000 * redraw)
        sts = np.stack([np.concatenate([_sweep(rng, nd, ns, step) for nd, ns in shapes]) for _ in range(E)])
        case = build_case(shapes, sts, [_axis(ns, step) for _, ns in shapes], [_axis(nd, step, reverse_y) for nd, _ in shapes])
        if restated_coverage_equal(case):
            return case, redraw
    raise AssertionError("no seed of case %r gives the restatement's coverage" % (shapes,))


def constructed_cases():
    cases = {}
    # a checkerboard: at level 0.5 every interior cell is a saddle; the centre value 0.25 (a + b + c + d) is 0.5 + the mean
    # of the cell's perturbations, above in some cells and below in others (both decisions, asserted)
    rng = np.random.default_rng(77)
    nd, ns = 6, 7
    ii, jj = np.meshgrid(np.arange(nd), np.arange(ns), indexing="ij")
    z = ((ii + jj) % 2).astype(np.float64) + rng.uniform(-0.2, 0.2, (nd, ns))
    centre = 0.25 * (((z[:-1, :-1] + z[:-1, 1:]) + z[1:, 1:]) + z[1:, :-1])
    assert (centre > 0.5).any() and (centre <= 0.5).any()
    cases["checkerboard"] = build_case([(nd, ns)], z.reshape(1, -1), [_axis(ns, 0.5)], [_axis(nd, 0.5)], [[[0.5]]])
    # levels exactly equal to node values: 0 at the hypocentre's 0 (a loop of four coincident vertices that draws nothing),
    # an interior node's value and a boundary node's value
    rng = np.random.default_rng(78)
    nd, ns = 9, 8
    slow = 1.0 / rng.uniform(2.0, 4.0, nd * ns)
    t = np.asarray(fast_sweep_ext.fast_sweep(slow, 0.5, 4, 3, nd, ns), dtype=np.float64)
    assert t[4 * ns + 3] == 0.0
    lev = sorted([0.0, float(t[2 * ns + 5]), float(t[0 * ns + 6])])
    cases["node_levels"] = build_case([(nd, ns)], t.reshape(1, -1), [_axis(ns, 0.5)], [_axis(nd, 0.5)], [[lev]])
    # a plateau: a block of equal values, contoured just below, at and just above it
    nd, ns = 7, 7
    ii, jj = np.meshgrid(np.arange(nd), np.arange(ns), indexing="ij")
    z = np.minimum(np.hypot(ii - 3.0, jj - 3.0), 2.0) + 0.01 * ii
    z[2:5, 2:5] = 1.5
    cases["plateau"] = build_case([(nd, ns)], z.reshape(1, -1), [_axis(ns, 0.5)], [_axis(nd, 0.5)], [[[1.25, 1.5, 1.75]]])
    # three bumps: at 0.5 two closed lines and open lines around the bump on the boundary
    nd, ns = 12, 14
    ii, jj = np.meshgrid(np.arange(nd, dtype=np.float64), np.arange(ns, dtype=np.float64), indexing="ij")
    z = np.exp(-((ii - 3) ** 2 + (jj - 3) ** 2) / 3.0) + np.exp(-((ii - 8) ** 2 + (jj - 9) ** 2) / 4.0) \
        + np.exp(-((ii - 11) ** 2 + (jj - 2) ** 2) / 3.0) + np.exp(-((ii - 1) ** 2 + (jj - 13) ** 2) / 3.0)
    case = build_case([(nd, ns)], z.reshape(1, -1), [_axis(ns, 0.5)], [_axis(nd, 0.5)], [[[0.3, 0.5]]])
    lo, lvl = case["cp_line_offsets"], case["cp_level_offsets"][0, 0]
    v = case["cp_vertices"]
    closed = [bool(np.array_equal(v[lo[k]], v[lo[k + 1] - 1])) for k in range(lvl[1], lvl[2])]
    assert len(closed) >= 3 and any(closed) and not all(closed), closed
    cases["bumps"] = case
    for name, case in cases.items():
        assert restated_coverage_equal(case), name
    return cases


def level_pairs(n=200):
    rng = np.random.default_rng(20261021)
    pairs = np.empty((n, 2))
    vals, counts = np.zeros((n, LMAX)), np.zeros(n, dtype=np.int64)
    fig, ax = plt.subplots()
    for k in range(n):
        hi = float(10.0 ** rng.uniform(-3, 3) * rng.uniform(1, 10))
        lo = 0.0 if k % 2 == 0 else float(rng.uniform(-1, 1) * hi)
        lo, hi = min(lo, hi), max(lo, hi)
        cs = ax.contour(np.array([[lo, hi], [hi, lo]]))
        assert len(cs.levels) <= LMAX
        pairs[k] = lo, hi
        vals[k, :len(cs.levels)], counts[k] = cs.levels, len(cs.levels)
    plt.close(fig)
    return pairs, vals, counts


MODEL_SHAPES, MODEL_PSIZE = [(6, 9), (8, 5)], 0.5
MODEL_NAMES = ("uparr", "uperp", "durations", "velocities", "nucleation_strike", "nucleation_dip", "time")


def model_case(seed=20261099, n=9, nensemble=4):
    """a population of a two-subfault model and the rupture fronts of its ensemble, the start times formed as
    beat/models/seismic.py:1253-1272 forms them: positions2idxs of the nucleation point, the reference's sweep of
    1 / velocities from there, plus the subfault's time.  Kept only where the reference's C sweep (pow(x, 0.5)) and the
    sequential form the device sweep is pinned to (sqrt(x)) agree bit for bit, so that the device's start times are the
    recorded ones.  -> (case with Q (n, nparams), idx (E,), layout sizes; redraws)"""
    from beat.utility import positions2idxs
    from oracle import oracle as orc
    nsub = len(MODEL_SHAPES)
    P = sum(nd * ns for nd, ns in MODEL_SHAPES)
    sizes = [P, P, P, P, nsub, nsub, nsub]
    off = np.concatenate([[0], np.cumsum(sizes)])
    poff = np.concatenate([[0], np.cumsum([nd * ns for nd, ns in MODEL_SHAPES])])
    for redraw in range(20):
        rng = np.random.default_rng(seed + 1000 * redraw)
        Q = np.empty((n, off[-1]))
        Q[:, off[0]:off[1]] = rng.uniform(0.0, 4.0, (n, P))
        Q[:, off[1]:off[2]] = rng.uniform(-1.0, 1.0, (n, P))
        Q[:, off[2]:off[3]] = rng.uniform(1.0, 3.0, (n, P))
        Q[:, off[3]:off[4]] = rng.uniform(2.0, 4.0, (n, P))
        for s, (nd, ns) in enumerate(MODEL_SHAPES):
            Q[:, off[4] + s] = rng.uniform(0.1, ns - 0.6, n) * MODEL_PSIZE
            Q[:, off[5] + s] = rng.uniform(0.1, nd - 0.6, n) * MODEL_PSIZE
            Q[:, off[6] + s] = rng.uniform(-1.0, 1.0, n)
        sts, same = np.empty((n, P)), True
        for c in range(n):
            for s, (nd, ns) in enumerate(MODEL_SHAPES):
                hd = int(positions2idxs(Q[c, off[5] + s], cell_size=MODEL_PSIZE))
                hs = int(positions2idxs(Q[c, off[4] + s], cell_size=MODEL_PSIZE))
                slow = np.ascontiguousarray(1.0 / Q[c, off[3] + poff[s]:off[3] + poff[s + 1]])
                t = np.asarray(fast_sweep_ext.fast_sweep(slow, MODEL_PSIZE, hd, hs, nd, ns), dtype=np.float64)
                same = same and np.array_equal(t, orc.fast_sweep_exact(slow, MODEL_PSIZE, hd, hs, nd, ns))
                sts[c, poff[s]:poff[s + 1]] = t + Q[c, off[6] + s]
        idx = np.floor(np.arange(0, n, float(n) / nensemble)).astype("int32")      # plotting/ffi.py:602-603
        case = build_case(MODEL_SHAPES, sts[idx], [_axis(ns, MODEL_PSIZE) for _, ns in MODEL_SHAPES],
                          [_axis(nd, MODEL_PSIZE) for nd, _ in MODEL_SHAPES])
        if same and restated_coverage_equal(case):
            case.update(Q=Q, idx=idx, all_sts=sts, layout_sizes=np.array(sizes, dtype=np.int64),
                        psize=np.full(nsub, MODEL_PSIZE))
            return case, redraw
    raise AssertionError("no seed of the model case is kept")


def main():
    out = {}
    out["lev_pairs"], out["lev_values"], out["lev_counts"] = level_pairs()
    cases, redraws = {}, 0
    # (name, subfault shapes, patch size [km], draws): 25 pixels per km -- 33 x 17 has more than 256 cells
    for seed, (name, shapes, step, E, rev) in enumerate((("s2x2", [(2, 2)], 1.0, 2, False), ("s3x2", [(3, 2)], 1.0, 2, False),
                                                         ("s9x7", [(9, 7)], 0.5, 3, True), ("s12x11", [(12, 11)], 0.5, 2, False),
                                                         ("s20x20", [(20, 20)], 0.5, 2, False),
                                                         ("s33x17", [(33, 17)], 0.25, 2, False),
                                                         ("two", [(6, 9), (8, 5)], 0.5, 3, False))):
        cases[name], r = sweep_case(20261021 + seed, shapes, step, E, rev)
        redraws += r
    cases["model"], r = model_case()
    redraws += r
    cases.update(constructed_cases())
    for name, case in cases.items():
        for k, v in case.items():
            out["%s_%s" % (name, k)] = v
    out["keys"] = np.array(sorted(cases))
    path = os.path.join(GOLDEN, "rupture_fronts.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d seeded cases drawn again, %d bytes" % (path, len(cases), redraws, os.path.getsize(path)))


if __name__ == "__main__":
    main()
