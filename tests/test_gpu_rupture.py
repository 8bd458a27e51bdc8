"""GPU tests of the rupture-front arrays (csrc/rupture.hip, beat_amd/rupture.py): the contour kernels against the numpy
restatement tests/rupture_ref.py (which tests/test_rupture_host.py pins to contourpy's lines), the polyline rasteriser bit
for bit against the grids of the reference's own ``fuzzy_rupture_fronts`` / ``draw_line_on_array``
(tests/golden/rupture_fronts.npz), and the two ensemble functions on a small two-subfault model.  Fixtures only: no
matplotlib and no reference here.

Printed by the end-to-end test on an MI355X (a property of the trace order, not an error): the share of
pixels where the density of the device's own contours differs from the reference route's, and the largest difference --
0.0000 % of 6200 and of 4350 pixels, largest difference 0 on the "model" case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rupture_ref as rref  # noqa: E402
from test_gpu_hypers import _dev  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES, _G = rref.load_cases(os.path.join(HERE, "golden", "rupture_fronts.npz"))
NAMES = sorted(CASES)
LW = 7
LMAX = rref.LMAX
MODEL_NAMES = ("uparr", "uperp", "durations", "velocities", "nucleation_strike", "nucleation_dip", "time")   # the fixture's layout


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.fixture(scope="module")
def restated():
    """the restatement's contours of every case and their grids per subfault, computed once"""
    out = {}
    for name in NAMES:
        c = CASES[name]
        v, lo, lvl = rref.contours(c["sts"], c["n_dip"], c["n_strike"], c["xs"], c["ys"], c["level_lists"])
        grids = [rref.polyline_density(v, lo, c["s%d_extent" % s], c["s%d_grid" % s].shape, LW, lines=rref.subfault_lines(lvl, s))
                 for s in range(len(c["n_dip"]))]
        out[name] = (v, lo, lvl, grids)
    return out


def _contours(ctx, c, sts=None, levels="case"):
    from beat_amd import rupture as R
    return R.start_time_contours(c["sts"] if sts is None else sts, c["n_dip"], c["n_strike"], c["xs"], c["ys"],
                                 levels=c["level_lists_flat"] if levels == "case" else levels, ctx=ctx)


for _c in CASES.values():        # levels per draw: the same list for every subfault only where there is one subfault
    _c["level_lists_flat"] = [e[0] for e in _c["level_lists"]] if len(_c["n_dip"]) == 1 else None


# ------------------------------------------------------------------------------------------------- 1 contours
@pytest.mark.parametrize("name", NAMES)
def test_1_contours_equal_the_restatement(ctx, restated, name):
    c = CASES[name]
    v, lo, lvl, _ = restated[name]
    auto = name.startswith("s") or name in ("two", "model")       # the cases whose levels matplotlib chose
    out = _contours(ctx, c, levels=None if auto else "case")
    assert np.array_equal(out["levels"], c["levels"]) and np.array_equal(out["nlevels"], c["nlevels"])
    assert isinstance(out["vertices"], np.ndarray) and out["line_offsets"].dtype == np.int64
    assert np.array_equal(out["line_offsets"], lo) and np.array_equal(out["level_offsets"], lvl)
    assert np.array_equal(out["vertices"], v)
    # device arrays in -> tensors out, the same bits
    dev = _contours(ctx, c, sts=_dev(c["sts"], ctx), levels=None if auto else "case")
    assert dev["vertices"].is_cuda and dev["line_offsets"].is_cuda
    assert np.array_equal(dev["vertices"].cpu().numpy(), v) and np.array_equal(dev["line_offsets"].cpu().numpy(), lo)
    # the nested lists of one draw and subfault
    from beat_amd.rupture import allsegs
    e, s = c["sts"].shape[0] - 1, len(c["n_dip"]) - 1
    segs = allsegs(out, e, s)
    assert len(segs) == c["nlevels"][e, s]
    for l, lines in enumerate(segs):
        assert len(lines) == lvl[e, s, l + 1] - lvl[e, s, l]
        for k, line in zip(range(lvl[e, s, l], lvl[e, s, l + 1]), lines):
            assert np.array_equal(line, v[lo[k]:lo[k + 1]])


def test_1_closed_lines_repeat_their_first_vertex_and_small_subfaults_are_empty(ctx):
    c = CASES["bumps"]
    out = _contours(ctx, c)
    v, lo = out["vertices"], out["line_offsets"]
    closed = [bool(np.array_equal(v[lo[k]], v[lo[k + 1] - 1])) for k in range(len(lo) - 1)]
    assert any(closed) and not all(closed)
    from beat_amd import rupture as R
    for nd, ns in ((1, 5), (5, 1), (1, 1)):
        out = R.start_time_contours(np.arange(float(nd * ns))[None], nd, ns, np.arange(float(ns)), np.arange(float(nd)),
                                    levels=[1.5], ctx=ctx)
        assert out["vertices"].shape == (0, 2) and out["line_offsets"].tolist() == [0] and not out["level_offsets"].any()


def test_1_cut_into_calls_and_permuted_draws_give_the_same_bits(ctx):
    """65 draws as 1 + 64 and in another order"""
    from beat_amd import rupture as R
    c = CASES["two"]
    rng = np.random.default_rng(3)
    sts = np.concatenate([c["sts"] * f for f in 1.0 + 0.37 * rng.random(22)])[:65]
    whole = _contours(ctx, c, sts=sts, levels=None)
    parts = R._concat_contours([_contours(ctx, c, sts=sts[:1], levels=None), _contours(ctx, c, sts=sts[1:], levels=None)])
    for k in ("vertices", "line_offsets", "level_offsets", "levels", "nlevels"):
        assert np.array_equal(whole[k], parts[k]), k
    perm = rng.permutation(65)
    other = _contours(ctx, c, sts=sts[perm], levels=None)
    for new, old in enumerate(perm):
        for s in range(2):
            a, b = R.allsegs(other, new, s), R.allsegs(whole, int(old), s)
            assert len(a) == len(b)
            for la, lb in zip(a, b):
                assert len(la) == len(lb) and all(np.array_equal(p, q) for p, q in zip(la, lb))
    assert np.array_equal(other["levels"], whole["levels"][perm])


# ------------------------------------------------------------------------------------------------- 2 the rasteriser
@pytest.mark.parametrize("name", NAMES)
def test_2_recorded_contourpy_lines_give_the_reference_grid_bit_for_bit(ctx, name):
    from beat_amd import rupture as R
    c = CASES[name]
    E = c["sts"].shape[0]
    for s in range(len(c["n_dip"])):
        lines = rref.subfault_lines(c["cp_level_offsets"], s)
        shape = c["s%d_grid" % s].shape
        grid, cov = R.polyline_density(c["cp_vertices"], c["cp_line_offsets"], c["s%d_extent" % s], shape, LW, lines=lines,
                                       ctx=ctx)
        assert grid.dtype == np.float64 and cov.dtype == np.int32
        assert np.array_equal(grid, c["s%d_raw" % s]) and np.array_equal(cov, c["s%d_coverage" % s])
        grid[grid > E / 2] = E / 2
        assert np.array_equal(grid, c["s%d_grid" % s])
    # device arrays, all lines of a one-subfault case at once
    if len(c["n_dip"]) == 1:
        g, cv = R.polyline_density(_dev(c["cp_vertices"], ctx), _dev(c["cp_line_offsets"], ctx), c["s0_extent"],
                                   c["s0_grid"].shape, LW, ctx=ctx)
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), c["s0_raw"]) and np.array_equal(cv.cpu().numpy(), c["s0_coverage"])


@pytest.mark.parametrize("name", NAMES)
def test_2_restated_lines_give_the_restated_grid(ctx, restated, name):
    from beat_amd import rupture as R
    c = CASES[name]
    v, lo, lvl, grids = restated[name]
    for s in range(len(c["n_dip"])):
        grid, cov = R.polyline_density(v, lo, c["s%d_extent" % s], c["s%d_grid" % s].shape, LW,
                                       lines=rref.subfault_lines(lvl, s), ctx=ctx)
        assert np.array_equal(grid, grids[s][0]) and np.array_equal(cov, grids[s][1])
        assert np.array_equal(cov, c["s%d_coverage" % s])


@pytest.mark.parametrize("strip,rows", [("1", "3"), ("7", "64"), ("31", "5"), ("4096", "4096")])
def test_2_grid_is_independent_of_the_tile_and_of_the_cut_into_calls(ctx, monkeypatch, strip, rows):
    """BEATAMD_PD_STRIP / BEATAMD_PD_ROWS (a context of the test suite re-reads them at every call)"""
    from beat_amd import rupture as R
    c = CASES["s12x11"]
    shape, ext = c["s0_grid"].shape, c["s0_extent"]
    monkeypatch.setenv("BEATAMD_PD_STRIP", strip)
    monkeypatch.setenv("BEATAMD_PD_ROWS", rows)
    grid, cov = R.polyline_density(c["cp_vertices"], c["cp_line_offsets"], ext, shape, LW, ctx=ctx)
    assert np.array_equal(grid, c["s0_raw"]) and np.array_equal(cov, c["s0_coverage"])
    n = len(c["cp_line_offsets"]) - 1
    g, cv = None, None
    for lines in (np.arange(0, 1), np.arange(1, n // 2), np.arange(n // 2, n)):
        g, cv = R.polyline_density(c["cp_vertices"], c["cp_line_offsets"], ext, shape, LW, g, cv, lines=lines, ctx=ctx)
    assert np.array_equal(g, c["s0_raw"]) and np.array_equal(cv, c["s0_coverage"])


def _random_polylines(rng, extent, nlines, nvert):
    xmin, xmax, ymin, ymax = extent
    verts, lo = [], [0]
    for k in range(nlines):
        n = int(rng.integers(2, nvert + 1))
        verts.append(np.stack([rng.uniform(xmin, xmax, n), rng.uniform(ymin, ymax, n)], axis=1))
        lo.append(lo[-1] + n)
    return verts, lo


@pytest.mark.parametrize("shape", [(2, 2), (3, 500), (500, 3), (475, 475)])
def test_2_grid_shapes_last_row_and_column_and_empty_polylines(ctx, shape):
    """more than 256 segments in a line (two chunks), lines along the last row and the last column (never written), a
    polyline of one vertex and one of none, a segment whose two ends share a pixel"""
    from beat_amd import rupture as R
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    ext = (-2.0, 7.5, 10.0, 11.25)
    verts, lo = _random_polylines(rng, ext, 5, 12)
    long_line = np.stack([rng.uniform(ext[0], ext[1], 300), rng.uniform(ext[2], ext[3], 300)], axis=1)
    extra = [long_line,
             np.array([[ext[0], ext[3]], [ext[1], ext[3]]]),                   # along the last row
             np.array([[ext[1], ext[2]], [ext[1], ext[3]]]),                   # along the last column
             np.array([[1.0, 10.5]]), np.zeros((0, 2)),                        # one vertex, no vertex
             np.array([[1.0, 10.5], [1.0, 10.5], [3.0, 10.75]]),               # a zero-length segment first
             np.array([[ext[0], ext[2]], [ext[1], ext[3]]])]                   # corner to corner
    for line in extra:
        verts.append(line)
        lo.append(lo[-1] + len(line))
    v, lo = np.concatenate(verts), np.array(lo, dtype=np.int64)
    want, want_cov = rref.polyline_density(v, lo, ext, shape, LW)
    grid, cov = R.polyline_density(v, lo, ext, shape, LW, ctx=ctx)
    assert np.array_equal(grid, want) and np.array_equal(cov, want_cov)
    assert not grid[-1].any() and not grid[:, -1].any()
    if min(shape) > 3:
        assert grid.any() and cov.max() >= 2
    # another width, continuing a grid
    want2, cov2 = rref.polyline_density(v, lo, ext, shape, 2.5, grid=want, coverage=want_cov)
    grid2, cv2 = R.polyline_density(v, lo, ext, shape, 2.5, grid=grid, coverage=cov, ctx=ctx)
    assert np.array_equal(grid2, want2) and np.array_equal(cv2, cov2)


def test_2_errors(ctx):
    from beat_amd import rupture as R
    c = CASES["s9x7"]
    v, lo, ext, shape = c["cp_vertices"], c["cp_line_offsets"], c["s0_extent"], c["s0_grid"].shape
    # a NaN start time names the draw; a NaN level too
    sts = c["sts"].copy()
    sts[1, 17] = np.nan
    with pytest.raises(ValueError, match="draw 1"):
        _contours(ctx, c, sts=sts, levels=None)
    with pytest.raises(ValueError, match="draw 1"):
        _contours(ctx, c, sts=_dev(sts, ctx), levels=None)
    with pytest.raises(ValueError, match="draw 2"):
        _contours(ctx, c, levels=[[0.5], [0.5], [np.inf]])
    with pytest.raises(ValueError, match="2304"):
        R.start_time_contours(np.zeros((1, 49 * 48)), 49, 48, np.arange(48.0), np.arange(49.0), ctx=ctx)
    # a vertex outside the grid is the reference's TypeError, one that is not finite a ValueError
    out = v.copy()
    out[5, 0] = ext[1] + 0.2 * (ext[1] - ext[0])
    with pytest.raises(TypeError, match="outside"):
        R.polyline_density(out, lo, ext, shape, LW, ctx=ctx)
    with pytest.raises(TypeError, match="outside"):
        R.polyline_density(_dev(out, ctx), lo, ext, shape, LW, ctx=ctx)
    nan = v.copy()
    nan[7, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        R.polyline_density(nan, lo, ext, shape, LW, ctx=ctx)
    # the limits of beatamd_trace_density_update, and offsets / selections outside their arrays
    for bad_shape in ((1, 50), (50, 4097)):
        with pytest.raises(ValueError, match="2 ... 4096"):
            R.polyline_density(v, lo, ext, bad_shape, LW, ctx=ctx)
    for lw in (0.0, 64.5):
        with pytest.raises(ValueError, match="linewidth"):
            R.polyline_density(v, lo, ext, shape, lw, ctx=ctx)
    with pytest.raises(IndexError):
        R.polyline_density(v, lo, ext, shape, LW, lines=[len(lo) - 1], ctx=ctx)
    bad_lo = lo.copy()
    bad_lo[-1] = len(v) + 1
    with pytest.raises(IndexError):
        R.polyline_density(v, bad_lo, ext, shape, LW, ctx=ctx)
    # and the calls still work afterwards (the status word is cleared)
    grid, _ = R.polyline_density(v, lo, ext, shape, LW, lines=rref.subfault_lines(c["cp_level_offsets"], 0), ctx=ctx)
    assert np.array_equal(grid, c["s0_raw"])


# ------------------------------------------------------------------------------------------------- 3 end to end
@pytest.fixture(scope="module")
def model(ctx):
    """the compiled synthetic problem with the fault and the layout of the fixture's "model" case: the start times need the
    velocities, the nucleation points and the times only, the library behind the one wavemap is never read"""
    from beat_amd.synthetic import SyntheticSpec, build_problem
    c = CASES["model"]
    spec = SyntheticSpec(c["n_dip"], c["n_strike"], [float(v) for v in c["psize"]], T=1, N=8, D=5, S=16, st_min=-1.0, st_dt=0.5,
                         du_min=1.0, du_dt=0.5, slip_varnames=("uparr", "uperp"), vel_bounds=(2.0, 4.0), time_bounds=(-1.0, 1.0))
    prob, host = build_problem(spec)
    sizes = host["layout"].varsizes
    assert list(sizes)[:len(MODEL_NAMES)] == list(MODEL_NAMES)
    assert [sizes[k] for k in MODEL_NAMES] == [int(v) for v in c["layout_sizes"]]
    f = prob.compile(ctx)
    yield f
    f.release()


def _population(f, Q):
    """the fixture's rows in the model's layout: the variables behind the fixture's (the noise scale) are zero"""
    return np.hstack([Q, np.zeros((Q.shape[0], f.problem.layout.size - Q.shape[1]))])


def test_3_rupture_front_ensemble_end_to_end(ctx, model, restated):
    from beat_amd import rupture as R
    c = CASES["model"]
    Q, idx = _population(model, c["Q"]), c["idx"]
    # the device's sweep gives the recorded start times (it is pinned bit for bit to the sequential reference)
    assert np.array_equal(model.start_times(_dev(Q, ctx)).cpu().numpy(), c["all_sts"])
    out = R.rupture_front_ensemble(model, Q, Q[1], len(idx), c["xs"], c["ys"], batch=3)
    assert np.array_equal(out["indices"], idx)
    E = len(idx)
    best = R.rupture_contours(model, Q[1:2], c["xs"], c["ys"])
    off = np.concatenate([[0], np.cumsum(np.array(c["n_dip"]) * np.array(c["n_strike"]))])
    for s, sub in enumerate(out["subfaults"]):
        ref_grid = c["s%d_grid" % s]
        assert sub["shape"] == ref_grid.shape and np.array_equal(sub["extent"], c["s%d_extent" % s])
        assert np.array_equal(sub["coverage"], c["s%d_coverage" % s])              # exact: independent of any order
        want = restated["model"][3][s][0].copy()
        want[want > E / 2] = E / 2
        assert np.array_equal(sub["density"], want)
        diff = sub["density"] != ref_grid
        print("model subfault %d: density differs from the reference route in %.4f %% of %d pixels, largest |difference| %.3f"
              % (s, 100.0 * diff.mean(), diff.size, np.abs(sub["density"] - ref_grid).max()))
        assert np.array_equal(sub["best_start_times"].ravel(), c["all_sts"][1, off[s]:off[s + 1]])
        z = sub["best_start_times"]
        assert np.array_equal(sub["best_levels"], R.auto_levels(z.min(), z.max()))
        for l, lev in enumerate(sub["best_levels"]):
            want_lines = rref.level_lines(z, c["xs"][s], c["ys"][s], float(lev))
            assert len(want_lines) == len(sub["best_contours"][l])
            assert all(np.array_equal(a, b) for a, b in zip(want_lines, sub["best_contours"][l]))
        assert len(R.allsegs(best, 0, s)) == len(sub["best_contours"])
        lay = model.problem.layout
        assert sub["hypocentre"] == R.hypocentre_marker(Q[1, lay.offset("nucleation_dip", s)],
                                                        Q[1, lay.offset("nucleation_strike", s)], c["psize"][s], c["n_dip"][s])
    # tensors in: the same arrays; batches of one draw
    dev = R.rupture_front_ensemble(model, _dev(Q, ctx), _dev(Q[1], ctx), len(idx), c["xs"], c["ys"], batch=1)
    for a, b in zip(dev["subfaults"], out["subfaults"]):
        assert np.array_equal(a["density"], b["density"]) and np.array_equal(a["coverage"], b["coverage"])


def test_3_slip_vector_statistics(ctx, model):
    """mean and std within the bound DESIGN 3.9 derives for the running moments: n * 2^-52 * max|x| per column"""
    from beat_amd import rupture as R
    c = CASES["model"]
    Q = _population(model, np.concatenate([c["Q"] * f for f in np.linspace(0.9, 1.1, 23)]))          # 207 rows
    lay = model.problem.layout
    P, n = model.problem.npatches, Q.shape[0]
    rakes = [10.0, -75.0]
    out = R.slip_vector_statistics(model, Q, Q[4], rakes, c["xs"], c["ys"], batch=64)
    again = R.slip_vector_statistics(model, _dev(Q, ctx), Q[4], rakes, c["xs"], c["ys"], batch=207)
    off = np.concatenate([[0], np.cumsum(np.array(c["n_dip"]) * np.array(c["n_strike"]))])
    total = np.sqrt(sum(Q[4, lay.offset(v):lay.offset(v) + P] ** 2 for v in ("uparr", "uperp")))
    for s, sub in enumerate(out):
        sl = slice(off[s], off[s + 1])
        for name in ("uparr", "uperp"):
            x = Q[:, lay.offset(name):lay.offset(name) + P][:, sl]
            bound = n * 2.0 ** -52 * np.abs(x).max(axis=0)
            assert np.all(np.abs(sub["mean"][name] - x.mean(axis=0)) <= bound)
            assert np.all(np.abs(sub["std"][name] - x.std(axis=0)) <= bound)
            assert np.array_equal(sub["mean"][name], again[s]["mean"][name])        # the cut into calls changes no bit
            assert np.array_equal(sub["std"][name], again[s]["std"][name])
        assert not sub["mean"]["utens"].any() and not sub["std"]["utens"].any()
        assert sub["normalisation"] == total.max() / 3
        xg, yg = np.meshgrid(c["xs"][s], c["ys"][s])
        want = R.slip_vector_geometry(sub["mean"], sub["std"], 0.0, total.max(), rakes[s], xg, yg,
                                      dict(uparr=Q[4, lay.offset("uparr"):][:P][sl], uperp=Q[4, lay.offset("uperp"):][:P][sl]))
        for k in ("quivers", "ellipses", "reference_quivers"):
            assert np.array_equal(sub[k], want[k])
        assert sub["ellipses"].shape == (off[s + 1] - off[s], 100, 2)
