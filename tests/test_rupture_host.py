"""CPU tests of the rupture-front arrays (beat_amd/rupture.py, csrc/rupture.hip): matplotlib's automatic levels, the
marching-squares restatement (tests/rupture_ref.py) against contourpy's lines and against the reference's own density
grids (tests/golden/rupture_fronts.npz, written by tools/gen_golden_rupture.py), the host arithmetic of the slip-vector
statistics, the argument rules that need no device, and the kernels' resource usage."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rupture_ref as rref  # noqa: E402
from conftest import ROOT  # noqa: E402

CASES, G = rref.load_cases(os.path.join(ROOT, "tests", "golden", "rupture_fronts.npz"))
NAMES = sorted(CASES)
LW = 7
ULP = 2.0 ** -53


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_fixture_has_the_cases_the_kernels_can_go_wrong_on():
    shapes = set(tuple(int(v) for v in r) for c in CASES.values() for r in c["shape"])
    assert {(2, 2), (3, 2), (9, 7), (12, 11), (20, 20), (33, 17)} <= shapes
    assert len(CASES["two"]["n_dip"]) == 2 and CASES["two"]["shape"][0].tolist() != CASES["two"]["shape"][1].tolist()
    assert (33 - 1) * (17 - 1) > 256
    # both saddle decisions in the checkerboard
    c = CASES["checkerboard"]
    z = c["sts"][0].reshape(c["n_dip"][0], c["n_strike"][0])
    lev = c["level_lists"][0][0][0]
    saddle = [len(rref.cell_segments(z, i, j, lev)) == 2 for i in range(z.shape[0] - 1) for j in range(z.shape[1] - 1)]
    centre = 0.25 * (((z[:-1, :-1] + z[:-1, 1:]) + z[1:, 1:]) + z[1:, :-1])
    assert sum(saddle) >= 10 and (centre > lev).any() and (centre <= lev).any()
    # levels equal to node values, 0 at the hypocentre among them, and the degenerate loop that draws nothing
    c = CASES["node_levels"]
    for lev in c["level_lists"][0][0]:
        assert (c["sts"][0] == lev).any()
    assert c["level_lists"][0][0][0] == 0.0
    z = c["sts"][0].reshape(c["n_dip"][0], c["n_strike"][0])
    loop = rref.level_lines(z, c["xs"][0], c["ys"][0], 0.0)
    assert len(loop) == 1 and len(loop[0]) == 5 and np.all(loop[0] == loop[0][0])
    assert not rref.line_image(loop[0], c["s0_extent"], *c["s0_grid"].shape, LW).any()
    # a plateau cell
    c = CASES["plateau"]
    z = c["sts"][0].reshape(7, 7)
    assert np.all(z[2:5, 2:5] == 1.5) and 1.5 in c["level_lists"][0][0]
    # a level with at least three lines, open and closed
    c = CASES["bumps"]
    z = c["sts"][0].reshape(c["n_dip"][0], c["n_strike"][0])
    lines = rref.level_lines(z, c["xs"][0], c["ys"][0], 0.5)
    closed = [bool(np.array_equal(ln[0], ln[-1])) for ln in lines]
    assert len(lines) >= 3 and any(closed) and not all(closed)


def test_auto_levels_equal_matplotlibs_recorded_levels():
    from beat_amd.rupture import auto_levels
    pairs, vals, counts = G["lev_pairs"], G["lev_values"], G["lev_counts"]
    assert len(pairs) >= 200 and (pairs[:, 0] == 0.0).sum() >= 100 and counts.max() <= 10
    for (lo, hi), v, n in zip(pairs, vals, counts):
        assert np.array_equal(auto_levels(lo, hi), v[:n]), (lo, hi)
    # and the levels matplotlib chose for the start times of every sweep case
    for name in NAMES:
        c = CASES[name]
        if name.startswith("s") or name in ("two", "model"):
            off = np.concatenate([[0], np.cumsum(np.array(c["n_dip"]) * np.array(c["n_strike"]))])
            for e in range(c["sts"].shape[0]):
                for s in range(len(c["n_dip"])):
                    z = c["sts"][e, off[s]:off[s + 1]]
                    assert np.array_equal(auto_levels(z.min(), z.max()), c["level_lists"][e][s]), (name, e, s)


def test_auto_levels_equal_live_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from beat_amd.rupture import auto_levels
    rng = np.random.default_rng(5)
    fig, ax = plt.subplots()
    try:
        for k in range(60):
            hi = float(10.0 ** rng.uniform(-4, 4))
            lo = 0.0 if k % 2 else float(rng.uniform(-2, 0.999) * hi)
            cs = ax.contour(np.array([[lo, hi], [hi, lo]]))
            assert np.array_equal(auto_levels(lo, hi), cs.levels), (lo, hi)
    finally:
        plt.close(fig)


def _canon(points, U, tol):
    """every point -> the first row of U within tol of it (per coordinate); -1: none"""
    out = np.empty(len(points), dtype=np.int64)
    for k, (p, t) in enumerate(zip(points, tol)):
        hit = np.nonzero(np.all(np.abs(U - p) <= t, axis=1))[0]
        out[k] = hit[0] if len(hit) else -1
    return out


def _segments(idx):
    return set((min(a, b), max(a, b)) for a, b in zip(idx[:-1], idx[1:]))


@pytest.mark.parametrize("name", NAMES)
def test_restated_topology_and_vertices_equal_contourpys(name):
    """per (draw, subfault, level): the restatement's segments are contourpy's as sets, vertices matched to the nearest, and
    every vertex lies within 16 * 2^-53 * max(|x_p|, |x_q|) of contourpy's (about four roundings in each of two equivalent
    interpolation formulas; measured on the fixture: 2.1 units at most)"""
    c = CASES[name]
    off = np.concatenate([[0], np.cumsum(np.array(c["n_dip"]) * np.array(c["n_strike"]))])
    cp_v, cp_lo, cp_lvl = c["cp_vertices"], c["cp_line_offsets"], c["cp_level_offsets"]
    worst = 0.0
    for e in range(c["sts"].shape[0]):
        for s in range(len(c["n_dip"])):
            z = c["sts"][e, off[s]:off[s + 1]].reshape(c["n_dip"][s], c["n_strike"][s])
            for l, lev in enumerate(c["level_lists"][e][s]):
                scales = []
                lines = rref.level_lines(z, c["xs"][s], c["ys"][s], float(lev), scales)
                cp_lines = [cp_v[cp_lo[k]:cp_lo[k + 1]] for k in range(cp_lvl[e, s, l], cp_lvl[e, s, l + 1])]
                assert len(lines) == len(cp_lines), (e, s, l)
                if not lines:
                    continue
                U = np.unique(np.concatenate(cp_lines), axis=0)
                big = 16 * ULP * np.array([np.abs(c["xs"][s]).max(), np.abs(c["ys"][s]).max()])
                ours, theirs = set(), set()
                for ln, sc in zip(lines, scales):
                    idx = _canon(ln, U, 16 * ULP * sc)
                    assert (idx >= 0).all(), (e, s, l)
                    worst = max(worst, float((np.abs(U[idx] - ln) / (ULP * sc)).max()))
                    ours |= _segments(idx)
                for ln in cp_lines:
                    theirs |= _segments(_canon(ln, U, np.broadcast_to(big, ln.shape)))
                assert ours == theirs, (e, s, l)
    print("%s: largest vertex distance %.2f units of 2^-53 max(|p|, |q|)" % (name, worst))
    assert worst <= 16.0


@pytest.mark.parametrize("name", NAMES)
def test_restated_drawing_of_contourpys_lines_equals_the_reference_grid(name):
    c = CASES[name]
    E = c["sts"].shape[0]
    for s in range(len(c["n_dip"])):
        lines = rref.subfault_lines(c["cp_level_offsets"], s)
        grid, cov = rref.polyline_density(c["cp_vertices"], c["cp_line_offsets"], c["s%d_extent" % s],
                                          c["s%d_grid" % s].shape, LW, lines=lines)
        assert np.array_equal(grid, c["s%d_raw" % s]) and np.array_equal(cov, c["s%d_coverage" % s])
        grid[grid > E / 2] = E / 2
        assert np.array_equal(grid, c["s%d_grid" % s])


@pytest.mark.parametrize("name", NAMES)
def test_restated_contours_give_the_recorded_coverage(name):
    c = CASES[name]
    v, lo, lvl = rref.contours(c["sts"], c["n_dip"], c["n_strike"], c["xs"], c["ys"], c["level_lists"])
    for s in range(len(c["n_dip"])):
        _, cov = rref.polyline_density(v, lo, c["s%d_extent" % s], c["s%d_grid" % s].shape, LW,
                                       lines=rref.subfault_lines(lvl, s))
        assert np.array_equal(cov, c["s%d_coverage" % s])


def _euler_to_matrix(alpha, beta, gamma):
    """pyrocko.moment_tensor.euler_to_matrix, restated from memory (unverified)"""
    ca, cb, cg = np.cos(alpha), np.cos(beta), np.cos(gamma)
    sa, sb, sg = np.sin(alpha), np.sin(beta), np.sin(gamma)
    return np.array([[cb * cg - ca * sb * sg, sb * cg + ca * cb * sg, sa * sg],
                     [-cb * sg - ca * sb * cg, -sb * sg + ca * cb * cg, sa * cg],
                     [sa * sb, -sa * cb, ca]])


def _transcription(uparr, uperp, utens, slip_max, rake, xgr, ygr):
    """plotting/ffi.py:687-733 on arrays, line by line -> (normalisation, U, V or None, list of (xcoords, ycoords))"""
    r2d, d2r = 180.0 / np.pi, np.pi / 180.0
    uparrmean, uperpmean, utensmean = uparr.mean(axis=0), uperp.mean(axis=0), utens.mean(axis=0)
    U = V = None
    if uparrmean.sum() != 0.0:
        normalisation = slip_max / 3
        angles = np.arctan2(-uperpmean, uparrmean) * r2d + rake
        slips = np.sqrt((uperpmean ** 2 + uparrmean ** 2)).ravel()
        slips /= normalisation
        U, V = np.cos(angles * d2r) * slips, np.sin(angles * d2r) * slips
        uparrstd = uparr.std(axis=0) / normalisation
        uperpstd = uperp.std(axis=0) / normalisation
    elif utensmean.sum() != 0:
        uperpstd = uparrstd = utens.std(axis=0)
        normalisation = utens.max()
    slipvecrotmat = _euler_to_matrix(0.0, 0.0, rake * d2r)
    circle = np.linspace(0, 2 * np.pi, 100)
    curves = []
    for i, (upe, upa) in enumerate(zip(uperpstd, uparrstd)):
        ellipse_x = 2 * upa * np.cos(circle)
        ellipse_y = 2 * upe * np.sin(circle)
        ellipse = np.vstack([ellipse_x, ellipse_y, np.zeros_like(ellipse_x)]).T
        rot_ellipse = ellipse.dot(slipvecrotmat)
        xcoords = xgr.ravel()[i] + rot_ellipse[:, 0]
        ycoords = ygr.ravel()[i] + rot_ellipse[:, 1]
        if U is not None:
            xcoords += U[i]
            ycoords += V[i]
        curves.append((xcoords, ycoords))
    return normalisation, U, V, curves


@pytest.mark.parametrize("tensile", [False, True])
def test_slip_vector_geometry_equals_a_transcription_of_the_reference(tensile):
    from beat_amd.rupture import slip_vector_geometry
    rng = np.random.default_rng(11 + tensile)
    n, nd, ns, rake = 200, 3, 4, 37.5
    P = nd * ns
    uparr = np.zeros((n, P)) if tensile else rng.uniform(0, 4, (n, P))
    uperp = np.zeros((n, P)) if tensile else rng.uniform(-1, 1, (n, P))
    utens = rng.uniform(0, 2, (n, P)) if tensile else np.zeros((n, P))
    xgr, ygr = np.meshgrid(0.5 + np.arange(ns), 0.5 + np.arange(nd))
    slip_max = 5.25
    norm, U, V, curves = _transcription(uparr, uperp, utens, slip_max, rake, xgr, ygr)
    mean = dict(uparr=uparr.mean(axis=0), uperp=uperp.mean(axis=0), utens=utens.mean(axis=0))
    std = dict(uparr=uparr.std(axis=0), uperp=uperp.std(axis=0), utens=utens.std(axis=0))
    ref_pt = dict(uparr=uparr[3], uperp=uperp[3])
    out = slip_vector_geometry(mean, std, utens.max(), slip_max, rake, xgr, ygr, ref_pt)
    assert out["normalisation"] == norm
    if tensile:
        assert out["quivers"] is None and out["reference_quivers"] is None
    else:
        assert np.array_equal(out["quivers"][:, 0], U) and np.array_equal(out["quivers"][:, 1], V)
        # the black quivers of the reference point (:737-753) with the same normalisation
        ang = np.arctan2(-uperp[3], uparr[3]) * (180.0 / np.pi) + rake
        sl = np.sqrt((uperp[3] ** 2 + uparr[3] ** 2)) / norm
        assert np.array_equal(out["reference_quivers"][:, 0], np.cos(ang * (np.pi / 180.0)) * sl)
    assert out["ellipses"].shape == (P, 100, 2)
    for i, (xc, yc) in enumerate(curves):
        assert np.array_equal(out["ellipses"][i, :, 0], xc) and np.array_equal(out["ellipses"][i, :, 1], yc)
    with pytest.raises(ValueError, match="zero"):
        z = dict(uparr=np.zeros(P), uperp=np.zeros(P), utens=np.zeros(P))
        slip_vector_geometry(z, z, 0.0, 1.0, rake, xgr, ygr)


def test_argument_rules_that_need_no_device():
    from beat_amd import rupture as R, rupture_binding as rb
    hpp = open(os.path.join(ROOT, "beat_amd", "csrc", "kernels.hpp")).read()
    assert "CT_LMAX = %d" % rb.LMAX in hpp and "CT_MAX_NODES = %d" % rb.MAX_NODES in hpp
    assert "CT_SUB_FIELDS = %d" % rb.SUB_FIELDS in hpp
    subs = rb.subfault_table([6, 8], [9, 5])
    assert subs.tolist() == [[6, 9, 0, 0, 0], [8, 5, 54, 9, 6]]
    assert rb.subfault_table(48, 48).shape == (1, 5)
    with pytest.raises(ValueError, match="2304"):
        rb.subfault_table(49, 48)
    with pytest.raises(ValueError):
        rb.subfault_table([3, 4], [5])
    x, y = rb.check_coordinates(np.arange(5.0), np.arange(3.0)[::-1], rb.subfault_table(3, 5))
    assert x.tolist() == [0, 1, 2, 3, 4] and y.tolist() == [2, 1, 0]
    with pytest.raises(ValueError, match="monotone"):
        rb.check_coordinates([0.0, 1.0, 1.0, 2.0, 3.0], np.arange(3.0), rb.subfault_table(3, 5))
    with pytest.raises(ValueError, match="subfault 0 must be"):
        rb.check_coordinates(np.arange(4.0), np.arange(3.0), rb.subfault_table(3, 5))
    with pytest.raises(ValueError, match="not finite"):
        lv = np.zeros((2, 1, rb.LMAX))
        lv[1, 0, 1] = np.nan
        rb.check_levels(lv, np.full((2, 1), 3, dtype=np.int32), 2, 1)
    with pytest.raises(ValueError, match="at most 16"):
        R._level_tables(list(np.arange(17.0)), 1, 1)
    with pytest.raises(ValueError, match="increasing"):
        R._level_tables([1.0, 1.0], 1, 1)
    lv, nl = R._level_tables([[0.0, 1.0], [2.0]], 2, 1)
    assert nl.ravel().tolist() == [2, 1] and lv[1, 0, 0] == 2.0
    for size in ((1, 10), (10, 4097)):
        with pytest.raises(ValueError, match="2 ... 4096"):
            rb.check_grid_size(size)
    # fuzzy_rupture_fronts' grid, restated as written
    ext, shape = R.front_grid(0.5 + np.arange(20.0), 0.5 + np.arange(20.0))
    assert ext == (0.5, 19.5, 0.5, 19.5) and shape == (475, 475)
    with pytest.raises(ValueError, match="pixels"):
        R.front_grid([0.5, 0.52], [0.5, 1.5])
    with pytest.raises(ValueError, match="pixels"):
        R.front_grid(np.arange(0.0, 200.0, 10.0), [0.5, 1.5])
    assert R.hypocentre_marker(3.2, 7.9, 2.0, 6) == (7.0, 9.0)
    assert np.array_equal(R.euler_rotation_z(0.3), _euler_to_matrix(0.0, 0.0, 0.3))


@pytest.mark.skipif(_gpu_present(), reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    from beat_amd import BeatAmdError, rupture as R
    c = CASES["s3x2"]
    with pytest.raises(BeatAmdError):
        R.start_time_contours(c["sts"], c["n_dip"], c["n_strike"], c["xs"], c["ys"])
    with pytest.raises(BeatAmdError):
        R.polyline_density(c["cp_vertices"], c["cp_line_offsets"], c["s0_extent"], c["s0_grid"].shape)


KERNELS = ("k_rupture_minmax", "k_contour_count", "k_contour_fill", "k_polyline_check", "k_polyline_density")


def test_rupture_kernels_compile_for_gfx950_without_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "beat_amd", "csrc", "rupture.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "rupture.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    scratch, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    assert len(scratch) == len(KERNELS), sorted(scratch)
    for kern in KERNELS:
        hits = [k for k in scratch if kern in k]
        assert hits and all(scratch[k] == 0 for k in hits), (kern, scratch)
