"""CPU tests of tests/sweep_ref.py and oracle.fast_sweep_exact, the expectation of tests/test_gpu_sweep_exact.py: the C and
the numpy writing of the exact expressions give equal bits and equal iteration counts on every case the GPU file runs;
the exact expressions stay within a measured, printed distance of the reference's pow arithmetic; every case builder
delivers the property it is named for, computed in the kernel's expression order; every stop-rule case has the sequential
and the kernel-order err on opposite sides of 0.1 at the committed patch size, the other decision changes the times, and
the CPU model of the kernel's stop rule without its fallback to the sequential sum returns those other times."""
import glob
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_ref as sr  # noqa: E402
from oracle import oracle as orc  # noqa: E402


# ------------------------------------------------------------------------------------------ the two restatements agree
@pytest.mark.parametrize("ni,nj", sr.GRIDS)
def test_c_and_numpy_restatements_agree_explicit(ni, nj):
    slow, hi, hj, names = sr.explicit_case(ni, nj)
    times, iters, _ = sr.explicit_reference(ni, nj)
    t, it = sr.host_sweep(slow, sr.H, hi, hj, ni, nj)
    for c, name in enumerate(names):
        assert np.array_equal(t[c], times[c], equal_nan=True), (ni, nj, name)
    assert np.array_equal(it, iters), (ni, nj)
    assert not np.isnan(times).any()


def test_c_and_numpy_restatements_agree_stop_cases():
    cases = [sr.stop_case(c) for c in sr.STOP_CASES]
    for shape in sorted({(c["ni"], c["nj"]) for c in cases}):
        sel = [c for c in cases if (c["ni"], c["nj"]) == shape]
        t, it = sr.host_sweep(np.array([c["slow"] for c in sel]), np.array([c["h"] for c in sel]),
                              np.array([c["hi"] for c in sel]), np.array([c["hj"] for c in sel]), *shape)
        for k, c in enumerate(sel):
            assert np.array_equal(t[k], c["times"]) and it[k] == c["iters"], (shape, c["h"].hex())


@pytest.mark.parametrize("which", range(len(sr.MODEL_SETS)))
def test_c_and_numpy_restatements_agree_model_sets(which):
    grids, sizes = sr.MODEL_SETS[which]
    spec, layout, Q, _ = sr.model_population(which)
    ref = sr.model_reference(which)
    at = 0
    for sf, ((nd, ns), h) in enumerate(zip(grids, sizes)):
        n = nd * ns
        v0 = layout.offset("velocities") + at
        hi = np.rint((Q[:, layout.offset("nucleation_dip", sf)] - h / 2.0) / h).astype(np.int16).astype(np.int32)
        hj = np.rint((Q[:, layout.offset("nucleation_strike", sf)] - h / 2.0) / h).astype(np.int16).astype(np.int32)
        assert np.array_equal(hi, orc.positions2idxs(Q[:, layout.offset("nucleation_dip", sf)], h))
        assert np.array_equal(hj, orc.positions2idxs(Q[:, layout.offset("nucleation_strike", sf)], h))
        t, _ = sr.host_sweep(1.0 / Q[:, v0:v0 + n], h, hi, hj, nd, ns)
        assert np.array_equal(t + Q[:, [layout.offset("time", sf)]], ref[:, at:at + n]), (which, sf)
        at += n
    assert at == spec.P and np.isfinite(ref).all()


# ------------------------------------------------------------------------- distance from the reference's own arithmetic
# measured on sr.pow_cases() (1200 grids) with glibc's pow on x86-64: 20 of 147,406 cells differ, by 2 ulp at the most
POW_ULP_MEASURED = 2
POW_ULP_BOUND = 2 * POW_ULP_MEASURED         # the margin: another libm's pow


def _load_ref_extension():
    so = glob.glob(os.path.join(os.path.dirname(os.path.abspath(orc.__file__)), "_ref", "fast_sweep_ext*.so"))
    if not so:
        return None
    spec = importlib.util.spec_from_file_location("fast_sweep_ext", so[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_exact_expressions_against_the_reference_pow():
    ext = _load_ref_extension()
    cells = differ = worst = 0
    for slow, h, hi, hj, ni, nj in sr.pow_cases():
        exact, it_exact, _ = orc.fast_sweep_exact(slow, h, hi, hj, ni, nj, with_err=True)
        with_pow, it_pow = orc.fast_sweep(slow, h, hi, hj, ni, nj, with_iters=True)
        assert it_pow == it_exact
        others = [with_pow]
        if ext is not None:
            others.append(np.asarray(ext.fast_sweep(slow, h, hi, hj, ni, nj)))
            assert np.array_equal(others[0], others[1])
        for o in others:
            assert np.array_equal(np.isnan(o), np.isnan(exact)) and np.array_equal(np.isinf(o), np.isinf(exact))
            d = sr.ulp_distance(o, exact)
            worst = max(worst, int(d.max()))
        cells += exact.size
        differ += int((sr.ulp_distance(others[0], exact) > 0).sum())
    print("sqrt and d*d against pow: %d of %d cells differ (%.4f %%), at most %d ulp; reference extension %s"
          % (differ, cells, 100.0 * differ / cells, worst, "compared too" if ext is not None else "not built here"))
    assert worst <= POW_ULP_BOUND
    assert differ > 0      # (were they equal everywhere, the pow oracle would do for the bitwise test)


# ----------------------------------------------------------------------------------- the builders deliver their property
def _field(ni, nj, name):
    slow, _, _, names = sr.explicit_case(ni, nj)
    return slow[[n.split("@")[0] for n in names].index(name)]


def test_iteration_counts_present():
    iters = np.concatenate([sr.explicit_reference(ni, nj)[1] for ni, nj in sr.GRIDS])
    for want in (1, 2, 3):
        assert (iters == want).any(), np.bincount(iters)
    assert (iters >= 6).any(), np.bincount(iters)
    # every grid with an interior has a grid of at least three iterations; the large ones one of six or more
    for ni, nj in sr.GRIDS:
        it = sr.explicit_reference(ni, nj)[1]
        if min(ni, nj) >= 16:
            assert it.max() >= 6, (ni, nj, it)


def test_grids_that_end_on_a_nan_err_are_present():
    for ni, nj in sr.GRIDS:
        if ni * nj < 3:
            continue
        slow, hi, hj, names = sr.explicit_case(ni, nj)
        times, iters, last = sr.explicit_reference(ni, nj)
        sel = [c for c, n in enumerate(names) if n.startswith("inf@")]
        # a cell that is never reached stays +inf, inf - inf makes err NaN and NaN > 0.1 ends the loop
        assert sel and all(np.isnan(last[c]) and np.isinf(times[c]).any() for c in sel), (ni, nj)
        assert all(np.isfinite(times[c]).any() for c in sel)


def test_non_plain_cells_are_present():
    for ni, nj in sr.GRIDS:
        tiny, one = _field(ni, nj, "tiny"), _field(ni, nj, "onefail")
        assert not sr.plain_cells(tiny, sr.H).any()
        assert (~sr.plain_cells(one, sr.H)).sum() == 1
        for name in ("uniform", "random", "huge", "window", "checker", "maze"):
            assert sr.plain_cells(_field(ni, nj, name), sr.H).all(), (ni, nj, name)


def test_overflow_window_cells_are_present():
    for ni, nj in sr.GRIDS:
        w = _field(ni, nj, "window")
        ovf = sr.overflow_cells(w, sr.H)
        assert ovf.any(), (ni, nj)
        if ni * nj >= 15:
            assert (~ovf).any()
        # the "huge" field does not reach the window
        assert not sr.overflow_cells(_field(ni, nj, "huge"), sr.H).any()
    # the window takes part: on a row, where only the linear arm runs, its times are finite sums of S = f*h near 1e154
    times, _, _ = sr.explicit_reference(1, 7)
    _, _, _, names = sr.explicit_case(1, 7)
    t = times[names.index("window@0,0")]
    assert np.isfinite(t).all() and t.max() > 1e153


def test_workgroup_batches_mix_what_they_claim():
    ni, nj = sr.WG_GRID
    assert ni * nj <= 512                                  # four grids per workgroup
    _, iters, _ = sr.explicit_reference(ni, nj)
    slow, hi, hj, names, sel = sr.workgroup_case(max(sr.WG_COUNTS))
    assert sorted(sr.WG_COUNTS) == [1, 4, 5, 9] and len(sel) == 9
    plain = [bool(sr.plain_cells(s, sr.H).all()) for s in slow]
    first = [int(iters[s]) for s in sel[:4]]
    assert plain[:4] == [True, False, True, False]         # __all(plain) of one wave must not reach its neighbours
    assert 1 in first and 2 in first and max(first) >= 6, first
    assert not all(plain[4:8]) and any(plain[4:8])


def test_model_sets_hold_ties_of_both_parities_and_their_neighbours():
    for which, (grids, sizes) in enumerate(sr.MODEL_SETS):
        spec, layout, Q, ties = sr.model_population(which)
        parities, moved = set(), 0
        for (sf, axis), rec in ties.items():
            h = sizes[sf]
            col = layout.offset(axis, sf)
            n = grids[sf][0 if axis == "nucleation_dip" else 1]
            for c, k, step in rec:
                x = (Q[c, col] - 0.0 - (h / 2.0)) / h      # the kernel's expression
                idx = int(orc.positions2idxs(Q[c:c + 1, col], h)[0])
                assert 0 <= idx < n
                if step == 0:
                    assert x == k + 0.5 and idx == (k if k % 2 == 0 else k + 1)     # half to even
                    parities.add(k % 2)
                else:
                    assert idx in (k, k + 1)
                    moved += idx != (k if k % 2 == 0 else k + 1)
        assert parities == {0, 1}, which
        assert moved > 0, which        # a neighbouring double of a tie rounds the other way
        assert Q[:, layout.offset("time", 0)].min() > 0.0 and Q[:, layout.offset("time", 1)].min() > 0.0
    assert sorted({h for _, sizes in sr.MODEL_SETS for h in sizes}) == [0.5, 0.7, 1.0]


# ------------------------------------------------------------------------------------------------------ the stop rule
def test_stop_cases_cover_both_directions_and_grid_sizes():
    early = [c for c in sr.STOP_CASES if c[5] == "kernel_stops_early"]
    runs_on = [c for c in sr.STOP_CASES if c[5] == "kernel_runs_on"]
    assert len(early) + len(runs_on) == len(sr.STOP_CASES) and early and runs_on
    for group in (early, runs_on):
        assert any(c[0] * c[1] > 64 for c in group) and any(c[0] * c[1] <= 64 for c in group)
    assert len({(c[0], c[1]) for c in sr.STOP_CASES}) >= 2


@pytest.mark.parametrize("case", sr.STOP_CASES, ids=lambda c: "%dx%d-seed%d" % c[:3])
def test_stop_case_straddles_the_threshold_and_the_decision_matters(case):
    c = sr.stop_case(case)
    k = c["k"]
    # opposite sides of 0.1, both inside the window in which the kernel repeats the sum
    assert (c["seq"] > sr.ERR_STOP) != (c["ker"] > sr.ERR_STOP)
    assert abs(c["ker"] - sr.ERR_STOP) <= sr.ERR_WINDOW and abs(c["seq"] - sr.ERR_STOP) <= sr.ERR_WINDOW
    assert c["seq"] == c["errs"][k - 1] and (c["errs"][:k - 1] > 1.0).all()
    if c["direction"] == "kernel_stops_early":
        assert c["seq"] > sr.ERR_STOP and c["iters"] > k
    else:
        assert c["seq"] <= sr.ERR_STOP and c["iters"] == k
    # the wrong decision (one iteration fewer, or one more) changes at least one time
    assert not np.array_equal(c["wrong"], c["times"])
    assert np.isfinite(c["times"]).all() and np.isfinite(c["wrong"]).all()
    # the kernel's stop rule as written gives the reference's times; with the fallback taken out it gives others
    args = (c["slow"][None], c["h"], np.array([c["hi"]]), np.array([c["hj"]]), c["ni"], c["nj"])
    with_fb, it_fb = sr.host_sweep(*args, err_order="kernel", fallback=True)
    assert np.array_equal(with_fb[0], c["times"]) and it_fb[0] == c["iters"]
    without, it_no = sr.host_sweep(*args, err_order="kernel", fallback=False)
    assert not np.array_equal(without[0], c["times"])
    assert it_no[0] != c["iters"]
    if c["direction"] == "kernel_stops_early":
        assert it_no[0] == k and np.array_equal(without[0], c["wrong"])
    else:
        assert it_no[0] > k
        if it_no[0] == k + 1:
            assert np.array_equal(without[0], c["wrong"])
