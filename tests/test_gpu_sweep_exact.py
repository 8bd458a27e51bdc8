"""The rupture-time sweep (csrc/sweep.hip) against a sequential CPU implementation of the same expressions, bit for bit.

sweep.hip promises "bitwise the times of a sequential implementation of the same expressions" (correctly rounded sqrt for
the reference's pow(x, 0.5)), that the unscaled Newton sqrt may stand in wherever SWEEP_PLAIN holds, and that the stop
decision err > 0.1 is the reference's although err is summed in another order.  The expectation is
oracle.fast_sweep_exact (oracle/beat_oracle.c bo_fast_sweep_exact: the reference's loops with sqrt and d*d, no FMA
contraction); tests/test_sweep_ref_host.py holds it to a second writing and checks that the inputs of tests/sweep_ref.py
are what they are named for.  Every comparison is np.array_equal on the float64 times: no tolerance.

Each case runs the default kernel and, for grids of at most 64 rows, the first version (BEATAMD_SWEEP_V1=1) too."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


def _versions(monkeypatch, ni, call):
    """-> [(name, result)]: the default kernel, and the first version where the default is not already it"""
    monkeypatch.delenv("BEATAMD_SWEEP_V1", raising=False)
    out = [("default", call())]
    if ni <= 64:
        monkeypatch.setenv("BEATAMD_SWEEP_V1", "1")
        out.append(("first version", call()))
        monkeypatch.delenv("BEATAMD_SWEEP_V1", raising=False)
    return out


# ---------------------------------------------------------------------------------------------------- explicit mode
@pytest.mark.parametrize("ni,nj", sr.GRIDS)
def test_explicit_sweep_is_bitwise_the_sequential_reference(ctx, monkeypatch, ni, nj):
    slow, hi, hj, names = sr.explicit_case(ni, nj)
    want, _, _ = sr.explicit_reference(ni, nj)
    for version, got in _versions(monkeypatch, ni, lambda: ctx.fast_sweep_batch(slow, sr.H, hi, hj, ni, nj)):
        assert got.shape == want.shape
        for c, name in enumerate(names):
            assert np.array_equal(got[c], want[c]), (ni, nj, name, version, _where(got[c], want[c]))


def _where(got, want):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    k = int(bad[0])
    return "%d cells differ, first %d: %r != %r" % (bad.size, k, float(got[k]), float(want[k]))


# ---------------------------------------------------------------------------------------------- four-wave workgroups
@pytest.mark.parametrize("C", sr.WG_COUNTS)
def test_four_wave_workgroups_keep_their_grids_apart(ctx, monkeypatch, C):
    """plain and non-plain grids, and grids of 1, 2 and six or more outer iterations, in the waves of one workgroup"""
    ni, nj = sr.WG_GRID
    slow, hi, hj, names, sel = sr.workgroup_case(C)
    want = sr.explicit_reference(ni, nj)[0][sel]
    for version, got in _versions(monkeypatch, ni, lambda: ctx.fast_sweep_batch(slow, sr.H, hi, hj, ni, nj)):
        for c, name in enumerate(names):
            assert np.array_equal(got[c], want[c]), (C, name, version, _where(got[c], want[c]))


# ------------------------------------------------------------------------------------------------------ the stop rule
@pytest.mark.parametrize("case", sr.STOP_CASES, ids=lambda c: "%dx%d-seed%d" % c[:3])
def test_stop_decision_is_the_sequential_sums(ctx, monkeypatch, case):
    """At this patch size the sequential err and the err in the kernel's summation order lie on opposite sides of 0.1
    (tests/test_sweep_ref_host.py): without the repeat of the sum in the reference's order the kernel would sweep one
    iteration fewer, or more, and return other times (c["wrong"])."""
    c = sr.stop_case(case)
    ni, nj = c["ni"], c["nj"]
    args = (c["slow"][None], c["h"], np.array([c["hi"]], dtype=np.int32), np.array([c["hj"]], dtype=np.int32), ni, nj)
    for version, got in _versions(monkeypatch, ni, lambda: ctx.fast_sweep_batch(*args)):
        assert not np.array_equal(got[0], c["wrong"]), (case, version, "the other stop decision's times")
        assert np.array_equal(got[0], c["times"]), (case, version, _where(got[0], c["times"]))


# ---------------------------------------------------------------------------------------------------- the model path
@pytest.mark.parametrize("which", range(len(sr.MODEL_SETS)))
def test_model_path_is_bitwise_the_sequential_reference(ctx, monkeypatch, which):
    """kernel mode 1 through CompiledModel.start_times: slowness = 1 / velocities, the hypocentre index by rint and a cast
    through int16 from nucleation positions on and beside the half-way ties, + the subfault's nucleation time"""
    from beat_amd.synthetic import build_problem
    grids, sizes = sr.MODEL_SETS[which]
    spec, layout, Q, _ = sr.model_population(which)
    want = sr.model_reference(which)
    prob, _ = build_problem(spec)
    model = prob.compile(ctx)
    try:
        for version, got in _versions(monkeypatch, min(g[0] for g in grids), lambda: model.start_times(Q)):
            assert got.shape == want.shape
            at = 0
            for sf, (nd, ns) in enumerate(grids):
                for c in range(Q.shape[0]):
                    a, b = got[c, at:at + nd * ns], want[c, at:at + nd * ns]
                    assert np.array_equal(a, b), (which, sf, c, version, _where(a, b))
                at += nd * ns
    finally:
        model.release()
