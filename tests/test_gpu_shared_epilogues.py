"""The misfit epilogues of the four lane-per-chain stacking kernels (gfshared.hip), through the fused model.

The kernels share their block decode, step iterator and epilogues; the parity tests assert kernel names for the
store-synthetics epilogue only.  Here every kernel runs the scalar-weight misfit (epilogue 1), the residual store in
front of a dense quadratic form (2) and the bidiagonal band (3 inside k_gfstack_ws, 2 + the banded kernel elsewhere) on
a toy library T, P, D, S, N = 3, 17, 3, 6, 200: the last 64-sample tile holds 8 samples; 70 chains are a partial second
wavefront, 530 chains two 512-chain groups with the second nearly empty.

One chain per lane and the same sample order in every kernel: no reduction order is involved, so the likelihood rows of
all of them are bitwise equal on the same (float-rounded) library."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (label, environment, float copies, reported name up to the mode; {m} = epilogue, {b} = epilogue of the band case)
KERNELS = [
    ("ws", {"BEATAMD_GS_CG": "512"}, False, "k_gfstack_ws<1,{b},3,"),
    ("wsp<1>", {"BEATAMD_GS_CG": "512"}, True, "k_gfstack_ws32<{m},3,"),
    ("wsp<0>", {"BEATAMD_GS_CG": "512", "BEATAMD_GS_PAIR": "1"}, False, "k_gfstack_wsp64<{m},3,"),
    ("dma 64", {"BEATAMD_GS_CG": "64"}, False, "k_gfstack_dma<1,1,{m},64,1>"),
    ("dma 512", {"BEATAMD_GS_CG": "512", "BEATAMD_GS_WS": "0"}, False, "k_gfstack_dma<8,1,{m},64,1>"),
    ("dmaf", {"BEATAMD_GS_CG": "128"}, True, "k_gfstack_dmaf<2,1,{m}>"),
]
KNOBS = ("BEATAMD_GF_KERNEL", "BEATAMD_GS_CG", "BEATAMD_GS_WS", "BEATAMD_GS_PAIR", "BEATAMD_QF_BAND")


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.mark.parametrize("C", [70, 530])
@pytest.mark.parametrize("epilogue", ["scalar", "dense", "band"])
def test_every_lane_per_chain_kernel_runs_every_misfit_epilogue(ctx, monkeypatch, epilogue, C):
    from beat_amd.synthetic import SyntheticSpec, build_problem
    spec = SyntheticSpec((17,), (1,), (1.0,), T=3, N=200, D=3, S=6, st_dt=1.5,     # (6 start times cover the 17 km rupture)
                         covariance="scalar" if epilogue == "scalar" else "toeplitz")
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    try:
        _run_every_kernel(ctx, monkeypatch, f, spec, host, epilogue, C)
    finally:
        f.release()


def _run_every_kernel(ctx, monkeypatch, f, spec, host, epilogue, C):
    from beat_amd.synthetic import draw_population
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], C)
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    if epilogue == "dense":
        monkeypatch.setenv("BEATAMD_QF_BAND", "0")     # the dense quadratic form behind the residual store
    mode = {"scalar": 1, "dense": 2, "band": 2}[epilogue]
    band = 3 if epilogue == "band" else mode           # the bidiagonal epilogue exists in k_gfstack_ws only
    f.round_libraries_to_f32()                         # one library for all kernels, the float ones included
    f.set_f32(False)
    monkeypatch.setenv("BEATAMD_GF_KERNEL", "0")
    S = f.batch(Q)
    assert ctx.last_kernel().startswith("k_gfstack<"), ctx.last_kernel()
    monkeypatch.setenv("BEATAMD_GF_KERNEL", "1")
    first = None
    for label, env, f32, name in KERNELS:
        for knob in ("BEATAMD_GS_CG", "BEATAMD_GS_WS", "BEATAMD_GS_PAIR"):
            monkeypatch.delenv(knob, raising=False)
        for knob, val in env.items():
            monkeypatch.setenv(knob, val)
        f.set_f32(f32)
        L = f.batch(Q)
        want = name.format(m=mode, b=band)
        assert ctx.last_kernel().startswith(want), (label, want, ctx.last_kernel())
        if first is None:
            first = L
        assert np.array_equal(L, first), label
        # the tolerance of test_fused_model_with_shared_row_kernel (tests/test_gpu_parity.py)
        np.testing.assert_allclose(S, L, rtol=1e-11, atol=1e-9, err_msg=label)
