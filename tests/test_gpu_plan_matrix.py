"""The plan of a stacking call over the branches of its selection (csrc: GfPlan, gf_plan_call): for the smallest shape that
reaches each branch, which kernel ran, what the plan text says and how many chains a group holds are the ones recorded on
the commit before the planner existed; where the branch is not the streaming kernel itself, the result is bit for bit the
streaming kernel's (BEATAMD_GF_KERNEL=0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, P, D, S, N = 2, 5, 3, 11, 64   # unless a case says otherwise

# id -> (kind, arguments, knobs).  kind "stack": SeismicGFLibrary.stack_all_batch of a random library [T, P, D, S, N] with
# C chains; kind "model": LogpForwFunc.batch of a beat_amd.synthetic problem.  BEATAMD_GS_TUNE=0 everywhere: no group size is
# chosen by timing.
CASES = {}


def _stack(name, C, interp="nearest_neighbor", knobs=(), **shape):
    CASES[name] = ("stack", dict(dict(C=C, interp=interp, T=T, P=P, D=D, S=S, N=N), **shape), dict(knobs))


def _model(name, C, knobs=(), f32=False, **spec):
    CASES[name] = ("model", dict(C=C, f32=f32, spec=spec), dict(knobs))


# 1, 2: the streaming kernel -- fewer than 48 chains; an odd sample count
_stack("1 C=40 nn", 40)
_stack("2 C=64 N=63", 64, N=63)
# 3: k_gfstack_dma with one row / four rows per chain
_stack("3 C=64 nn", 64)
_stack("3 C=100 ml", 100, "multilinear")
# 4: either side of the runs kernel's threshold
_stack("4 C=191 ml", 191, "multilinear")
_stack("4 C=192 ml", 192, "multilinear")
# 5: k_gfstack_ws with one group; one chain more: the static table prefers three 256-chain groups, and two 512-chain groups
# where the size is fixed (nthint and the XCD grid order flip)
_stack("5 C=512 nn", 512)
_stack("5 C=513 nn", 513)
_stack("5 C=513 nn GS_CG=512", 513, knobs={"BEATAMD_GS_CG": "512"})
# 6: one knob each at 512 chains
for _k, _v in (("GS_WS", "0"), ("GS_CG", "1024"), ("GS_CG", "256"), ("GS_DMA", "1"), ("GS_NT", "32"), ("GS_PAIR", "1")):
    _stack("6 C=512 nn %s=%s" % (_k, _v), 512, knobs={"BEATAMD_" + _k: _v})
# 7: more rows per patch than an LDS buffer of k_gfstack_ws holds
_stack("7 C=512 nn D*S=12*20", 512, D=12, S=20)
# 8, 9: who evaluates the bidiagonal misfit -- k_quadform_band1 behind a residual store, k_gfstack_ws, the runs kernel, the
# combine kernel of the patch ranges; then each without the fused epilogue
_BAND1 = {
    "C=64 N=128": dict(C=64, N=128),
    "C=512 N=128": dict(C=512, N=128),
    "C=192 ml": dict(C=192, N=64, interpolation="multilinear"),
    "C=512 N=120 P=64 T=1": dict(C=512, N=120, T=1, patches=(8, 8), S=15),   # (15 start times cover the 8 x 8 km rupture)
}
for _n, _a in _BAND1.items():
    _model("8 band1 " + _n, covariance="exponential", **_a)
    _model("9 band1 " + _n + " QF_FUSE=0", covariance="exponential", knobs={"BEATAMD_QF_FUSE": "0"}, **_a)
# 10: float rows -- the pair-gather kernel has no bidiagonal epilogue
_model("10 band1 C=512 N=128 f32", covariance="exponential", f32=True, **_BAND1["C=512 N=128"])
# 11: the patch ranges of a short-trace library, tables per chain / per station slot
for _C in (64, 512):
    for _i in ("nearest_neighbor", "multilinear"):
        for _s in (False, True):
            _model("11 split C=%d %s%s" % (_C, "ml" if _i == "multilinear" else "nn", " shifts" if _s else ""), C=_C, N=120, T=1,
                   patches=(8, 8), S=15, interpolation=_i, station_shifts=_s, covariance="scalar")

# (last_kernel, plan, chains_per_group) of every case, recorded by running `_observe` below on the commit before the
# planner (d7dd79f) on an MI355X
EXPECTED = {
    '1 C=40 nn': ('k_gfstack<0,1,1,2,0>',
        'streaming kernel: fewer than 48 chains share too few rows',
        0),
    '2 C=64 N=63': ('k_gfstack<0,1,1,1,0>',
        'streaming kernel: odd sample count (the chain-shared kernels move 16-byte lanes)',
        0),
    '3 C=64 nn': ('k_gfstack_dma<1,1,0,64,1>',
        'lane <-> chain kernel with 64-chain groups (small batch): row buffers of 33 slots',
        64),
    '3 C=100 ml': ('k_gfstack_dma<2,4,0,64,1>',
        'lane <-> chain kernel with 128-chain groups (small batch): row buffers of 33 slots',
        128),
    '4 C=191 ml': ('k_gfstack_dma<4,4,0,64,1>',
        'lane <-> chain kernel with 256-chain groups (small batch): row buffers of 33 slots',
        256),
    '4 C=192 ml': ('k_gfstack_runs<0,1>',
        'runs kernel: 518-chain groups, multilinear; 104 row slots per LDS buffer (a patch has D*(S+1) = 36 '
        'dense slots), one pass per patch',
        518),
    '5 C=512 nn': ('k_gfstack_ws<1,0,3,1>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 64 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 33) rows), one pass per patch',
        512),
    '5 C=513 nn': ('k_gfstack_dma<4,1,0,64,1>',
        'lane <-> chain kernel with 256-chain groups (group size measured fastest): row buffers of 33 slots',
        256),
    '5 C=513 nn GS_CG=512': ('k_gfstack_ws<1,0,3,0>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 64 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 33) rows), one pass per patch',
        512),
    '6 C=512 nn GS_WS=0': ('k_gfstack_dma<8,1,0,64,1>',
        'lane <-> chain kernel with 512-chain groups (group size measured fastest): row buffers of 64 slots',
        512),
    '6 C=512 nn GS_CG=1024': ('k_gfstack_dma<16,1,0,32,1>',
        'lane <-> chain kernel with 1024-chain groups (group size measured fastest): row buffers of 64 slots',
        1024),
    '6 C=512 nn GS_CG=256': ('k_gfstack_dma<4,1,0,64,1>',
        'lane <-> chain kernel with 256-chain groups (group size measured fastest): row buffers of 33 slots',
        256),
    '6 C=512 nn GS_DMA=1': ('k_gfstack_dma<8,1,0,64,0>',
        'lane <-> chain kernel with 512-chain groups (group size measured fastest): row buffers of 33 slots',
        512),
    '6 C=512 nn GS_NT=32': ('k_gfstack_dma<8,1,0,32,1>',
        'lane <-> chain kernel with 512-chain groups (group size measured fastest): row buffers of 64 slots',
        512),
    '6 C=512 nn GS_PAIR=1': ('k_gfstack_wsp64<0,3,1>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 64 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 33) rows), one pass per patch',
        512),
    '7 C=512 nn D*S=12*20': ('k_gfstack_ws<1,0,3,1>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 96 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 240) rows), patches that touch more are staged in passes of equal size',
        512),
    '8 band1 C=64 N=128': ('k_gfstack_dma<1,1,2,64,1>',
        'lane <-> chain kernel with 64-chain groups (small batch): row buffers of 33 slots',
        64),
    '9 band1 C=64 N=128 QF_FUSE=0': ('k_gfstack_dma<1,1,2,64,1>',
        'lane <-> chain kernel with 64-chain groups (small batch): row buffers of 33 slots',
        64),
    '8 band1 C=512 N=128': ('k_gfstack_ws<1,3,3,1>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 64 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 33) rows), one pass per patch',
        512),
    '9 band1 C=512 N=128 QF_FUSE=0': ('k_gfstack_ws<1,2,3,1>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 64 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 33) rows), one pass per patch',
        512),
    '8 band1 C=192 ml': ('k_gfstack_runs<3,1>',
        'runs kernel: 518-chain groups, multilinear; 104 row slots per LDS buffer (a patch has D*(S+1) = 36 '
        'dense slots), one pass per patch',
        518),
    '9 band1 C=192 ml QF_FUSE=0': ('k_gfstack_runs<2,1>',
        'runs kernel: 518-chain groups, multilinear; 104 row slots per LDS buffer (a patch has D*(S+1) = 36 '
        'dense slots), one pass per patch',
        518),
    '8 band1 C=512 N=120 P=64 T=1': ('k_gfstack_ws<1,0,3,1>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 64 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 45) rows), one pass per patch; 120-sample traces: patches stacked in 2 '
        'ranges of 32 (4 walks instead of 2), partial synthetics summed in range order',
        512),
    '9 band1 C=512 N=120 P=64 T=1 QF_FUSE=0': ('k_gfstack_ws<1,0,3,1>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 64 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 45) rows), one pass per patch; 120-sample traces: patches stacked in 2 '
        'ranges of 32 (4 walks instead of 2), partial synthetics summed in range order',
        512),
    '10 band1 C=512 N=128 f32': ('k_gfstack_ws32<2,3,1>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 64 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 33) rows), one pass per patch',
        512),
    '11 split C=64 nn': ('k_gfstack_ws<1,0,3,1>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 64 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 45) rows), one pass per patch; 120-sample traces: patches stacked in 2 '
        'ranges of 32 (4 walks instead of 2), partial synthetics summed in range order',
        512),
    '11 split C=64 nn shifts': ('k_gfstack_ws<1,0,3,1>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 64 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 45) rows), one pass per patch; 120-sample traces: patches stacked in 2 '
        'ranges of 32 (4 walks instead of 2), partial synthetics summed in range order',
        512),
    '11 split C=64 ml': ('k_gfstack<1,1,1,2,0>',
        'streaming kernel: chosen by BEATAMD_GF_KERNEL or no chain-shared kernel fits this library; '
        '120-sample traces: patches stacked in 2 ranges of 32 (4 walks instead of 2), partial synthetics '
        'summed in range order',
        0),
    '11 split C=64 ml shifts': ('k_gfstack<1,1,1,2,0>',
        'streaming kernel: chosen by BEATAMD_GF_KERNEL or no chain-shared kernel fits this library; '
        '120-sample traces: patches stacked in 2 ranges of 32 (4 walks instead of 2), partial synthetics '
        'summed in range order',
        0),
    '11 split C=512 nn': ('k_gfstack_ws<1,0,3,1>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 64 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 45) rows), one pass per patch; 120-sample traces: patches stacked in 2 '
        'ranges of 32 (4 walks instead of 2), partial synthetics summed in range order',
        512),
    '11 split C=512 nn shifts': ('k_gfstack_ws<1,0,3,1>',
        'loader/consumer kernel: 512-chain groups, nearest neighbour; 64 row slots per LDS buffer (a patch '
        'can touch min(512, D*S = 45) rows), one pass per patch; 120-sample traces: patches stacked in 2 '
        'ranges of 32 (4 walks instead of 2), partial synthetics summed in range order',
        512),
    '11 split C=512 ml': ('k_gfstack_runs<0,1>',
        'runs kernel: 518-chain groups, multilinear; 104 row slots per LDS buffer (a patch has D*(S+1) = 48 '
        'dense slots), one pass per patch; 120-sample traces: patches stacked in 2 ranges of 32 (4 walks '
        'instead of 2), partial synthetics summed in range order',
        518),
    '11 split C=512 ml shifts': ('k_gfstack_runs<0,1>',
        'runs kernel: 518-chain groups, multilinear; 104 row slots per LDS buffer (a patch has D*(S+1) = 48 '
        'dense slots), one pass per patch; 120-sample traces: patches stacked in 2 ranges of 32 (4 walks '
        'instead of 2), partial synthetics summed in range order',
        518),
}


def _run(ctx, kind, a):
    """one call of the case on ctx -> a function that repeats it"""
    if kind == "stack":
        from beat_amd.ffi import SeismicGFLibrary, SeismicGFLibraryConfig
        rng = np.random.default_rng(a["D"] * a["S"] + a["C"])
        G = rng.standard_normal((a["T"], a["P"], a["D"], a["S"], a["N"]))
        gf = SeismicGFLibrary(SeismicGFLibraryConfig(dimensions=G.shape, starttime_sampling=0.5, duration_sampling=0.5,
                                                     starttime_min=0.0, duration_min=0.5))
        gf.setup(*G.shape, allocate=True)
        gf._gfmatrix[:] = G
        gf.init_optimization(ctx)
        dur = 0.5 + 0.5 * rng.uniform(0, a["D"] - 1, (a["C"], a["P"]))
        st = 0.5 * rng.uniform(0, a["S"] - 1, (a["C"], a["T"], a["P"]))
        sl = rng.uniform(-2, 2, (a["C"], a["P"]))
        return lambda: np.asarray(gf.stack_all_batch(dur, st, sl, interpolation=a["interp"]))
    from beat_amd.synthetic import SyntheticSpec, build_problem, draw_population
    kw = dict(dict(T=T, N=N, D=D, S=S), **a["spec"])
    dip, strike = kw.pop("patches", (P, 1))
    spec = SyntheticSpec((dip,), (strike,), (1.0,), **kw)
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    if a["f32"]:
        f.round_libraries_to_f32()
        f.set_f32()
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], a["C"])
    return lambda: np.asarray(f.batch(Q))


def _observe(name, setenv):
    """the case on a context of its own (no earlier launch sizes a row buffer) -> what it launched, and whether the
    streaming kernel gives the same bits"""
    from beat_amd.engine import Context
    kind, a, knobs = CASES[name]
    setenv("BEATAMD_GS_TUNE", "0")
    for k, v in knobs.items():
        setenv(k, v)
    ctx = Context(0)
    try:
        call = _run(ctx, kind, a)
        out = call()
        seen = (ctx.last_kernel(), ctx.gf_plan()["plan"], ctx.gf_group_stats()["chains_per_group"])
        same = None
        if not seen[0].startswith("k_gfstack<"):
            setenv("BEATAMD_GF_KERNEL", "0")
            twin = call()
            assert ctx.last_kernel().startswith("k_gfstack<"), ctx.last_kernel()
            same = np.array_equal(out, twin)
    finally:
        ctx.close()
    return seen, same


@pytest.mark.parametrize("name", list(CASES))
def test_plan_is_the_recorded_one(monkeypatch, name):
    seen, same = _observe(name, monkeypatch.setenv)
    print("%r: %r," % (name, seen))
    assert seen == EXPECTED[name]
    assert same is not False, "the streaming kernel gives other bits"
