"""The fused Metropolis step skips the proposals that left the prior box (BEATAMD_SKIP_PARKED, default on): their chains
leave the distinct rows and, as whole wavefronts, the gather of k_gfstack_ws.  The chain states, likelihood vectors and
accept flags are bit for bit those of the step that evaluates every chain (BEATAMD_SKIP_PARKED=0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.fixture(scope="module")
def model(ctx):
    from beat_amd.synthetic import SyntheticSpec, build_problem
    spec = SyntheticSpec((20,), (20,), (1.0,), T=8, N=512, D=3, S=25, nuc_margin=0.0, time_bounds=(0.0, 0.0))
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    lay = host["layout"]
    lo, up = lay.bounds(host["lower"], host["upper"])
    return spec, host, f, lo, up


def _inputs(spec, host, f, C, n_active, seed):
    from beat_amd.synthetic import draw_population
    lay = host["layout"]
    lo, up = lay.bounds(host["lower"], host["upper"])
    rng = np.random.default_rng(seed)
    Q0 = draw_population(spec, lay, host["lower"], host["upper"], C, seed_offset=2000 + seed)
    L0 = f.batch(Q0)
    steps = []
    for _ in range(3):
        delta = rng.standard_normal((C, lay.size)) * (up - lo) * 1e-3
        out = np.ones(C, bool)
        out[rng.permutation(C)[:n_active]] = False
        delta[out] *= 1e5          # certainly outside the box: parked, rejected
        steps.append((delta, np.log(rng.random(C))))
    return Q0, L0, steps


def _run_astep(monkeypatch, f, Q0, L0, steps, lo, up, skip):
    monkeypatch.setenv("BEATAMD_SKIP_PARKED", "1" if skip else "0")
    Q, L = Q0.copy(), L0.copy()
    accs = []
    for delta, log_u in steps:
        accs.append(f.astep_batch(Q, L, delta, np.ones(Q.shape[0]), lo, up, log_u, 0.5).copy())
    return Q, L, np.array(accs)


@pytest.mark.parametrize("C,n_active", [(512, 320), (512, 0), (512, 512), (512, 1), (512, 64), (512, 65),
                                        (530, 333), (1024, 640)])
def test_astep_skip_parked_bitwise(ctx, model, monkeypatch, C, n_active):
    spec, host, f, lo, up = model
    monkeypatch.setenv("BEATAMD_GS_CG", "512")
    monkeypatch.setenv("BEATAMD_GS_WS", "1")
    Q0, L0, steps = _inputs(spec, host, f, C, n_active, seed=C + n_active)
    Qa, La, aa = _run_astep(monkeypatch, f, Q0, L0, steps, lo, up, skip=True)
    assert ctx.last_kernel().startswith("k_gfstack_ws<")
    Qb, Lb, ab = _run_astep(monkeypatch, f, Q0, L0, steps, lo, up, skip=False)
    assert np.array_equal(aa, ab)
    assert np.array_equal(Qa, Qb) and np.array_equal(La, Lb)
    if n_active == 0:
        assert not aa.any()
        assert np.array_equal(La, L0) and np.array_equal(Qa, Q0)
    if n_active >= 64:
        assert aa.any()


def test_mstep_skip_parked_bitwise(ctx, model, monkeypatch):
    """the device-drawn step (proposal kernel + forward model + accept, one call) with its counters"""
    import torch
    from beat_amd.synthetic import draw_population
    spec, host, f, lo, up = model
    monkeypatch.setenv("BEATAMD_GS_CG", "512")
    monkeypatch.setenv("BEATAMD_GS_WS", "1")
    lay = host["layout"]
    C = 512
    Q0 = draw_population(spec, lay, host["lower"], host["upper"], C, seed_offset=4000)
    L0 = f.batch(Q0)
    scales = torch.from_numpy((up - lo) * 5e-4).cuda()
    lo_d, up_d = torch.from_numpy(lo).cuda(), torch.from_numpy(up).cuda()
    ones = torch.ones(C, dtype=torch.float64, device="cuda")
    res = []
    for skip in (True, False):
        monkeypatch.setenv("BEATAMD_SKIP_PARKED", "1" if skip else "0")
        Q, L = torch.from_numpy(Q0).cuda(), torch.from_numpy(L0).cuda()
        acc = torch.zeros(C, dtype=torch.int32, device="cuda")
        acc_sum = torch.zeros(C, dtype=torch.int32, device="cuda")
        n_acc = torch.zeros(1, dtype=torch.int64, device="cuda")
        accs = []
        for step in range(4):
            f.mstep_batch(Q, L, scales, 0, 0, 91, step, 0, ones, lo_d, up_d, 0.5, acc, acc_sum, n_acc)
            accs.append(acc.cpu().numpy().copy())
        assert ctx.last_kernel().startswith("k_gfstack_ws<")
        res.append((Q.cpu().numpy(), L.cpu().numpy(), np.array(accs), acc_sum.cpu().numpy(), int(n_acc.item())))
    (Qa, La, aa, sa, na), (Qb, Lb, ab, sb, nb) = res
    assert np.array_equal(aa, ab) and np.array_equal(sa, sb) and na == nb
    assert np.array_equal(Qa, Qb) and np.array_equal(La, Lb)
    assert 0 < na < 4 * C


@pytest.mark.parametrize("skip", [True, False])
def test_all_parked_mstep_advances_step_counter(ctx, model, monkeypatch, skip):
    """every proposal outside the box (chain 0 included): nothing accepted, states untouched, and the device step
    counter the draws read still moves on once per step"""
    import torch
    from beat_amd.synthetic import draw_population
    spec, host, f, lo, up = model
    monkeypatch.setenv("BEATAMD_GS_CG", "512")
    monkeypatch.setenv("BEATAMD_GS_WS", "1")
    monkeypatch.setenv("BEATAMD_SKIP_PARKED", "1" if skip else "0")
    lay = host["layout"]
    C = 512
    Q0 = draw_population(spec, lay, host["lower"], host["upper"], C, seed_offset=5000)
    L0 = f.batch(Q0)
    scales = torch.from_numpy((up - lo) * 1e3).cuda()     # certainly outside the box
    lo_d, up_d = torch.from_numpy(lo).cuda(), torch.from_numpy(up).cuda()
    ones = torch.ones(C, dtype=torch.float64, device="cuda")
    Q, L = torch.from_numpy(Q0).cuda(), torch.from_numpy(L0).cuda()
    acc = torch.ones(C, dtype=torch.int32, device="cuda")
    n_acc = torch.zeros(1, dtype=torch.int64, device="cuda")
    counter = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    ctx.set_step_counter(counter)
    try:
        for _ in range(3):
            f.mstep_batch(Q, L, scales, 0, 0, 93, 0, 0, ones, lo_d, up_d, 0.5, acc, None, n_acc)
        ctx.synchronize()
        assert ctx.last_kernel().startswith("k_gfstack_ws<")
        assert int(counter.item()) == 10
    finally:
        ctx.set_step_counter(None)
    assert int(acc.sum().item()) == 0 and int(n_acc.item()) == 0
    assert np.array_equal(Q.cpu().numpy(), Q0) and np.array_equal(L.cpu().numpy(), L0)
