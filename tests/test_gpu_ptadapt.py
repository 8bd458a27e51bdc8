"""GPU tests of the PT proposal adaptation (csrc/ptadapt.hip and the grouped proposal entries): the streaming weighted
moments against the numpy restatement (tests/ptadapt_ref.py) and the reference's calc_sample_covariance
(tests/golden/pt_proposal.npz), the invariances of their summation order, the factor, the grouped draws and fused steps
against the ungrouped entries, and pt_sample with update_proposal end to end, on one rank and two."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import ptadapt_ref as ref
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _window_inputs(seed, n, R, G, updates, spread=5.0):
    """states: per chain a random walk (steps 0.1) around a mean of order 10; likes spread over `spread`"""
    rng = np.random.default_rng(seed)
    x = 10.0 + rng.standard_normal(n) + 0.1 * rng.standard_normal((G * R, n))
    Q = np.empty((updates, G * R, n))
    for t in range(updates):
        x = x + 0.1 * rng.standard_normal((G * R, n))
        Q[t] = x
    like = -spread * rng.uniform(size=(updates, G * R)) ** 4
    return Q, like


def _accumulate(ctx, dev, Q, like, G, host=False, splits=None):
    """reset around the first rows, then one update per Q[t] -> (state, ref) as numpy; `splits`: the groups of every call
    in separate calls on slices of the same arrays; host: numpy arrays through the same entries"""
    import torch
    n = Q.shape[2]
    R = Q.shape[1] // G
    if host:
        state, r0 = np.zeros((G, ref.stride(n))), np.zeros((G, n))
        Qd = [np.ascontiguousarray(q) for q in Q]
        Ld = [np.ascontiguousarray(l) for l in like]
    else:
        state = torch.zeros((G, ref.stride(n)), dtype=torch.float64, device=dev)
        r0 = torch.zeros((G, n), dtype=torch.float64, device=dev)
        Qd = [_t(q, dev) for q in Q]
        # like as the last column of a likelihood matrix, as the sampler hands it over
        Ld = [_t(np.stack([np.zeros_like(l), l], axis=1), dev) for l in like]
    cuts = [0, G] if not splits else np.cumsum([0] + list(splits)).tolist()
    assert cuts[-1] == G
    for a, b in zip(cuts[:-1], cuts[1:]):
        ctx.group_moments_reset(state[a:b], n, Qd[0][a * R:b * R], r0[a:b])
    for t in range(len(Qd)):
        for a, b in zip(cuts[:-1], cuts[1:]):
            if host:
                ctx.group_moments_update(state[a:b], Qd[t][a * R:b * R], Ld[t][a * R:b * R], r0[a:b])
            else:
                from beat_amd.sampler.ops import _Base
                ctx.group_moments_update(state[a:b], Qd[t][a * R:b * R], _Base(Ld[t][a * R:b * R, -1]), r0[a:b],
                                         like_stride=2)
    if host:
        return state, r0
    return state.cpu().numpy(), r0.cpu().numpy()


def _cov_of(ctx, dev, state, n):
    import torch
    st = _t(state, dev)
    F = torch.zeros((state.shape[0], n, n), dtype=torch.float64, device=dev)
    _, cov, flags = ctx.group_moments_factor(st, n, F, want_cov=True)
    return F.cpu().numpy(), cov.cpu().numpy(), flags.cpu().numpy()


def _close_states(a, b):
    """two evaluations of the same sums: header to 1e-12, S1 / S2 to 1e-12 of the group's largest entry (a sum of N terms
    of either sign is known to N 2^-53 of its largest partial sums, not of itself)"""
    assert np.array_equal(a[:, 3:5], b[:, 3:5])
    np.testing.assert_allclose(a[:, :3], b[:, :3], rtol=1e-12)
    for g in range(a.shape[0]):
        np.testing.assert_allclose(a[g, ref.HDR:], b[g, ref.HDR:], rtol=0, atol=1e-12 * np.abs(b[g, ref.HDR:]).max())


# every n, R and G of the list below appears; 1 .. 40 updates
SHAPES = [(1, 1, 1, 12), (2, 3, 3, 5), (15, 4, 1, 40), (16, 5, 3, 7), (17, 64, 1, 3), (63, 257, 1, 1), (64, 3, 32, 30),
          (65, 5, 3, 20), (130, 64, 3, 4), (130, 257, 32, 2), (17, 1, 32, 25)]


@pytest.mark.parametrize("n,R,G,updates", SHAPES)
def test_moments_match_the_restatement(ctx, dev, n, R, G, updates):
    """cov of the kernel's state within 3 (N_s + 8) 2^-53 a_i a_j (ptadapt_ref.cov_bound) of the restatement fed the same
    inputs; of 32 groups the first, one in the middle and the last are restated"""
    Q, like = _window_inputs(100 + n + R, n, R, G, updates)
    state, r0 = _accumulate(ctx, dev, Q, like, G)
    assert np.array_equal(r0, ref.group_ref(Q[0], G))
    _, cov, flags = _cov_of(ctx, dev, state, n)
    assert (state[:, 3] == updates * R).all() and (state[:, 4] == 0).all()
    # nothing above the diagonal of S2 is ever written
    S2 = state[:, ref.HDR + n:].reshape(G, n, n)
    assert (np.triu(S2, 1) == 0).all()
    worst = 0.0
    for g in sorted({0, G // 2, G - 1}):
        rows = slice(g * R, (g + 1) * R)
        st = ref.new_state(1, n)
        for t in range(updates):
            ref.update(st, Q[t, rows], like[t, rows], r0[g:g + 1])
        cov_r, fl = ref.finish(st, n)
        assert fl[0] == flags[g] == 0 or (fl[0] == 1 and flags[g] == 1)
        _close_states(state[g:g + 1], st)
        if fl[0]:
            continue
        X, lk = Q[:, rows].reshape(-1, n), like[:, rows].reshape(-1)
        frac = np.abs(cov[g] - cov_r[0]) / ref.cov_bound(X, lk, r0[g])
        assert np.array_equal(cov[g], cov[g].T)
        worst = max(worst, frac.max())
    print("n %d R %d G %d updates %d: largest |dcov| / bound = %.3g" % (n, R, G, updates, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name", ("n1", "n5", "n7", "n17", "n33"))
def test_moments_match_the_reference_fixture(ctx, dev, name):
    fix = load_golden("pt_proposal")
    steps, R = (int(v) for v in fix[name + "_shape"])
    X, like = fix[name + "_X"], fix[name + "_like"]
    n = X.shape[1]
    state, r0 = _accumulate(ctx, dev, X.reshape(steps, R, n), like.reshape(steps, R), 1)
    F, cov, flags = _cov_of(ctx, dev, state, n)
    assert flags[0] == 0
    frac = np.abs(cov[0] - fix[name + "_cov"]) / ref.cov_bound(X, like, r0[0])
    print("%s: largest |dcov| / bound = %.3g" % (name, frac.max()))
    assert frac.max() <= 1.0
    np.testing.assert_allclose(F[0].T @ F[0], cov[0], rtol=0, atol=1e-9 * np.abs(cov[0]).max())


@pytest.mark.parametrize("name", ("spike", "single"))
def test_degenerate_windows_raise_flag_one(ctx, dev, name):
    import torch
    fix = load_golden("pt_proposal")
    steps, R = (int(v) for v in fix[name + "_shape"])
    X, like = fix[name + "_X"], fix[name + "_like"]
    state, _ = _accumulate(ctx, dev, X.reshape(steps, R, 5), like.reshape(steps, R), 1)
    F = torch.full((1, 5, 5), 7.0, dtype=torch.float64, device=dev)
    _, _, flags = ctx.group_moments_factor(_t(state, dev), 5, F)
    assert int(flags[0]) == 1 and bool((F == 7.0).all())


def _hard_inputs(n, R, G, updates):
    """a window with everything in it: the maximum rises by 30 and later by 800, rows that are not finite"""
    Q, like = _window_inputs(7, n, R, G, updates)
    like[2, ::3] += 30.0
    like[4, 1::5] += 800.0
    Q[1, 2, n // 2] = np.nan
    Q[3, R + 1, 0] = np.inf
    like[5, 2 * R] = np.nan
    like[0, 3 * R + 1] = -np.inf
    return Q, like


def test_summation_order_is_the_groups_own(ctx, dev):
    """array_equal on the whole state: 32 groups in one call against calls of 1 + 7 + 24 groups, device against host
    arrays, with rescale steps (+30, +800) and skipped rows on the way; against the restatement to rounding"""
    n, R, G, updates = 65, 5, 32, 6
    Q, like = _hard_inputs(n, R, G, updates)
    whole, r0 = _accumulate(ctx, dev, Q, like, G)
    split, r1 = _accumulate(ctx, dev, Q, like, G, splits=(1, 7, 24))
    host, r2 = _accumulate(ctx, dev, Q, like, G, host=True)
    assert np.array_equal(r0, r1) and np.array_equal(r0, r2)
    assert np.array_equal(whole, split)
    assert np.array_equal(whole, host)
    # rows that are not finite are counted and add nothing
    nbad = np.zeros(G)
    nbad[[0, 1, 2, 3]] = 1
    assert np.array_equal(whole[:, 4], nbad) and np.array_equal(whole[:, 3], updates * R - nbad)
    assert np.isfinite(whole).all() and (whole[:, 0] > 790).all()
    st = ref.new_state(G, n)
    for t in range(updates):
        ref.update(st, Q[t], like[t], r0)
    _close_states(whole, st)


def test_rescale_forgets_nothing_it_should_keep(ctx, dev):
    """a maximum that rises by 30 keeps the earlier samples at weight e^-30; one that rises by 800 leaves them at 0: the
    state then is the one of the later rows alone, bit for bit"""
    n, R = 17, 4
    Q, like = _window_inputs(11, n, R, 1, 6)
    like[3:] += 800.0
    state, r0 = _accumulate(ctx, dev, Q, like, 1)
    import torch
    st = torch.zeros((1, ref.stride(n)), dtype=torch.float64, device=dev)
    ctx.group_moments_reset(st, n)
    for t in range(3, 6):
        ctx.group_moments_update(st, _t(Q[t], dev), _t(like[t], dev), _t(r0, dev))
    late = st.cpu().numpy()
    assert np.array_equal(state[0, :3], late[0, :3]) and np.array_equal(state[0, ref.HDR:], late[0, ref.HDR:])
    assert state[0, 3] == 24 and late[0, 3] == 12
    like2 = like.copy()
    like2[3:] -= 770.0                       # a rise by 30
    s30, _ = _accumulate(ctx, dev, Q, like2, 1)
    r = ref.new_state(1, n)
    for t in range(6):
        ref.update(r, Q[t], like2[t], r0)
    _close_states(s30, r)
    assert s30[0, 1] > late[0, 1]            # the early rows still count


@pytest.mark.parametrize("n", (5, 64, 65, 130))
def test_factor_and_flag_two(ctx, dev, n):
    """F^T F against numpy's Cholesky of the kernel's own cov at 1e-9 of its largest entry (test_chol_inverse_batch_kernel's
    tolerance); an indefinite group gets flag 2, keeps its factor, and the other groups of the call are factored"""
    import torch
    R, G, updates = 16, 3, (n + 15) // 16 + 2
    Q, like = _window_inputs(5, n, R, G, updates)
    state, r0 = _accumulate(ctx, dev, Q, like, G)
    F, cov, flags = _cov_of(ctx, dev, state, n)
    assert flags.tolist() == [0, 0, 0]
    for g in range(G):
        L = np.linalg.cholesky(cov[g])
        tol = 1e-9 * np.abs(cov[g]).max()
        assert np.abs(F[g].T @ F[g] - L @ L.T).max() <= tol
        assert np.abs(F[g] - L.T).max() <= 1e-9 * np.abs(L).max()
        assert (np.tril(F[g], -1) == 0).all()
    # group 1 made indefinite: the variance of its last parameter turned negative
    bad = state.copy()
    S0, S1 = bad[1, 1], bad[1, ref.HDR:ref.HDR + n]
    S2 = bad[1, ref.HDR + n:].reshape(n, n)
    S2[n - 1, n - 1] = S0 * ((S1[n - 1] / S0) ** 2 - cov[1, n - 1, n - 1])
    Fd = torch.full((G, n, n), 7.0, dtype=torch.float64, device=dev)
    _, cov2, flags2 = ctx.group_moments_factor(_t(bad, dev), n, Fd, want_cov=True)
    assert flags2.cpu().numpy().tolist() == [0, 2, 0]
    Fd = Fd.cpu().numpy()
    assert (Fd[1] == 7.0).all() and np.array_equal(Fd[0], F[0]) and np.array_equal(Fd[2], F[2])
    assert cov2.cpu().numpy()[1, n - 1, n - 1] < 0
    # host arrays: the same numbers
    Fh = np.full((G, n, n), 7.0)
    _, covh, flagsh = ctx.group_moments_factor(bad, n, Fh, want_cov=True)
    assert flagsh.tolist() == [0, 2, 0] and np.array_equal(Fh, Fd) and np.array_equal(covh, cov2.cpu().numpy())


@pytest.mark.parametrize("df", (0, 1))
@pytest.mark.parametrize("R", (1, 5, 64))
@pytest.mark.parametrize("n", (4, 64, 65, 130))
def test_grouped_draw_is_the_ungrouped_draw_per_group(ctx, dev, n, R, df):
    import torch
    G, fc = 3, 11
    rng = np.random.default_rng(n + R)
    Fs = _t(np.triu(rng.standard_normal((G, n, n))) * 0.1, dev)
    d, lu = ctx.proposal_draw_grouped(Fs[:1].repeat(G, 1, 1).contiguous(), G * R, 77, 9, first_chain=fc, df=df)
    d0, lu0 = ctx.proposal_draw(Fs[0], G * R, 77, 9, first_chain=fc, df=df)
    assert torch.equal(d, d0) and torch.equal(lu, lu0)
    d, lu = ctx.proposal_draw_grouped(Fs, G * R, 77, 9, first_chain=fc, df=df)
    for g in range(G):
        dg, lg = ctx.proposal_draw(Fs[g].contiguous(), R, 77, 9, first_chain=fc + g * R, df=df)
        assert torch.equal(d[g * R:(g + 1) * R], dg) and torch.equal(lu[g * R:(g + 1) * R], lg), g
    assert bool(torch.isfinite(d).all()) and float(d.abs().max()) > 0
    with pytest.raises(ValueError):
        ctx.proposal_draw_grouped(Fs, G * R + 1, 77, 9)


def _step_problem(ctx, dev, ndip, C):
    import torch
    from beat_amd.synthetic import SyntheticSpec, build_problem, draw_population
    spec = SyntheticSpec((ndip,), (ndip,), (1.0,), T=3, N=32, D=3, S=25)
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    lay = host["layout"]
    lo_h, up_h = lay.bounds(host["lower"], host["upper"])
    Q = _t(draw_population(spec, lay, host["lower"], host["upper"], C), dev)
    return f, Q, f.batch(Q), lo_h, up_h


@pytest.mark.parametrize("ndip,G,R", [(2, 6, 8), (4, 6, 8), (6, 6, 8), (4, 7, 10), (6, 7, 10)])
def test_grouped_fused_step(ctx, dev, ndip, G, R):
    """20 steps of mstep_batch_grouped: with equal factors bitwise mstep_batch (16 and 52 parameters: the one-launch draw, 112:
    the GEMM); with distinct factors bitwise the grouped draw + astep_batch where both go through the GEMM (more than 64
    parameters; up to 64 the fused draw is an FMA chain, test_fused_step_equals_draw_plus_astep) -- there to a tolerance
    with the chains re-joined after every step.  48 chains and a batch of 70."""
    import torch
    C = G * R
    f, Q, L, lo_h, up_h = _step_problem(ctx, dev, ndip, C)
    npar = Q.shape[1]
    assert (npar <= 64) == (ndip <= 4)
    lo, up = _t(lo_h, dev), _t(up_h, dev)
    rng = np.random.default_rng(3)
    span = up_h - lo_h
    Fs = _t(rng.standard_normal((G, npar, npar)) * 2e-3 * span[None, None, :] / np.sqrt(npar)
            * (1.0 + np.arange(G))[:, None, None] / G, dev)
    scaling = _t(0.5 + rng.random(C), dev)
    beta = _t(rng.random(C), dev)

    def fresh():
        return (Q.clone(), L.clone(), torch.zeros(C, dtype=torch.int32, device=dev),
                torch.zeros(C, dtype=torch.int32, device=dev), torch.zeros((), dtype=torch.int64, device=dev))
    # equal factors
    same = Fs[2:3].repeat(G, 1, 1).contiguous()
    QA, LA, accA, sumA, nA = fresh()
    QB, LB, accB, sumB, nB = fresh()
    for step in range(20):
        f.mstep_batch(QA, LA, Fs[2].contiguous(), None, 0, 77, step, 5, scaling, lo, up, beta, accA, sumA, nA)
        f.mstep_batch_grouped(QB, LB, same, 0, 77, step, 5, scaling, lo, up, beta, accB, sumB, nB)
    assert torch.equal(QA, QB) and torch.equal(LA, LB) and torch.equal(sumA, sumB) and int(nA) == int(nB) > 0
    # distinct factors against the pieces
    QA, LA, accA, sumA, nA = fresh()
    QB, LB, accB, sumB, nB = fresh()
    total = 0
    for step in range(20):
        delta, log_u = ctx.proposal_draw_grouped(Fs, C, 77, step, first_chain=5, df=2)
        f.astep_batch(QA, LA, delta, scaling, lo, up, log_u, beta, accA)
        f.mstep_batch_grouped(QB, LB, Fs, 2, 77, step, 5, scaling, lo, up, beta, accB, sumB, nB)
        assert torch.equal(accA, accB), step
        total += int(accA.sum())
        if npar > 64:
            assert torch.equal(QA, QB) and torch.equal(LA, LB), step
        else:
            np.testing.assert_allclose(QB.cpu().numpy(), QA.cpu().numpy(), rtol=1e-13, atol=1e-15)
            np.testing.assert_allclose(LB.cpu().numpy(), LA.cpu().numpy(), rtol=1e-9)
            QB.copy_(QA)
            LB.copy_(LA)
    assert 0 < total < 20 * C and int(nB) == total and int(sumB.sum()) == total
    with pytest.raises(ValueError):
        f.mstep_batch_grouped(QB, LB, torch.zeros((11, npar, npar), dtype=torch.float64, device=dev), 0, 77, 0, 5, scaling,
                              lo, up, beta, accB)


def _stepper(target, lo_h, up_h, C, Fs, dev):
    from beat_amd.sampler.metropolis import BatchedMetropolis
    st = BatchedMetropolis(target, lo_h, up_h, C, device=dev, tune_interval=8, seed=3, first_chain=16)
    st.set_proposal(np.diag((0.01 * (up_h - lo_h)) ** 2))
    st.set_group_proposals(Fs)
    return st


def test_grouped_steps_replay_from_a_graph(ctx, dev):
    """BatchedMetropolis with group proposals: 20 steps replayed from a captured graph (chunks of 8 around the step-size
    tuning) are bitwise the eager loop.  On the geometry-mode model, the one whose step the samplers capture: the stacking
    launch of a seismic model reads a counter of its previous launch back and is not captured, grouped or not."""
    import torch
    from beat_amd.synthetic import build_geometry_problem
    prob, lay, lower, upper = build_geometry_problem(sizes=(30, 25))
    lo_h, up_h = lay.bounds(lower, upper)
    f = prob.compile(ctx)
    G, R = 6, 8
    C, npar = G * R, lo_h.size
    rng = np.random.default_rng(4)
    Q = _t(lo_h + (up_h - lo_h) * (0.3 + 0.4 * rng.random((C, npar))), dev)
    L = f.batch(Q)
    assert hasattr(f, "mstep_batch_grouped") and bool(torch.isfinite(L[:, -1]).all())
    Fs = _t(np.triu(rng.standard_normal((G, npar, npar))) * 0.02 * (up_h - lo_h)[None, None, :]
            * (1.0 + np.arange(G))[:, None, None] / G, dev)
    beta = _t(np.repeat(1.2 ** -np.arange(G), R), dev)
    out = []
    for use_graph in (False, True):
        st = _stepper(f, lo_h, up_h, C, Fs, dev)
        q, l = Q.clone(), L.clone()
        n_acc = torch.zeros((), dtype=torch.int64, device=dev)
        st.run(q, l, beta, 20, n_acc, use_graph=use_graph)
        out.append((q, l, st.scaling.clone(), int(n_acc)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[0][2], out[1][2]) and 0 < out[0][3] == out[1][3] < 20 * C


def test_unfused_route_takes_the_group_proposals(ctx, dev):
    """a target without a fused step (what a TargetShardedLogp offers) goes through ops.draw(groups=) + astep_batch: with
    more than 64 parameters bitwise the fused grouped step, tuning included"""
    import torch
    G, R = 6, 8
    C = G * R
    f, Q, L, lo_h, up_h = _step_problem(ctx, dev, 6, C)
    npar = Q.shape[1]
    rng = np.random.default_rng(4)
    Fs = _t(rng.standard_normal((G, npar, npar)) * 2e-3 * (up_h - lo_h)[None, None, :] / np.sqrt(npar), dev)
    beta = _t(np.repeat(1.2 ** -np.arange(G), R), dev)

    class Unfused(object):
        nparams, nllk = f.nparams, f.nllk
        batch, astep_batch = f.batch, f.astep_batch
    Unfused.ctx = ctx
    out = []
    for target in (f, Unfused()):
        st = _stepper(target, lo_h, up_h, C, Fs, dev)
        q, l = Q.clone(), L.clone()
        n_acc = torch.zeros((), dtype=torch.int64, device=dev)
        st.run(q, l, beta, 20, n_acc)
        out.append((q, l, st.scaling.clone(), int(n_acc)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.equal(out[0][2], out[1][2]) and 0 < out[0][3] == out[1][3]
    st.clear_group_proposals()
    assert st.group_factors is None


def test_pt_sample_adapts_per_temperature(ctx, dev, tmp_path):
    """2 posterior + 4 tempered temperatures x 8 replicas, buffer_size 40, burnin 30: updates recorded with flags 0, the
    factors differ between temperatures, two runs agree bitwise, and two ranks sharing the GPU (three temperatures
    each) give the samples, the manager's history and the factors of one rank bit for bit"""
    import _ptadapt_gpu_worker as worker
    f, lo, up = worker.build(ctx)
    runs = [worker.run_pt(f, lo, up, dev) for _ in range(2)]
    (s, ls, man), (s2, ls2, man2) = runs
    assert np.array_equal(s, s2) and np.array_equal(ls, ls2) and man.history == man2.history
    F, F2 = man.proposal_factors.cpu().numpy(), man2.proposal_factors.cpu().numpy()
    npar = lo.size
    assert np.array_equal(F, F2) and F.shape == (6, npar, npar) and npar == 16
    steps = [st for st, _ in man.proposal_updates]
    closed, updated = ref.window_closings([man.loop_steps], 40, -1)
    assert man.windows_closed == closed and len(steps) >= 2 and set(steps) <= set(closed) and min(steps) > 30
    assert all((fl == 0).all() and fl.shape == (6,) for _, fl in man.proposal_updates)
    for a in range(6):
        for b in range(a + 1, 6):
            assert not np.array_equal(F[a], F[b]), (a, b)
    F0 = np.linalg.cholesky(np.diag((0.01 * (up - lo)) ** 2)).T
    assert all(not np.array_equal(F[g], F0) for g in range(6))
    assert s.shape == (160, npar) and np.isfinite(ls).all()
    # the default run does not go through any of it
    s0, ls0, man0 = worker.run_pt(f, lo, up, dev, update_proposal=False)
    assert man0.proposal_updates == [] and man0.proposal_factors is None and not np.array_equal(s0, s)
    # two ranks on the one GPU
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = str(tmp_path / "w2.npz")
    env.update(BEATAMD_TEST_BACKEND="gloo", BEATAMD_TEST_OUT=out, OMP_NUM_THREADS="1")
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "_ptadapt_gpu_worker.py")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("PTADAPT_GPU_WORKER_OK") == 2, r.stdout[-2000:]
    two = np.load(out)
    assert np.array_equal(two["s"], s) and np.array_equal(two["ls"], ls)
    assert np.array_equal(two["history"], np.asarray(man.history)) and float(two["scale"]) == man.current_scale
    assert np.array_equal(two["factors"].reshape(6, npar, npar), F)
    assert two["update_steps"].tolist() == steps and (two["flags"] == 0).all() and two["flags"].shape == (len(steps), 3)
