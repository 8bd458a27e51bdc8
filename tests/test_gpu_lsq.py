"""GPU tests of the least-squares start (csrc/lsq.hip): the normal equations against numpy's A^T A / A^T d of the
reference's design matrices (tests/golden/lsq.npz) and at the tile edges, batch independence, the active set against scipy's
solutions and the numpy restatement, the end-to-end solution, the start population and the samplers' ``start``."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsq_ref  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ("s2x3", "joint3x4", "ml5x7", "s1x17", "two_sub", "geo40", "zero", "positive")
_MODELS = {}


def _ctx():
    import beat_amd
    return beat_amd.get_context(0)


def _model(name):
    """the compiled model of a fixture case, built once"""
    if name not in _MODELS:
        case = lsq_ref.load_case(load_golden("lsq"), name)
        prob, lay = lsq_ref.build_problem(case)
        _MODELS[name] = (case, prob.compile(_ctx()), lay)
    return _MODELS[name]


def _slip(lay, Q, var="uparr"):
    o = lay.offsets[var]
    return Q[:, o:o + lay.varsizes[var]]


def _check_normal(name, A, d, Nm, b):
    assert np.array_equal(Nm, Nm.T), name
    refN, refb = A.T @ A, A.T @ d
    fN = np.abs(Nm - refN) / np.maximum(lsq_ref.gram_bound(A), np.finfo(float).tiny)
    fb = np.abs(b - refb) / np.maximum(lsq_ref.rhs_bound(A, d), np.finfo(float).tiny)
    assert fN.max() <= 1.0 and fb.max() <= 1.0, (name, fN.max(), fb.max())
    return float(fN.max()), float(fb.max())


# ------------------------------------------------------------------------------------------------- G1 normal equations
@pytest.mark.parametrize("name", CASES)
def test_g1_normal_equations_of_the_fixture(name):
    """entrywise within 2 (n_rows + 2) 2^-53 (|A|^T |A|)_ij of numpy's A^T A (the summation bound of both sides), likewise
    b; the matrix exactly symmetric"""
    case, f, lay = _model(name)
    Nm, b = f.lsq_normal_equations(case["Q"])
    worst = [_check_normal((name, c), case["A"][c], case["d"][c], Nm[c], b[c]) for c in range(case["Q"].shape[0])]
    print("%s: worst |difference| / bound: N %.3g, b %.3g" % (name, max(w[0] for w in worst), max(w[1] for w in worst)))


# (grid, T, N, C, interpolation): P = 1, 6, 15, 16, 17, 35, 65, 130 -- below, at and above the 16-row MFMA block and the
# 64-patch tile, up to three tiles per side; N = 1 ... 257 around the 16-sample chunk and the 64-lane stride of the
# right-hand side; C = 1, 63, 64, 65, 130
SHAPES = [((1, 1, 1.0), 2, 1, 1, "nearest_neighbor"), ((2, 3, 1.0), 2, 3, 63, "multilinear"),
          ((3, 5, 1.0), 1, 5, 64, "nearest_neighbor"), ((4, 4, 1.0), 2, 64, 65, "multilinear"),
          ((1, 17, 0.5), 2, 65, 1, "nearest_neighbor"), ((5, 7, 1.0), 1, 130, 2, "multilinear"),
          ((5, 13, 0.5), 2, 257, 3, "nearest_neighbor"), ((10, 13, 0.5), 1, 5, 130, "nearest_neighbor"),
          ((10, 13, 0.5), 2, 64, 2, "multilinear")]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "P%d_T%d_N%d_C%d_%s" % (s[0][0] * s[0][1], s[1], s[2], s[3], s[4][:2]))
def test_g1_normal_equations_at_tile_edges(shape):
    grid, T, N, C, interp = shape
    case = lsq_ref.synthetic_case(grid, T, N, interp, C, seed=100 + N + C)
    prob, lay = lsq_ref.build_problem(case)
    f = prob.compile(_ctx())
    try:
        Q = case["Q"]
        Nm, b = f.lsq_normal_equations(Q)
        case["st0"] = f.start_times(Q)          # (the sweep has its own tests)
        step = max(1, C // 5)
        for c in sorted(set(list(range(0, C, step)) + [C - 1])):
            A, d = lsq_ref.design(case, c)
            _check_normal((shape, c), A, d, Nm[c], b[c])
    finally:
        f.release()


def test_g1_batch_independence_and_device_inputs():
    """(N_c, b_c, x_c) of a chain bit for bit the same alone, inside a batch and in a permuted batch; host and device
    inputs give the same bits"""
    import torch
    for name in ("ml5x7", "joint3x4"):
        case, f, lay = _model(name)
        rng = np.random.default_rng(8)
        Q = case["lower"] + (case["upper"] - case["lower"]) * rng.random((67, case["lower"].size))
        Q[:case["Q"].shape[0]] = case["Q"]
        Nm, b = f.lsq_normal_equations(Q)
        X = f.lsq_solution(Q)
        perm = rng.permutation(Q.shape[0])
        Np, bp = f.lsq_normal_equations(np.ascontiguousarray(Q[perm]))
        Xp = f.lsq_solution(np.ascontiguousarray(Q[perm]))
        assert np.array_equal(Np, Nm[perm]) and np.array_equal(bp, b[perm]) and np.array_equal(Xp, X[perm])
        for c in (0, 1, 66):
            N1, b1 = f.lsq_normal_equations(Q[c:c + 1])
            assert np.array_equal(N1[0], Nm[c]) and np.array_equal(b1[0], b[c])
            assert np.array_equal(f.lsq_solution(Q[c:c + 1])[0], X[c])
        Qd = torch.from_numpy(Q).cuda()
        Nd, bd = f.lsq_normal_equations(Qd)
        Xd = f.lsq_solution(Qd)
        assert torch.is_tensor(Nd) and Nd.is_cuda and torch.is_tensor(Xd) and Xd.is_cuda
        assert np.array_equal(Nd.cpu().numpy(), Nm) and np.array_equal(bd.cpu().numpy(), b)
        assert np.array_equal(Xd.cpu().numpy(), X)


# ------------------------------------------------------------------------------------------------- G2 active set
def _fixture_systems():
    g = load_golden("lsq")
    out = []
    for name in CASES:
        case = lsq_ref.load_case(g, name)
        for c in range(case["Q"].shape[0]):
            A, d = case["A"][c], case["d"][c]
            out.append((name, A, d, case["m_ref"][c]))
    return out


def test_g2_nnls_batch_against_scipy_and_the_restatement():
    ctx = _ctx()
    for name, A, d, m_ref in _fixture_systems():
        Nm, b = A.T @ A, A.T @ d
        x, it, st = ctx.nnls_batch(Nm[None], b[None])
        xr, itr, str_, _ = lsq_ref.nnls_normal(Nm, b)
        assert st[0] == 0 and str_ == 0 and it[0] == itr, (name, it[0], itr)
        assert np.array_equal(x[0] != 0, m_ref != 0), name
        bound = lsq_ref.solution_bound(A, m_ref)
        assert np.abs(x[0] - m_ref).max() <= bound and np.abs(x[0] - xr).max() <= bound, name
        if name == "zero":
            assert it[0] == 0 and not x[0].any()
        if name == "positive":
            ref = np.linalg.solve(np.linalg.cholesky(Nm).T, np.linalg.solve(np.linalg.cholesky(Nm), b))
            assert (x[0] > 0).all() and np.abs(x[0] - ref).max() <= bound


def test_g2_nan_chain_is_flagged_alone_and_the_cap_is_reported(monkeypatch):
    import torch
    ctx = _ctx()
    sysm = [s for s in _fixture_systems() if s[0] == "s1x17"]
    Nm = np.stack([A.T @ A for _, A, d, _ in sysm] * 3)
    b = np.stack([A.T @ d for _, A, d, _ in sysm] * 3)
    x0, it0, st0 = ctx.nnls_batch(Nm, b)
    assert not st0.any() and np.array_equal(x0[:2], x0[2:4]) and np.array_equal(x0[:2], x0[4:])
    bad = Nm.copy()
    bad[3, 5, 2] = np.nan
    x1, it1, st1 = ctx.nnls_batch(bad, b)
    assert list(st1) == [0, 0, 0, 2, 0, 0] and np.isnan(x1[3]).all()
    keep = [0, 1, 2, 4, 5]
    assert np.array_equal(x1[keep], x0[keep]) and np.array_equal(it1[keep], it0[keep])
    # device arrays give the same bits
    xd, itd, std = ctx.nnls_batch(torch.from_numpy(Nm).cuda(), torch.from_numpy(b).cuda())
    assert np.array_equal(xd.cpu().numpy(), x0) and np.array_equal(itd.cpu().numpy(), it0)
    # the iteration cap forced small: status 1, and RuntimeError with scipy's text from the model
    monkeypatch.setenv("BEATAMD_NNLS_MAXITER", "2")
    x2, it2, st2 = ctx.nnls_batch(Nm, b)
    assert (st2 == 1).all() and (it2 == 2).all()
    case, f, lay = _model("s1x17")
    with pytest.raises(RuntimeError, match=r"^Maximum number of iterations reached\.$"):
        f.lsq_solution(case["Q"])
    monkeypatch.delenv("BEATAMD_NNLS_MAXITER")
    assert not f.lsq_solution(case["Q"], return_info=True)[2].any()


# ------------------------------------------------------------------------------------------------- G3 end to end
@pytest.mark.parametrize("name", CASES)
def test_g3_lsq_solution_end_to_end(name):
    case, f, lay = _model(name)
    Q = case["Q"]
    out, it, st = f.lsq_solution(Q, return_info=True)
    assert not st.any()
    sl, up = lay.offsets["uparr"], lay.offsets["uperp"]
    P = int(case["P"])
    rest = np.ones(Q.shape[1], dtype=bool)
    rest[sl:sl + P] = rest[up:up + P] = False
    assert np.array_equal(out[:, rest], Q[:, rest])
    assert not out[:, up:up + P].any()
    for c in range(Q.shape[0]):
        m, m_ref = out[c, sl:sl + P], case["m_ref"][c]
        assert np.array_equal(m != 0, m_ref != 0), (name, c)
        assert np.abs(m - m_ref).max() <= lsq_ref.solution_bound(case["A"][c], m_ref), (name, c)
    if name == "zero":
        assert it[0] == 0


def test_g3_flagged_chain_raises_index_error():
    case, f, lay = _model("joint3x4")
    Q = np.array(case["Q"])
    Q[1, lay.offsets["time"]] = 500.0          # start times beyond the library's axis
    bad = np.zeros(Q.shape[0], dtype=np.int32)
    with pytest.raises(IndexError):
        f.lsq_normal_equations(Q, chain_bad=bad)
    assert list(bad) == [0, 1, 0]
    with pytest.raises(IndexError):
        f.lsq_solution(Q)
    f.lsq_solution(case["Q"])                   # the status word is cleared: the next call is clean


# ------------------------------------------------------------------------------------------------- G4 start population, samplers
def _box(case):
    return case["lower"], case["upper"]


def test_g4_start_population_keeps_the_prior_draws():
    import torch
    from beat_amd.models.lsq import lsq_start_population
    from beat_amd.sampler import SMC
    case, f, lay = _model("joint3x4")
    lo, up = _box(case)
    start = lsq_start_population(f, 48, 7)
    step = SMC(f, lo, up, n_chains=48, device=torch.device("cuda", 0), random_seed=7)
    prior = step.initialize_population().cpu().numpy()
    P = int(case["P"])
    rest = np.ones(lo.size, dtype=bool)
    for v in ("uparr", "uperp"):
        rest[lay.offsets[v]:lay.offsets[v] + P] = False
    assert start.shape == prior.shape and np.array_equal(start[:, rest], prior[:, rest])
    assert not _slip(lay, start, "uperp").any() and (_slip(lay, start) >= 0).all() and _slip(lay, start).any()
    with pytest.raises(TypeError, match="Argument `start` should have dicts equal the number of chains"):
        step.initialize_population(start[:5])


def test_g4_smc_sample_from_the_lsq_start(tmp_path):
    import torch
    from beat_amd.models.lsq import lsq_start_population, prior_population
    from beat_amd.sampler import SMC, smc_sample
    case, f, lay = _model("joint3x4")
    lo, up = _box(case)
    dev = torch.device("cuda", 0)
    n = 64
    start = lsq_start_population(f, n, 11)

    def run(tag, **kw):
        step = SMC(f, lo, up, n_chains=n, device=dev, random_seed=11, tune_interval=3)
        home = str(tmp_path / tag)
        pop, lp, betas = smc_sample(3, step, max_stages=2, homepath=home, async_stage_files=False, **kw)
        z = np.load(os.path.join(home, "stage_0", "sampler_state.npz"))
        return pop, lp, betas, z["population"], z["lpoints"]

    pop_s, lp_s, betas_s, q0_s, l0_s = run("lsq", start=start)
    assert np.array_equal(q0_s, start) and np.array_equal(l0_s, f.batch(start))
    assert len(betas_s) == 4 and np.isfinite(lp_s).all()          # stage 0, two tempering stages, the final stage
    pop_r, lp_r, betas_r, q0_r, l0_r = run("random")
    assert np.array_equal(q0_r, prior_population(lo, up, n, 11))
    assert l0_s[:, -1].mean() > l0_r[:, -1].mean()
    # start=None is the run without the argument; the prior draws handed in as `start` reproduce it bit for bit
    pop_n, lp_n, betas_n, _, _ = run("none", start=None)
    pop_p, lp_p, betas_p, _, _ = run("prior", start=q0_r)
    for a, b in ((pop_n, pop_r), (lp_n, lp_r), (pop_p, pop_r), (lp_p, lp_r)):
        assert np.array_equal(a, b)
    assert betas_n == betas_r == betas_p
    with pytest.raises(TypeError, match="Argument `start` should have dicts equal the number of chains"):
        smc_sample(3, SMC(f, lo, up, n_chains=n, device=dev, random_seed=11), start=start[:-1])


def test_g4_pt_sample_from_the_lsq_start(monkeypatch):
    import torch
    from beat_amd.models.lsq import lsq_start_population
    from beat_amd.sampler import pt_sample
    from beat_amd.sampler.metropolis import BatchedMetropolis
    case, f, lay = _model("joint3x4")
    lo, up = _box(case)
    seen = []
    evaluate = BatchedMetropolis.evaluate

    def spy(self, Q):
        L = evaluate(self, Q)
        seen.append((Q.cpu().numpy().copy(), L.cpu().numpy().copy()))
        return L
    monkeypatch.setattr(BatchedMetropolis, "evaluate", spy)
    n_total = 4 * 8
    start = lsq_start_population(f, n_total, 5)
    kw = dict(n_chains_posterior=1, n_chains_tempered=3, n_replicas=8, n_samples=16, swap_interval=(2, 3),
              beta_tune_interval=2, device=torch.device("cuda", 0), random_seed=5, tune_interval=4)
    s, ls, man = pt_sample(f, lo, up, start=start, **kw)
    assert np.array_equal(seen[0][0], start) and np.array_equal(seen[0][1], f.batch(start))
    assert s.shape == (16, lo.size) and np.isfinite(ls).all()
    s0, ls0, man0 = pt_sample(f, lo, up, **kw)
    assert seen[0][1][:, -1].mean() > seen[1][1][:, -1].mean()
    with pytest.raises(TypeError, match="Argument `start` should have dicts equal the number of chains"):
        pt_sample(f, lo, up, start=start[:-1], **kw)


# ------------------------------------------------------------------------------------------------- G5 two ranks on one GPU
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(nproc, out):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(BEATAMD_TEST_OUT=out, OMP_NUM_THREADS="1")
    worker = os.path.join(ROOT, "tests", "_lsq_gpu_worker.py")
    if nproc == 1:
        cmd = [sys.executable, worker]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("LSQ_GPU_WORKER_OK") == nproc, r.stdout[-2000:]
    return np.load(out)


def test_g5_two_ranks_on_one_gpu_equal_one_rank(tmp_path):
    one = _run_ranks(1, str(tmp_path / "w1.npz"))
    two = _run_ranks(2, str(tmp_path / "w2.npz"))
    for k in ("start", "pop", "lp", "betas"):
        assert np.array_equal(one[k], two[k]), k
    assert one["start"].shape[0] == 96 and np.isfinite(one["lp"]).all()
