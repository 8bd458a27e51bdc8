"""GPU tests of the sampler kernels (csrc/smc.hip, csrc/gemm.hip) through the C ABI: SMC stage
transition against the arrays captured from the reference's methods (tests/golden/smc.npz), the
proposal generator against its Python twin (tests/philox_ref.py, pinned to the published Philox
known answers on the CPU), the FP64 MFMA GEMM against numpy, and the failure behaviour the
advisor asked for (chain-local NaN for an index outside the GF library, weight-update
validation)."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


# ----------------------------------------------------------------------------- stage transition
def test_calc_beta_resample_factor_vs_reference_golden(ctx):
    """beatamd_smc_calc_beta / _smc_resample / _smc_population_factor against SMC.calc_beta,
    SMC.resample and np.cov(aweights) of the reference (smc.py:133-186, 290-324)"""
    import torch
    g = load_golden("smc")
    dev = torch.device("cuda", 0)
    for k in range(int(g["ncase"])):
        lk = np.ascontiguousarray(g["c%d_lk" % k])
        beta_in = float(g["c%d_beta_in" % k])
        b, w = ctx.smc_calc_beta(lk, beta_in, 1.0)
        # the bisection takes exactly the reference's decisions: same dyadic beta
        assert b == float(g["c%d_beta" % k])
        # exp() of the device vs numpy's: <= 1 ulp per term -> 1e-14 relative on the weights
        np.testing.assert_allclose(w, g["c%d_w" % k], rtol=1e-13, atol=0)
        assert abs(w.sum() - 1.0) < 1e-13
        # strided view: the `like` column of a likelihood matrix on the device
        L = torch.zeros((lk.size, 5), dtype=torch.float64, device=dev)
        L[:, -1] = torch.from_numpy(lk).to(dev)
        from beat_amd.sampler.ops import DeviceOps
        ops = DeviceOps(ctx)
        b2, w2 = ops.calc_beta(L[:, -1], beta_in, 1.0)
        assert b2 == b and np.array_equal(w2.cpu().numpy(), w)
        # resampling: sequential cumulative sum like np.cumsum -> bit-exact indices
        aux = float(np.ravel(g["c%d_aux" % k])[0])
        idx = ctx.smc_resample(np.ascontiguousarray(g["c%d_w" % k]), aux)
        assert idx.dtype == np.int32 and np.array_equal(idx, g["c%d_idx" % k])
        # proposal factor: F^T F = np.cov(population, aweights=weights, bias=False)
        F = ctx.smc_population_factor(np.ascontiguousarray(g["c%d_pop" % k]),
                                      np.ascontiguousarray(g["c%d_w" % k]))
        np.testing.assert_allclose(F.T @ F, g["c%d_cov" % k], rtol=1e-11, atol=1e-14)
        # final-stage weights (smc.py:526-529)
        wf = ctx.smc_stage_weights(lk, 1.0 - beta_in)
        t = np.exp((1.0 - beta_in) * (lk - lk.max()))
        np.testing.assert_allclose(wf, t / t.sum(), rtol=1e-13)


def test_stage_ops_large_population_vs_host_ops(ctx):
    """4096 and 10007 chains (BASELINE configs[3] population; an odd size): device vs host ops"""
    import torch
    from beat_amd.sampler.ops import DeviceOps, HostOps
    dops, hops = DeviceOps(ctx), HostOps()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4)
    for n in (4096, 10007):
        lk = torch.from_numpy(-1e4 * rng.random(n) ** 2)
        for beta in (0.0, 3e-4):
            bh, wh = hops.calc_beta(lk, beta, 1.0)
            bd, wd = dops.calc_beta(lk.to(dev), beta, 1.0)
            assert bd == bh
            np.testing.assert_allclose(wd.cpu().numpy(), wh.numpy(), rtol=1e-12, atol=1e-300)
            for aux in (0.0, 0.37, 0.999999):
                ih = hops.resample(wh, aux).numpy()
                idd = dops.resample(wh.to(dev), aux).cpu().numpy()
                assert np.array_equal(idd, ih)
        X = torch.from_numpy(rng.standard_normal((n, 37)))
        Fh = hops.population_factor(X, wh).numpy()
        Fd = dops.population_factor(X.to(dev), wh.to(dev)).cpu().numpy()
        if Fd.shape == Fh.shape:
            np.testing.assert_allclose(Fd, Fh, rtol=1e-10, atol=1e-13)
        else:   # many more chains than parameters: the compact Cholesky form of the same covariance
            assert Fd.shape == (37, 37)
            np.testing.assert_allclose(Fd.T @ Fd, Fh.T @ Fh, rtol=1e-9, atol=1e-12)
        sel = torch.from_numpy(rng.integers(0, n, 100).astype(np.int32))
        assert torch.equal(dops.gather(X.to(dev), sel.to(dev)).cpu(), X[sel.long()])
    ctx.synchronize()


def test_gather_rows_out_of_range_index_raises(ctx):
    X = np.arange(12.0).reshape(4, 3)
    np.testing.assert_array_equal(ctx.gather_rows(X, np.array([3, 0, 0], dtype=np.int32)), X[[3, 0, 0]])
    with pytest.raises(IndexError):
        ctx.gather_rows(X, np.array([1, 4], dtype=np.int32))


def test_metropolis_tune_kernel_is_pymc_table(ctx):
    import torch
    from beat_amd.sampler import step_tune
    dev = torch.device("cuda", 0)
    acc = np.array([0, 1, 4, 5, 19, 20, 21, 50, 51, 75, 76, 95, 96, 100], dtype=np.int32)
    sc = np.linspace(0.5, 2.0, acc.size)
    s_d, a_d = torch.from_numpy(sc.copy()).to(dev), torch.from_numpy(acc.copy()).to(dev)
    ctx.metropolis_tune(s_d, a_d, 100)
    np.testing.assert_array_equal(s_d.cpu().numpy(), step_tune(sc, acc / 100.0))
    assert int(a_d.abs().sum().item()) == 0


# ----------------------------------------------------------------------------- proposal rows
def test_proposal_normals_match_philox_reference(ctx):
    """z from the device generator = the Python Philox4x32-10 + Box-Muller twin; draws are a
    function of (seed, step, global chain) only"""
    import philox_ref as pr
    for K in (16, 7, 1):
        C = 33
        eye = np.eye(K)
        z, lu = ctx.proposal_draw(eye, C, seed=0x123456789abcdef, step=5)
        ref = pr.normals(C, K, 0x123456789abcdef, 5)
        np.testing.assert_allclose(z, ref, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(lu, pr.log_uniforms(C, 0x123456789abcdef, 5), rtol=1e-13)
        # sharding independence: chains 10..32 drawn as a block of their own
        z2, lu2 = ctx.proposal_draw(eye, C - 10, seed=0x123456789abcdef, step=5, first_chain=10)
        assert np.array_equal(z2, z[10:]) and np.array_equal(lu2, lu[10:])
        z3, _ = ctx.proposal_draw(eye, C, seed=0x123456789abcdef, step=6)
        assert not np.array_equal(z3, z)
    # multivariate t: rows divided by sqrt(chi2(df)/df)
    for df in (1, 2, 5):
        zc, _ = ctx.proposal_draw(np.eye(4), 50, seed=9, step=2, df=df)
        ref = pr.normals(50, 4, 9, 2) * pr.t_row_scale(50, 9, 2, df)[:, None]
        np.testing.assert_allclose(zc, ref, rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("C,K,npar", [(5, 3, 2), (130, 70, 200), (512, 512, 1204), (64, 1204, 1204)])
def test_proposal_gemm_vs_numpy(ctx, C, K, npar):
    """delta = z . F on the FP64 matrix cores (A = I check with an asymmetric factor included)"""
    import philox_ref as pr
    rng = np.random.default_rng(C + K)
    F = rng.standard_normal((K, npar)) * (1.0 + np.arange(npar))[None, :]   # asymmetric
    delta, _ = ctx.proposal_draw(F, C, seed=77, step=1)
    ref = pr.normals(C, K, 77, 1) @ F
    np.testing.assert_allclose(delta, ref, rtol=1e-11, atol=1e-9 * np.abs(ref).max())


def test_proposal_statistics_on_device(ctx):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    A = rng.standard_normal((4, 4))
    cov = A @ A.T + 0.5 * np.eye(4)
    from beat_amd.sampler.base import covariance_factor
    F = torch.from_numpy(covariance_factor(cov)).to(dev)
    x, lu = ctx.proposal_draw(F, 400000, seed=5, step=0)
    np.testing.assert_allclose(np.cov(x.cpu().numpy().T), cov, rtol=0.02, atol=0.02)
    u = np.exp(lu.cpu().numpy())
    assert abs(u.mean() - 0.5) < 0.003 and abs(u.var() - 1.0 / 12) < 0.002
    y, _ = ctx.proposal_draw(F, 400000, seed=6, step=0, df=1)
    y = y.cpu().numpy()
    np.testing.assert_allclose(np.median(np.abs(y), axis=0), np.sqrt(np.diag(cov)), rtol=0.02)


# ----------------------------------------------------------------------------- whitening GEMM
@pytest.mark.parametrize("R,N", [(1, 6), (300, 130), (1000, 512), (70, 1000)])
def test_whiten_rows_vs_numpy(ctx, R, N):
    """rows <- rows . W^T (beatamd_whiten_rows) for upper-triangular (chol_inverse) and full W"""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(R + N)
    rows = rng.standard_normal((R, N))
    for upper in (True, False):
        W = rng.standard_normal((N, N)) + 3.0 * np.eye(N)
        if upper:
            W = np.triu(W)
        d = torch.from_numpy(rows.copy()).to(dev)
        ctx.whiten_rows(d, W)
        ref = rows @ W.T
        np.testing.assert_allclose(d.cpu().numpy(), ref, rtol=1e-11, atol=1e-11 * np.abs(ref).max())


@pytest.mark.parametrize("B,R,N", [(1, 1, 6), (3, 300, 130), (2, 1000, 512), (5, 70, 1000), (4, 129, 257)])
def test_whiten_rows_batch_in_place_vs_numpy(ctx, B, R, N):
    """beatamd_whiten_rows_batch: rows[b] <- rows[b] . W[b]^T for all datasets of a wavemap in one call.  Upper
    triangular operators (chol_inverse) run IN PLACE column block by column block (ascending: a product column n needs
    the row's entries k >= n only -- sizes around the 64-row / 128-column tiles and the 16-wide k steps); one full
    operator in the batch sends the call through the buffered per-dataset route; host and device operators"""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(B + R + N)
    rows = rng.standard_normal((B, R, N))
    for upper in (True, False):
        W = rng.standard_normal((B, N, N)) + 3.0 * np.eye(N)
        if upper:
            W = np.triu(W)
        else:
            W[:B - 1] = np.triu(W[:B - 1])       # only the last operator is full
        ref = np.einsum("brk,bnk->brn", rows, W)
        for on_device in (False, True):
            d = torch.from_numpy(rows.copy()).to(dev)
            ctx.whiten_rows_batch(d, torch.from_numpy(W).to(dev) if on_device else W)
            np.testing.assert_allclose(d.cpu().numpy(), ref, rtol=1e-11, atol=1e-11 * np.abs(ref).max())
    with pytest.raises(ValueError):
        ctx.whiten_rows_batch(torch.zeros((2, 3, 8), dtype=torch.float64, device=dev), np.zeros((3, 8, 8)))


@pytest.mark.parametrize("B,N", [(1, 1), (3, 63), (2, 64), (4, 100), (5, 513), (2, 4096)])
def test_unwhiten_traces_vs_numpy(ctx, B, N):
    """beatamd_unwhiten_traces: X[t] <- inv(W[t]) . X[t] by back substitution (the residuals of a pre-whitened model are
    W_old (d - s), the covariance update wants d - s): sizes around the 64-row blocks, host and device arrays, against
    numpy's solve; a zero on the diagonal is a LinAlgError."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7 * B + N)
    W = np.triu(rng.standard_normal((B, N, N)) / np.sqrt(N)) + 2.0 * np.eye(N)
    x = rng.standard_normal((B, N))
    ref = np.stack([np.linalg.solve(W[b], x[b]) for b in range(B)])
    tol = dict(rtol=1e-10, atol=1e-11 * np.abs(ref).max())
    h = x.copy()
    ctx.unwhiten_traces(W, h)
    np.testing.assert_allclose(h, ref, **tol)
    d = torch.from_numpy(x.copy()).to(dev)
    ctx.unwhiten_traces(torch.from_numpy(W).to(dev), d)
    np.testing.assert_allclose(d.cpu().numpy(), ref, **tol)
    # back through the whitening product: W . inv(W) x = x
    np.testing.assert_allclose(np.einsum("bij,bj->bi", W, h), x, rtol=1e-9, atol=1e-10)
    if N > 1:
        Ws = W.copy()
        Ws[B - 1, N // 2, N // 2] = 0.0
        with pytest.raises(np.linalg.LinAlgError):
            ctx.unwhiten_traces(Ws, x.copy())
    with pytest.raises(ValueError):
        ctx.unwhiten_traces(W, np.zeros((B, N + 1)))


# ----------------------------------------------------------------------------- failure behaviour
def _small_model(ctx, **kw):
    from beat_amd.synthetic import SyntheticSpec, build_problem, draw_population
    spec = SyntheticSpec((4,), (4,), (1.0,), T=3, N=32, D=3, S=25, **kw)
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    lay = host["layout"]
    Q = draw_population(spec, lay, host["lower"], host["upper"], 70)
    return spec, prob, host, f, lay, Q


def test_index_outside_library_is_chain_local_nan_on_device(ctx):
    """An origin time that pushes the start times off the library grid: the reference raises
    IndexError (numpy fancy indexing).  Host arrays -> IndexError; device tensors (asynchronous)
    -> that chain's like is NaN, the others are untouched, the Metropolis step rejects it, and the
    next synchronisation raises IndexError."""
    import torch
    spec, prob, host, f, lay, Q = _small_model(ctx)
    dev = torch.device("cuda", 0)
    good = f.batch(Q)
    bad = Q.copy()
    bad[[3, 64], lay.offset("time")] = 100.0
    with pytest.raises(IndexError):
        f.batch(bad)
    Ld = f.batch(torch.from_numpy(bad).to(dev)).cpu().numpy()
    assert np.isnan(Ld[[3, 64], -1]).all()
    keep = np.setdiff1d(np.arange(70), [3, 64])
    np.testing.assert_array_equal(Ld[keep], good[keep])
    with pytest.raises(IndexError):
        ctx.synchronize()
    ctx.synchronize()  # the status word was cleared
    # astep: chain 0 proposes the off-grid origin time inside a (deliberately wide) prior box
    lo, up = lay.bounds(host["lower"], host["upper"])
    up = up.copy()
    up[lay.offset("time")] = 1000.0
    Q0 = torch.from_numpy(Q).to(dev)
    L0 = torch.from_numpy(good).to(dev)
    delta = torch.zeros_like(Q0)
    delta[0, lay.offset("time")] = 100.0
    acc = f.astep_batch(Q0, L0, delta, torch.ones(70, dtype=torch.float64, device=dev),
                        torch.from_numpy(lo).to(dev), torch.from_numpy(up).to(dev),
                        torch.full((70,), -1e300, dtype=torch.float64, device=dev), 1.0)
    acc = acc.cpu().numpy()
    assert acc[0] == 0 and acc[1:].all()          # zero moves are accepted (mr = 0 > log u)
    assert torch.equal(Q0.cpu(), torch.from_numpy(Q))
    with pytest.raises(IndexError):
        ctx.synchronize()


def test_update_weights_validation(ctx):
    """a dense update of a pre-whitened (scalar) weight set was silently accepted"""
    from beat_amd.synthetic import SyntheticSpec, build_problem
    spec = SyntheticSpec((4,), (4,), (1.0,), T=3, N=32, D=3, S=25, covariance="toeplitz")
    prob, host = build_problem(spec)
    W, sl = np.asarray(host["weights"]), np.asarray(host["slog"])
    f = prob.compile(ctx)
    f.update_weights(0, 2.0 * W, sl + 1.0)                  # same kind and size: fine
    with pytest.raises(ValueError):
        f.update_weights(0, W[:, :16, :16], sl)             # wrong size
    with pytest.raises(ValueError):
        ctx.weights_update(prob.wavemaps[0]._wset, np.ones(3), sl)   # scalar into a dense set
    prob2, _ = build_problem(spec)
    f2 = prob2.compile(ctx, prewhiten=True)
    with pytest.raises(ValueError):
        f2.update_weights(0, np.ones(3), sl)                # a pre-whitened wavemap takes dense operators
    with pytest.raises(ValueError):
        ctx.weights_update(prob2.wavemaps[0]._wset, W, sl)  # the library refuses a dense set for a scalar one


@pytest.mark.parametrize("K,n", [(40, 7), (1024, 12), (700, 130), (300, 200)])
def test_compact_proposal_factor(ctx, K, n):
    """R (n, n) upper triangular with R^T R = F^T F for a tall population factor (Gram matrix and
    blocked Cholesky on the device); DeviceOps uses it when chains >= 2 x parameters; a collapsed
    population (singular Gram matrix) keeps the tall factor"""
    import torch
    from beat_amd.sampler.ops import DeviceOps
    rng = np.random.default_rng(K + n)
    X = rng.standard_normal((K, n)) * (1.0 + np.arange(n))[None, :] + rng.standard_normal(n)
    w = rng.random(K)
    dev = torch.device("cuda", 0)
    F = ctx.smc_population_factor(torch.from_numpy(X).to(dev), torch.from_numpy(w).to(dev))
    R = ctx.factor_compact(F)
    cov = np.cov(X, aweights=w, bias=False, rowvar=0)
    Rn = R.cpu().numpy()
    assert np.array_equal(np.tril(Rn, -1), np.zeros((n, n))) and (np.diag(Rn) > 0).all()
    np.testing.assert_allclose(Rn.T @ Rn, cov, rtol=1e-10, atol=1e-12 * np.abs(cov).max())
    np.testing.assert_allclose(Rn, np.linalg.cholesky(cov).T, rtol=1e-8, atol=1e-10 * np.abs(Rn).max())
    ops = DeviceOps(ctx)
    P = ops.population_factor(torch.from_numpy(X).to(dev), torch.from_numpy(w).to(dev))
    assert tuple(P.shape) == ((n, n) if K >= 2 * n else (K, n))
    Pn = P.cpu().numpy()
    np.testing.assert_allclose(Pn.T @ Pn, cov, rtol=1e-10, atol=1e-12 * np.abs(cov).max())
    # collapsed population: two distinct points only -> rank 1 -> the tall factor stays
    Xc = np.repeat(X[:2], K // 2, axis=0)
    Pc = ops.population_factor(torch.from_numpy(Xc).to(dev), torch.from_numpy(np.ones(len(Xc))).to(dev))
    assert tuple(Pc.shape) == ((len(Xc), n) if n > 1 else (n, n))
    Pcn = Pc.cpu().numpy()
    np.testing.assert_allclose(Pcn.T @ Pcn, np.cov(Xc, rowvar=0), rtol=1e-9, atol=1e-9 * np.abs(cov).max())


@pytest.mark.parametrize("n", [5, 64, 100, 150, 200, 330])
def test_whitening_ratio_kernel(ctx, n):
    """M = W_new . inv(W_old) for upper-triangular whitening operators (blocked right-side triangular
    solve on the FP64 matrix cores, block columns in pairs: 1, 2, 3, 4 and 6 block columns) against numpy"""
    rng = np.random.default_rng(n)
    t = np.arange(n)
    def op(scale, corr):
        Cm = scale * np.exp(-np.abs(t[:, None] - t[None, :]) / corr) + 1e-3 * np.eye(n)
        return np.linalg.cholesky(np.linalg.inv(Cm)).T
    off = 1.0 if n <= 200 else 0.2      # (a random triangular matrix with unit entries is ill-conditioned beyond that)
    Wo = np.stack([op(0.7, 5.0), op(1.3, 2.0), off * np.triu(rng.standard_normal((n, n))) + 4.0 * np.eye(n)])
    Wn = np.stack([op(0.9, 4.0), op(0.4, 7.0), off * np.triu(rng.standard_normal((n, n))) + 3.0 * np.eye(n)])
    M = ctx.whitening_ratio_batch(Wn, Wo)
    for i in range(3):
        ref = Wn[i] @ np.linalg.inv(Wo[i])
        assert np.array_equal(np.tril(M[i], -1), np.zeros((n, n)))
        np.testing.assert_allclose(M[i], ref, rtol=0, atol=1e-10 * np.abs(ref).max())
        np.testing.assert_allclose(M[i] @ Wo[i], Wn[i], rtol=0, atol=1e-11 * np.abs(Wn[i]).max())
    bad = Wo.copy()
    bad[1, n // 2, n // 2] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        ctx.whitening_ratio_batch(Wn, bad)


@pytest.mark.parametrize("name", ["seis_dense_ml_shifts", "joint_multifault"])
def test_update_weights_on_prewhitened_library(ctx, name):
    """SURVEY 8(f) row 2, "re-whiten on update_weights": a wavemap compiled with a pre-whitened
    library follows a covariance update in place (rows and data times M = W_new . inv(W_old)) and
    gives the likelihoods of a model built with the new weights from scratch; twice in a row"""
    from test_gpu_parity import _specs
    from beat_amd.heart import chol_inverse_batch
    from beat_amd.synthetic import build_problem, draw_population
    spec = _specs()[name]
    prob, host = build_problem(spec)
    fp = prob.compile(ctx, prewhiten=True)
    probd, _ = build_problem(spec)
    fd = probd.compile(ctx)                                  # dense-weight twin
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], 70)
    np.testing.assert_allclose(fp.batch(Q), fd.batch(Q), rtol=1e-9, atol=1e-7)
    T, N = prob.wavemaps[0].data.shape
    t = np.arange(N)
    rng = np.random.default_rng(3)
    for rep in range(2):
        covs = np.stack([rng.uniform(0.2, 2.0) * np.exp(-np.abs(t[:, None] - t[None, :]) / rng.uniform(1.0, 6.0))
                         + 1e-3 * np.eye(N) for _ in range(T)])
        W, sl = chol_inverse_batch(covs)
        fp.update_weights(0, W, sl)
        fd.update_weights(0, W, sl)
        np.testing.assert_allclose(fp.batch(Q), fd.batch(Q), rtol=1e-9, atol=1e-7)


# ----------------------------------------------------------------------------- seams
def test_logp_forw_func_returns_unobserved_rvs(ctx):
    """B1: with return_rvs the compiled-function twin lists the free variables in q order in
    front of the deterministics, like model.unobserved_RVs (sampler/base.py:598-615)"""
    from beat_amd.synthetic import SyntheticSpec, build_problem, draw_population
    spec = SyntheticSpec((4,), (4,), (1.0,), T=2, N=16, D=3, S=25, geodetic_nobs=(6,), laplacian=True)
    prob, host = build_problem(spec)
    f = prob.compile(ctx, return_rvs=True)
    lay = host["layout"]
    q = draw_population(spec, lay, host["lower"], host["upper"], 1)[0]
    out = f(q)
    names = f.out_names
    assert names[:len(lay.varsizes)] == list(lay.varsizes) and names[-1] == "like"
    assert len(out) == len(names) and f._llk_index == len(out) - 1
    for (k, n), v in zip(lay.varsizes.items(), out):
        assert v.shape == (n,) and np.array_equal(v, q[lay.offset(k):lay.offset(k) + n])
    ll = f.batch(q[None])[0]
    assert out[f._llk_index] == ll[-1]
    assert out[-4].shape == (2,) and out[-3].shape == (1,) and out[-2].shape == ()
    f0 = prob.compile(ctx)
    assert len(f0(q)) == 4 and f0._llk_index == 3
    shared = {s.name: s for s in f.get_shared()}
    assert "geodetic_data" in shared and np.array_equal(shared["geodetic_data"].get_value(), host["gdata"])


def test_stack_all_patch_subset_and_modes(ctx):
    """B3: patchidxs subsets (base.py:651-656) and the reference's stack-mode names"""
    from beat_amd.ffi import SeismicGFLibrary, SeismicGFLibraryConfig
    from oracle import oracle as orc
    rng = np.random.default_rng(8)
    T, P, D, S, N = 3, 9, 2, 5, 40
    G = rng.standard_normal((T, P, D, S, N))
    gf = SeismicGFLibrary(SeismicGFLibraryConfig(dimensions=(T, P, D, S, N), starttime_sampling=0.5,
                                                 duration_sampling=0.5, starttime_min=0.0, duration_min=0.5))
    gf.setup(T, P, D, S, N, allocate=True)
    gf._gfmatrix[:] = G
    gf.init_optimization(ctx)
    for mode in ("numpy", "pytensor", "hip"):
        gf.set_stack_mode(mode)
    pidx = np.array([7, 2, 4], dtype="int16")
    dur, sl = rng.uniform(0.5, 1.0, 3), rng.uniform(0, 5, 3)
    st = rng.uniform(0, 2, (T, 3))
    for interp in ("nearest_neighbor", "multilinear"):
        out = gf.stack_all(dur, st, sl, targetidxs=np.arange(T)[:, None], patchidxs=pidx, interpolation=interp)
        ref = orc.stack_all(np.ascontiguousarray(G[:, pidx]), dur, st, sl, 0.5, 0.5, 0.0, 0.5, interp)
        np.testing.assert_allclose(out, ref, rtol=1e-12, atol=1e-12)
    # target subset
    out = gf.stack_all(dur, st[[2, 0]], sl, targetidxs=np.array([[2], [0]]), patchidxs=pidx)
    np.testing.assert_allclose(out, ref_nn(G, pidx, dur, st, sl, orc)[[2, 0]], rtol=1e-12, atol=1e-12)
    with pytest.raises(IndexError):
        gf.stack_all(dur, st, sl, targetidxs=np.arange(T), patchidxs=np.array([1, 1, 2]))


def ref_nn(G, pidx, dur, st, sl, orc):
    return orc.stack_all(np.ascontiguousarray(G[:, pidx]), dur, st, sl, 0.5, 0.5, 0.0, 0.5)


def test_library_files_round_trip_through_hbm(ctx, tmp_path):
    """f.2: <name>.traces.npy / .times.npy / .yaml (base.py:161-189, 364-373): save from a host
    library and from an HBM-only library, load memory-mapped, stream to HBM, same stacks"""
    import torch
    from beat_amd.ffi import SeismicGFLibrary, SeismicGFLibraryConfig, load_gf_library
    rng = np.random.default_rng(2)
    T, P, D, S, N = 4, 6, 2, 7, 64
    cfg = dict(dimensions=(T, P, D, S, N), starttime_sampling=0.25, duration_sampling=0.5,
               starttime_min=-0.5, duration_min=0.5, component="uperp", mapnumber=3, wavename="any_S")
    gf = SeismicGFLibrary(SeismicGFLibraryConfig(**cfg))
    gf.setup(T, P, D, S, N, allocate=True)
    gf._gfmatrix[:] = rng.standard_normal((T, P, D, S, N))
    for t in range(T):
        gf.set_patch_time(t, 10.0 + t)
    C = 50
    dur, st, sl = rng.uniform(0.5, 1.0, (C, P)), rng.uniform(-0.5, 1.0, (C, T, P)), rng.uniform(0, 5, (C, P))
    gf.init_optimization(ctx)
    before = gf.stack_all_batch(dur, st, sl, interpolation="multilinear")
    gf.save(str(tmp_path))
    g2 = load_gf_library(str(tmp_path), gf.filename)
    assert isinstance(g2._gfmatrix, np.memmap) and g2.filename == "seismic_uperp_any_S_3_0"
    assert g2.starttime_min == -0.5 and g2.starttime_sampling == 0.25 and g2.dimensions == (T, P, D, S, N)
    np.testing.assert_array_equal(g2._tmins, 10.0 + np.arange(T))
    g2.init_optimization(ctx)
    assert np.array_equal(g2.stack_all_batch(dur, st, sl, interpolation="multilinear"), before)
    # a library that exists only in HBM
    g3 = SeismicGFLibrary(SeismicGFLibraryConfig(**dict(cfg, component="uparr")))
    g3.adopt_device_tensor(torch.from_numpy(gf._gfmatrix).to("cuda:0"))
    g3.save(str(tmp_path))
    g4 = load_gf_library(str(tmp_path), g3.filename)
    np.testing.assert_array_equal(np.asarray(g4._gfmatrix), gf._gfmatrix)
    g4.init_optimization(ctx)
    assert np.array_equal(g4.stack_all_batch(dur, st, sl, interpolation="multilinear"), before)


# ----------------------------------------------------------------------------- multi-GPU readiness
def test_bench_two_ranks_over_rccl():
    """bench.py --gpus 2 --full under torchrun (one rank per GPU, RCCL): skipped on 1-GPU boxes.  Checks
    the line's contract fields and that the stage transition ran over both ranks."""
    import json
    import os
    import subprocess
    import sys

    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs, found %d" % torch.cuda.device_count())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29577", os.path.join(root, "bench.py"),
           "--gpus", "2", "--steps", "3", "--warmup", "1", "--chains", "64", "--full", "--no-cpu-baseline",
           "--targets", "4", "--samples", "256"]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["global_chains"] == 128
    assert d["stage_transition_ms"] > 0 and d["value"] > 0


def test_degenerate_weights_raise_on_device(ctx):
    """one dominant importance weight makes the weighted sample covariance 0/0;
    k_pop_factor raises the status word and the stage transition raises the reference's ValueError
    (smc.py:181-185) instead of sampling a stage with a NaN proposal factor"""
    import torch
    from beat_amd.sampler.ops import DeviceOps
    ops = DeviceOps(ctx)
    dev = torch.device("cuda", 0)
    X = torch.randn((300, 7), dtype=torch.float64, device=dev)
    w = torch.zeros(300, dtype=torch.float64, device=dev)
    w[11] = 1.0
    with pytest.raises(ValueError, match="Sample covariances contains Inf or NaN"):
        ops.population_factor(X, w)
    w = torch.full((300,), 1.0 / 300, dtype=torch.float64, device=dev)
    F = ops.population_factor(X, w)          # the status word was cleared: a healthy population works
    assert torch.isfinite(F).all()
    X[5, 2] = float("nan")
    with pytest.raises(ValueError, match="Sample covariances contains Inf or NaN"):
        ops.population_factor(X, w)


def test_univariate_proposals_match_philox_reference_and_their_laws(ctx):
    """beatamd_proposal_draw_univariate (NormalProposal / CauchyProposal / LaplaceProposal,
    beat/sampler/base.py:129-147): every draw equals the Python Philox twin, draws depend on (seed,
    step, global chain) only, and 2e5 draws follow the laws (quartiles; variance where it exists)"""
    import philox_ref as pr
    seed = 0xfeedface12345
    for kind in (0, 1, 2):
        for npar in (7, 16, 1):
            C = 29
            scale = np.linspace(0.5, 2.0, npar)
            d, lu = ctx.proposal_draw_univariate(kind, scale, C, seed=seed, step=3)
            ref = pr.univariate(C, npar, kind, scale, seed, 3)
            np.testing.assert_allclose(d, ref, rtol=1e-10, atol=1e-13)    # (tan near +-pi/2: device vs libm)
            np.testing.assert_allclose(lu, pr.log_uniforms(C, seed, 3), rtol=1e-13)
            d2, lu2 = ctx.proposal_draw_univariate(kind, scale, C - 9, seed=seed, step=3, first_chain=9)
            assert np.array_equal(d2, d[9:]) and np.array_equal(lu2, lu[9:])
        x, _ = ctx.proposal_draw_univariate(kind, np.ones(100), 2000, seed=11 + kind, step=0)
        x = np.asarray(x).ravel()
        q1, q2, q3 = np.quantile(x, [0.25, 0.5, 0.75])
        want_q3 = {0: 0.6744897501960817, 1: 1.0, 2: np.log(2.0)}[kind]
        assert abs(q2) < 0.01 and abs(q3 - want_q3) < 0.02 and abs(q1 + want_q3) < 0.02, (kind, q1, q2, q3)
        if kind != 1:
            assert abs(x.var() - {0: 1.0, 2: 2.0}[kind]) < 0.03, (kind, x.var())
    # PoissonProposal (base.py:150-155): poisson(lam = scale) - scale; exact twin, then the law (mean 0, variance lam,
    # integer steps, pmf of the smallest counts)
    for npar in (7, 2):
        lam = np.linspace(0.3, 40.0, npar)
        d, _ = ctx.proposal_draw_univariate(3, lam, 29, seed=seed, step=5)
        assert np.array_equal(d, pr.univariate(29, npar, 3, lam, seed, 5))
    lam = np.array([0.7, 3.0, 25.0, 400.0])
    x, _ = ctx.proposal_draw_univariate(3, lam, 200000, seed=5, step=1)
    x = np.asarray(x)
    k = x + lam
    assert np.array_equal(k, np.rint(k)) and k.min() >= 0
    assert np.all(np.abs(x.mean(0)) < 4.0 * np.sqrt(lam / 200000.0))
    np.testing.assert_allclose(x.var(0), lam, rtol=0.02)
    np.testing.assert_allclose((k[:, 0] == 0).mean(), np.exp(-0.7), atol=4e-3)
    np.testing.assert_allclose((k[:, 1] == 2).mean(), np.exp(-3.0) * 4.5, atol=4e-3)
    with pytest.raises(ValueError):
        ctx.proposal_draw_univariate(4, np.ones(4), 5, seed=1, step=0)
    # a Poisson step width beyond 500 (or NaN) handed to the C entry point directly: flagged on the device, raised at the
    # next synchronisation -- never silent NaN rows
    with pytest.raises(ValueError):
        ctx.proposal_draw_univariate(3, np.array([3.0, 600.0]), 8, seed=1, step=0)
        ctx.synchronize()
    ctx.synchronize()       # (the status word is cleared by the raise)


def test_metropolis_with_per_parameter_proposal_on_device(ctx):
    """BEAT configures Metropolis-style runs with proposal_dist Normal / Cauchy / Laplace: the batched
    stepper draws them on the device (used to raise NotImplementedError)"""
    import torch
    from beat_amd.sampler import SMC, smc_sample
    spec, prob, host, f, lay, _ = _small_model(ctx)
    lo, up = lay.bounds(host["lower"], host["upper"])
    for name in ("Normal", "Laplace", "Cauchy", "Poisson"):
        step = SMC(f, lo, up, n_chains=64, device=torch.device("cuda", 0), random_seed=2, proposal_name=name,
                   scale=1e-3, tune_interval=4)
        pop, lp, betas = smc_sample(6, step, max_stages=2)
        assert np.isfinite(lp[:, -1]).all() and pop.shape == (64, lo.size)
        assert ((pop >= lo) & (pop <= up)).all()
        assert 0.0 < np.mean(step.stage_acceptance) <= 1.0


def test_covariance_update_end_to_end(ctx):
    """SURVEY 8(f) row 3 / VERDICT r2 next #3: the per-stage covariance update of the reference's SMC
    (smc.py:492-503 -> seismic.py:1509-1534 -> covariance.py:307-325, 397-427 -> heart.py:211-253)
    composed on the device: MAP point -> synthetics -> residuals -> non-Toeplitz covariance ->
    PSD check by the factorisation -> whitening operators -> update_weights -> population evaluated
    again.  Checked against the oracle's twins of the same reference functions."""
    import torch
    from test_gpu_parity import _specs
    from beat_amd.covariance import NoiseCovarianceUpdate, running_window_rms_batch
    from beat_amd.sampler import SMC, smc_sample
    from beat_amd.synthetic import build_problem, draw_population
    from oracle import oracle as orc
    from oracle import problem_oracle
    spec = _specs()["seis_dense_ml_shifts"]
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    lay = host["layout"]
    Q = draw_population(spec, lay, host["lower"], host["upper"], 70)
    L0 = np.asarray(f.batch(Q))
    q_map = Q[int(np.argmax(L0[:, -1]))]
    upd = NoiseCovarianceUpdate(f)
    # the pieces against the reference's loops (oracle twins): synthetics, running rms, covariance
    covs, res = upd.data_covariances(q_map, 0)
    syn_ref = problem_oracle.forward(host, q_map)[1]["synthetics"]
    T, N = host["data"].shape
    np.testing.assert_allclose(res.cpu().numpy(), host["data"] - syn_ref, rtol=1e-9, atol=1e-9)
    r = res.cpu().numpy()
    w = N // 5
    stds_ref = np.stack([orc.running_window_rms(x, w, mode="same") for x in r])
    np.testing.assert_allclose(running_window_rms_batch(res, w).cpu().numpy(), stds_ref, rtol=1e-11)
    cov_ref = np.stack([orc.non_toeplitz_covariance(x, w) for x in r])
    np.testing.assert_allclose(covs.cpu().numpy(), cov_ref, rtol=1e-9, atol=1e-12)
    # the update: new weights = chol_inverse / log_pdet of the (repaired where needed) covariances
    upd.update_weights(q_map)
    assert upd.n_updates == 1 and upd.last_ms > 0
    host2 = dict(host)
    Wn, sl = [], []
    for t in range(T):
        c = cov_ref[t]
        try:
            np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            ev, evec = np.linalg.eigh(c)                       # utility.repair_covariance
            c = evec.dot(np.diag(np.maximum(ev, np.finfo(np.float64).eps))).dot(evec.T)
        Wn.append(orc.cov_chol_inverse(c))
        sl.append(orc.cov_log_pdet(c))
    host2["weights"], host2["slog"] = np.stack(Wn), np.array(sl)
    L1 = np.asarray(f.batch(Q))
    for c in (0, 13, 69):
        ref, _ = problem_oracle.forward(host2, Q[c])
        np.testing.assert_allclose(L1[c], ref, rtol=1e-6)          # north_star tolerance
        np.testing.assert_allclose(L1[c, -1], ref[-1], rtol=1e-8)
    assert not np.allclose(L0[:, -1], L1[:, -1])
    # a covariance that is not positive definite is found by the device factorisation and repaired
    bad = covs.clone()
    bad[1] = -bad[1]
    W, ld, flags = ctx.chol_inverse_batch_flags(bad)
    assert flags.cpu().numpy().tolist() == [0, 1] + [0] * (T - 2)
    # inside the sampler: every stage ends with an update and a re-evaluation of the population
    lo, up = lay.bounds(host["lower"], host["upper"])
    step = SMC(f, lo, up, n_chains=96, device=torch.device("cuda", 0), random_seed=4, tune_interval=3)
    upd2 = NoiseCovarianceUpdate(f)
    seen = []
    pop, lp, betas = smc_sample(3, step, max_stages=2, update=upd2,
                                on_stage=lambda s: seen.append(s.likelihoods.copy()))
    assert upd2.n_updates == len(seen) + 1 >= 2      # (+ the update after the initial stage, smc.py:459-503)
    assert all(np.isfinite(x).all() for x in seen) and np.isfinite(lp[:, -1]).all()


def _oracle_updated_weights(host, q_map, orc, problem_oracle):
    """the reference's per-stage weights at q_map through the oracle twins: residuals -> non-Toeplitz covariance
    (window n // 5) -> eigenvalue repair where needed -> chol_inverse / log_pdet"""
    syn = problem_oracle.forward(host, q_map)[1]["synthetics"]
    r = host["data"] - syn
    T, N = r.shape
    Wn, sl = [], []
    for t in range(T):
        c = orc.non_toeplitz_covariance(r[t], N // 5)
        try:
            np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            ev, evec = np.linalg.eigh(c)
            c = evec.dot(np.diag(np.maximum(ev, np.finfo(np.float64).eps))).dot(evec.T)
        Wn.append(orc.cov_chol_inverse(c))
        sl.append(orc.cov_log_pdet(c))
    return np.stack(Wn), np.array(sl)


def test_covariance_update_runs_after_the_initial_stage_and_survives_a_resume(ctx, tmp_path):
    """VERDICT r3 item 2c / ADVICE r3: the reference's update block sits inside the stage loop and therefore also
    runs after the initial (draws = 1) stage, before the first calc_beta (beat/sampler/smc.py:459-503).  The first
    tempering step must be the oracle's calc_beta on the prior population evaluated with the UPDATED weights.  The
    stage state keeps the point the weights were estimated at; a resumed run installs those weights again before it
    proposes against the saved likelihoods."""
    import torch
    from test_gpu_parity import _specs
    from beat_amd.covariance import NoiseCovarianceUpdate
    from beat_amd.sampler import SMC, smc_sample
    from beat_amd.synthetic import build_problem
    from oracle import oracle as orc
    from oracle import problem_oracle
    spec = _specs()["seis_dense_ml_shifts"]
    prob, host = build_problem(spec)
    lay = host["layout"]
    lo, up = lay.bounds(host["lower"], host["upper"])
    dev = torch.device("cuda", 0)

    def fresh():
        # (an update also rewrites the weights of the problem's wavemap objects: build the problem again)
        f = build_problem(spec)[0].compile(ctx)
        return f, SMC(f, lo, up, n_chains=96, device=dev, random_seed=4, tune_interval=3)

    f, step = fresh()
    home = str(tmp_path / "run")
    pop, lp, betas = smc_sample(3, step, max_stages=1, update=NoiseCovarianceUpdate(f), homepath=home)
    # the oracle's first beta: prior population (shared seeded stream), initial weights -> MAP -> new weights
    u = np.random.RandomState(4).random_sample((96, lo.size))
    Q0 = lo + (up - lo) * u
    L_init = np.array([problem_oracle.forward(host, q)[0] for q in Q0])
    q_map = Q0[int(np.argmax(L_init[:, -1]))]
    host2 = dict(host)
    host2["weights"], host2["slog"] = _oracle_updated_weights(host, q_map, orc, problem_oracle)
    like2 = np.array([problem_oracle.forward(host2, q)[0][-1] for q in Q0])
    beta_ref, _, _ = orc.calc_beta(like2, 0.0, 1.0)
    assert betas[0] == 0.0 and abs(betas[1] - beta_ref) <= 1e-9 * beta_ref, (betas, beta_ref)
    beta_wrong, _, _ = orc.calc_beta(L_init[:, -1], 0.0, 1.0)
    assert abs(beta_wrong - beta_ref) > 1e-6 * beta_ref        # (the old ordering would have given this one)
    # resume from stage 1 with a freshly compiled model (initial weights): the saved likelihoods must be
    # reproduced by the model once load_stage has run
    z = np.load(str(tmp_path / "run" / "stage_1" / "sampler_state.npz"))
    assert "update_map_point" in z.files
    f2, step2 = fresh()
    L_before = np.asarray(f2.batch(z["population"]))
    assert not np.allclose(L_before[:, -1], z["lpoints"][:, -1], rtol=1e-9)
    upd2 = NoiseCovarianceUpdate(f2)
    pop2, lp2, betas2 = smc_sample(3, step2, max_stages=1, update=upd2, homepath=home, resume_stage=1)
    assert upd2.n_updates >= 1
    f3, step3 = fresh()
    from beat_amd.sampler.smc import load_stage
    load_stage(step3, home, 1)
    NoiseCovarianceUpdate(f3).update_weights(step3.update_map_point)
    np.testing.assert_allclose(np.asarray(f3.batch(z["population"])), z["lpoints"], rtol=1e-9, atol=1e-9)
    assert np.isfinite(lp2[:, -1]).all()


def test_covariance_update_of_a_prewhitened_model(ctx):
    """a model compiled with a pre-whitened library returns W_old (d - s) as residuals; the noise
    covariance has to be estimated on d - s like the reference does (covariance.py:307-325).  The updated
    pre-whitened model must agree with the updated dense-W model (and the oracle's weights)."""
    from test_gpu_parity import _specs
    from beat_amd.covariance import NoiseCovarianceUpdate
    from beat_amd.synthetic import build_problem, draw_population
    from oracle import oracle as orc
    from oracle import problem_oracle
    spec = _specs()["seis_dense_ml_shifts"]
    prob_a, host = build_problem(spec)
    prob_b, _ = build_problem(spec)
    fa = prob_a.compile(ctx)
    fb = prob_b.compile(ctx, prewhiten=True)
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], 40)
    La0, Lb0 = np.asarray(fa.batch(Q)), np.asarray(fb.batch(Q))
    np.testing.assert_allclose(Lb0, La0, rtol=1e-9)
    q_map = Q[int(np.argmax(La0[:, -1]))]
    ua, ub = NoiseCovarianceUpdate(fa), NoiseCovarianceUpdate(fb)
    ca, ra = ua.data_covariances(q_map, 0)
    cb, rb = ub.data_covariances(q_map, 0)
    np.testing.assert_allclose(rb.cpu().numpy(), ra.cpu().numpy(), rtol=1e-8, atol=1e-9)   # d - s, not W (d - s)
    np.testing.assert_allclose(cb.cpu().numpy(), ca.cpu().numpy(), rtol=1e-6, atol=1e-12)
    for k in range(2):          # two successive updates: the second starts from an already re-whitened library
        ua.update_weights(q_map)
        ub.update_weights(q_map)
        La, Lb = np.asarray(fa.batch(Q)), np.asarray(fb.batch(Q))
        np.testing.assert_allclose(Lb, La, rtol=1e-6)
        q_map = Q[int(np.argmax(La[:, -1]))]
    host2 = dict(host)
    q_first = Q[int(np.argmax(La0[:, -1]))]
    host2["weights"], host2["slog"] = _oracle_updated_weights(host, q_map if False else q_first, orc, problem_oracle)
    fa2 = build_problem(spec)[0].compile(ctx)
    NoiseCovarianceUpdate(fa2).update_weights(q_first)
    ref = problem_oracle.forward(host2, Q[3])[0]
    np.testing.assert_allclose(np.asarray(fa2.batch(Q))[3], ref, rtol=1e-6)


@pytest.mark.parametrize("ndip,kind,df,per_chain_beta", [(4, -1, 0, False), (4, -1, 3, True), (4, 1, 0, False),
                                                         (6, -1, 0, True), (6, -1, 4, False), (6, 2, 0, False),
                                                         (4, 0, 0, False), (4, 3, 0, True)])
def test_fused_step_equals_draw_plus_astep(ctx, ndip, kind, df, per_chain_beta):
    """beatamd_ffi_mstep_batch (draws + proposal + forward model + accept + counters in one call) against
    the two calls it replaces, beatamd_proposal_draw[_univariate] + beatamd_ffi_astep_batch[_betas]: the
    same Philox counters, so the same chains.  More than 64 parameters: the same kernels run -> bitwise.
    Up to 64 the draws, the factor product and the box test are one kernel (k_draw_propose).  A per-parameter
    family (kind >= 0) has no product in it: the same device functions draw, scale, propose and accept in the
    same order on both paths and contraction is off -> bitwise too, Q, L and the flags after every step.  The
    multivariate proposal (kind < 0) goes through an FMA chain there instead of the matrix-core GEMM: last-bit
    differences in the proposal, compared to a tolerance and the chains re-joined after every step.
    The fixture has 52 parameters at ndip = 4, an even count: the odd tail of a row (second scale 0.0, second
    draw dropped) is covered by k_philox_univariate's npar = 7 test only.  70 chains leave the last workgroup
    of k_draw_propose with 6 of its 16 chains.
    Poisson (kind 3): integer steps of a parameter's span would leave the box every time, so every width is
    1e-3: 95 % of the rows draw k = 0 everywhere and move by -lam * scaling, the others jump by one in some
    parameter.  Measured on the build before the draws became shared device functions: 27 of the 4 x 70
    proposals accepted (8, 5, 7, 7 per step), 9.6 %; widths of 2e-3 / 5e-3 / 1e-2 gave 7.1 / 4.3 / 2.9 %."""
    import torch
    from beat_amd.synthetic import SyntheticSpec, build_problem, draw_population
    spec = SyntheticSpec((ndip,), (ndip,), (1.0,), T=3, N=32, D=3, S=25)
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    lay = host["layout"]
    npar = lay.size
    assert (npar <= 64) == (ndip == 4)
    dev = torch.device("cuda", 0)
    C = 70
    Q = torch.from_numpy(draw_population(spec, lay, host["lower"], host["upper"], C)).to(dev)
    L = f.batch(Q)
    lo_h, up_h = lay.bounds(host["lower"], host["upper"])
    lo, up = torch.from_numpy(lo_h).to(dev), torch.from_numpy(up_h).to(dev)
    rng = np.random.default_rng(3)
    span = np.where(up_h > lo_h, up_h - lo_h, 1.0)
    if kind < 0:
        factor = torch.from_numpy(rng.standard_normal((npar, npar)) * 2e-3 * span[None, :] / np.sqrt(npar)).to(dev)
    elif kind == 3:
        factor = torch.full((npar,), 1e-3, dtype=torch.float64, device=dev)
    else:
        factor = torch.from_numpy(2e-3 * span).to(dev)
    scaling = torch.from_numpy(0.5 + rng.random(C)).to(dev)
    beta = torch.from_numpy(rng.random(C)).to(dev) if per_chain_beta else 0.3
    QA, LA, QB, LB = Q.clone(), L.clone(), Q.clone(), L.clone()
    accA = torch.zeros(C, dtype=torch.int32, device=dev)
    accB = torch.zeros(C, dtype=torch.int32, device=dev)
    acc_sum = torch.zeros(C, dtype=torch.int32, device=dev)
    n_acc = torch.zeros((), dtype=torch.int64, device=dev)
    total = np.zeros(C, dtype=np.int64)
    for step in range(4):
        if kind < 0:
            delta, log_u = ctx.proposal_draw(factor, C, 77, step, first_chain=5, df=df)
        else:
            delta, log_u = ctx.proposal_draw_univariate(kind, factor, C, 77, step, first_chain=5)
        f.astep_batch(QA, LA, delta, scaling, lo, up, log_u, beta, accA)
        f.mstep_batch(QB, LB, factor, None if kind < 0 else kind, df, 77, step, 5, scaling, lo, up, beta, accB,
                      acc_sum, n_acc)
        assert torch.equal(accA, accB), "step %d" % step
        total += accA.cpu().numpy()
        if npar > 64 or kind >= 0:
            assert torch.equal(QA, QB) and torch.equal(LA, LB), "step %d" % step
        else:
            np.testing.assert_allclose(QB.cpu().numpy(), QA.cpu().numpy(), rtol=1e-13, atol=1e-15)
            np.testing.assert_allclose(LB.cpu().numpy(), LA.cpu().numpy(), rtol=1e-9)
            QB.copy_(QA)
            LB.copy_(LA)
    assert 0 < total.sum() < 4 * C
    if kind == 3:
        assert 0.05 * 4 * C <= total.sum() <= 0.95 * 4 * C
    assert np.array_equal(acc_sum.cpu().numpy(), total) and int(n_acc.item()) == total.sum()
