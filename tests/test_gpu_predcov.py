"""The velocity-model prediction covariance on the device (csrc/predcov.hip, beat_amd.covariance): the ensemble stack
against the reference's numbers (tests/golden/pred_cov.npz), exact integer arithmetic and the model's own mu; the sample
covariance bit for bit against the numpy restatement (tests/predcov_ref.py) at the kernel's tile and chunk edges; the
update end to end against the one-chain oracle composition with the reference's weights; and its rules -- threshold,
cache drop, an indefinite total, the sampler, target sharding."""
import os
import socket
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predcov_ref as pref  # noqa: E402
from _shard_predcov_gpu_worker import crust_ensemble, joint_problem  # noqa: E402
from conftest import ROOT, load_golden  # noqa: E402
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

SLIPS = ("uparr", "uperp")


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.fixture(scope="module")
def gold():
    return load_golden("pred_cov")


def _dev(a, ctx):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", ctx.device))


def _ensemble_of(G, varnames=SLIPS, crust_inds=None):
    """G [K, nvar, P, nobs] -> GeodeticGFEnsemble"""
    from beat_amd.ffi import GeodeticGFEnsemble, GeodeticGFLibrary, GeodeticGFLibraryConfig
    libs = {}
    for k in range(G.shape[0]):
        ci = k if crust_inds is None else crust_inds[k]
        libs[ci] = {}
        for iv, v in enumerate(varnames):
            gf = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=G.shape[2:], component=v, crust_ind=ci))
            gf.setup(G.shape[2], G.shape[3], allocate=True)
            gf._gfmatrix[:] = G[k, iv]
            libs[ci][v] = gf
    return GeodeticGFEnsemble(libs, varnames)


def _raw_stack(ctx, G, slips):
    """the C entries on plain arrays: G [K, nvar, P, nobs], slips [nvar, P] -> X [K, nobs] (libraries released again)"""
    K, nvar, P, nobs = G.shape
    ids = [ctx.geo_gflib_create(G[k, v]) for k in range(K) for v in range(nvar)]
    eid = ctx.geo_ensemble_create(ids, K, nvar)
    try:
        return ctx.geo_ensemble_stack(eid, K, nobs, np.ascontiguousarray(slips).ravel())
    finally:
        ctx.geo_ensemble_destroy(eid)
        for i in ids:
            ctx.geo_gflib_destroy(i)


# ------------------------------------------------------------------------------------------------- the ensemble stack
@pytest.mark.parametrize("case", ["small", "laquila"])
def test_stack_vs_fixture(ctx, gold, case):
    """the reference's stack_all per variant, summed over the slip variables: rtol = atol = 1e-12 (test_geo_stack_golden)"""
    G, slips, X = gold[case + "_G"], gold[case + "_slips"], gold[case + "_X"]
    ens = _ensemble_of(G)
    got = ens.stack_all({v: slips[i] for i, v in enumerate(SLIPS)})
    assert isinstance(got, np.ndarray) and got.shape == X.shape
    np.testing.assert_allclose(got, X, rtol=1e-12, atol=1e-12)
    dev = ens.stack_all(_dev(slips, ctx))
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)
    ens.release()


@pytest.mark.parametrize("P", [1, 15, 16, 17, 33])
def test_stack_shapes_on_exact_inputs(ctx, P):
    """integer-valued libraries and slips in [-7, 7]: every product and partial sum is an integer below 2^53, so the
    result equals int64 arithmetic whatever the order.  Patches around the sixteen-load groups; observation counts around
    the 128-column block and the Laquila total; 1, 2, 7 and 40 variants; one and two slip variables."""
    rng = np.random.default_rng(P)
    for nobs in (1, 127, 128, 129, 419):
        for K, nvar in ((1, 1), (2, 2), (7, 2), (40, 1)):
            G = rng.integers(-7, 8, (K, nvar, P, nobs))
            s = rng.integers(-7, 8, (nvar, P))
            want = np.einsum("kvpj,vp->kj", G, s)
            got = _raw_stack(ctx, G.astype(np.float64), s.astype(np.float64))
            assert got.shape == (K, nobs) and np.array_equal(got, want.astype(np.float64)), (P, nobs, K, nvar)


def test_ensemble_entry_points_refuse_bad_arguments(ctx):
    a, b = ctx.geo_gflib_create(np.zeros((3, 4))), ctx.geo_gflib_create(np.zeros((3, 5)))
    with pytest.raises(ValueError, match="is \\(3, 5\\)"):
        ctx.geo_ensemble_create([a, b], 2, 1)
    with pytest.raises(ValueError, match="unknown geodetic GF library"):
        ctx.geo_ensemble_create([a, 9999], 2, 1)
    eid = ctx.geo_ensemble_create([a, a], 2, 1)
    ctx.geo_gflib_destroy(a)
    with pytest.raises(ValueError, match="destroyed or replaced"):
        ctx.geo_ensemble_stack(eid, 2, 4, np.zeros(3))
    ctx.geo_ensemble_destroy(eid)
    ctx.geo_gflib_destroy(b)
    with pytest.raises(ValueError, match="at least 2 variants"):
        ctx.pred_covariance_batch(np.zeros((1, 4)), [4])
    with pytest.raises(ValueError, match="add up to"):
        ctx.pred_covariance_batch(np.zeros((3, 4)), [3])


# ------------------------------------------------------------------------------------------------- the sample covariance
T, KC = pref.PC_TILE, pref.PC_KC
COV_CASES = [
    # (K, sizes, which bases are given)
    (7, [T - 1, T, T + 1], (True, True, True)),            # one below, at and one above the tile edge (rows and columns)
    (2, [1, 205, 214], (False, True, True)),               # the Laquila sizes behind a one-point dataset: odd offsets
    (7, [2 * T + 1, 3], (True, False)),                    # three tiles a side, inner tiles included
    (KC, [T + 1, 5], (True, True)),                        # K at the chunk length
    (KC + 1, [T + 1, 5], (True, True)),                    # one above: a chunk of one row
    (2 * KC + 3, [9], (False,)),                           # three chunks, no base at all
]


@pytest.mark.parametrize("K,sizes,has_base", COV_CASES)
def test_covariance_bitwise_vs_restatement(ctx, K, sizes, has_base):
    rng = np.random.default_rng(K + sum(sizes))
    nobs = sum(sizes)
    X = 0.3 + rng.standard_normal((K, nobs)) * 10.0 ** rng.uniform(-2, 1, nobs)
    base = []
    for n, on in zip(sizes, has_base):
        b = rng.standard_normal((n, n))
        base.append(b @ b.T + n * np.eye(n) if on else None)
    want = pref.pred_covariance(X, sizes, base)
    if not any(has_base):
        base = None
    got = ctx.pred_covariance_batch(X, sizes, base)                                    # host arrays
    dbase = None if base is None else [None if b is None else _dev(b, ctx) for b in base]
    dgot = ctx.pred_covariance_batch(_dev(X, ctx), sizes, dbase)                       # device arrays
    mixed = ctx.pred_covariance_batch(_dev(X, ctx), sizes, base)                       # device X, host bases
    for i, n in enumerate(sizes):
        assert isinstance(got[i], np.ndarray) and got[i].shape == (n, n)
        assert np.array_equal(got[i], want[i]), (K, sizes, i, np.abs(got[i] - want[i]).max())
        assert dgot[i].is_cuda and np.array_equal(dgot[i].cpu().numpy(), want[i])
        assert np.array_equal(mixed[i].cpu().numpy(), want[i])
        assert np.array_equal(got[i], got[i].T)
    # into caller's matrices, in place
    out = [np.full((n, n), np.nan) for n in sizes]
    back = ctx.pred_covariance_batch(X, sizes, base, out=out)
    assert all(b is o and np.array_equal(o, w) for b, o, w in zip(back, out, want))


def test_covariance_vs_fixture_raw(ctx, gold):
    """against the reference's num.cov of the small case: the CPU tests' bound, 2 * 8 (K + 3) 2^-53 a_i a_j"""
    X, sizes = gold["small_X"], [int(n) for n in gold["small_sizes"]]
    got = ctx.pred_covariance_batch(X, sizes)
    o, worst = 0, 0.0
    for i, n in enumerate(sizes):
        frac = np.abs(got[i] - gold["small_raw%d" % i]) / pref.cov_bound(X[:, o:o + n])
        worst = max(worst, float(frac.max()))
        assert np.all(frac <= 2.0), (i, float(frac.max()))
        o += n
    print("device sample covariance vs the fixture's num.cov: worst |difference| / bound = %.3g" % worst)


# ------------------------------------------------------------------------------------------------- the update, end to end
def _laquila_problem(gold, data_covs=None):
    """a geodetic FFI problem over the two Laquila scenes with the fixture's reference libraries (variant 0), compiled with
    the data covariances alone -> (problem, layout, host arrays, Covariance objects)"""
    from beat_amd.ffi import GeodeticGFLibrary, GeodeticGFLibraryConfig
    from beat_amd.heart import Covariance
    from beat_amd.models import FFIProblem, GeodeticData, ParameterLayout
    laq = load_golden("laquila_geodetic")
    G = gold["laquila_G"]
    P, nobs = G.shape[2:]
    sizes = [int(n) for n in gold["laquila_sizes"]]
    gfs = {}
    for iv, v in enumerate(SLIPS):
        gg = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=(P, nobs), component=v))
        gg.setup(P, nobs, allocate=True)
        gg._gfmatrix[:] = G[0, iv]
        gfs[v] = gg
    lay = ParameterLayout(OrderedDict([(v, P) for v in SLIPS] + [("h_SAR", 1)]))
    lower = dict(uparr=0.0, uperp=0.0, h_SAR=-1.0)
    upper = dict(uparr=3.0, uperp=3.0, h_SAR=1.0)
    data = np.concatenate([laq["d%d_displacement" % d] for d in range(2)])
    odw = np.concatenate([laq["d%d_odw" % d] for d in range(2)])
    Cs = [laq["d%d_C" % d] for d in range(2)] if data_covs is None else data_covs
    covs = [Covariance(data=C) for C in Cs]
    W = [c.chol_inverse for c in covs]
    sl = [float(c.log_pdet) for c in covs]
    geo = GeodeticData(gfs, data, odw, sizes, W, sl, [("h_SAR", 0)] * 2)
    prob = FFIProblem(lay, [], [], [], SLIPS, geodetic=geo, lower=lower, upper=upper)
    host = dict(Gs=[G[0, 0], G[0, 1]], data=data, odw=odw, sizes=sizes, W=W, sl=sl, C=Cs)
    return prob, lay, host, covs


def _ffi_ref(host, lay, q, W, sl):
    """geodetic.py:1065-1081 for one chain through the oracle pieces"""
    pt = lay.rmap(q)
    mu = np.zeros(host["data"].size)
    for G, v in zip(host["Gs"], SLIPS):
        mu += orc.geo_stack(G, pt[v])
    res = (host["data"] - mu) * host["odw"]
    out, o = [], 0
    for n, Wk, slk in zip(host["sizes"], W, sl):
        out.append(orc.mvn_chol_logp(Wk, res[o:o + n], slk, pt["h_SAR"][0]))
        o += n
    return np.array(out + [sum(out)])


def _population(lay, lower, upper, C, seed=3):
    lo, up = lay.bounds(lower, upper)
    return lo + (up - lo) * np.random.default_rng(seed).random((C, lay.size))


def _q_map(gold, lay):
    q = np.zeros(lay.size)
    for i, v in enumerate(SLIPS):
        q[lay.offsets[v]:lay.offsets[v] + gold["laquila_slips"].shape[1]] = gold["laquila_slips"][i]
    return q


@pytest.fixture(scope="module")
def reference_weights(gold):
    """the reference's route on the host, once: num.cov of the fixture's X -> ensure_cov_psd -> Covariance(data,
    pred_v=repaired) -> chol_inverse, log_pdet (pinned to the reference by the fixture's log_pdet)"""
    from beat_amd.heart import Covariance
    from beat_amd.utility import ensure_cov_psd
    laq = load_golden("laquila_geodetic")
    X = gold["laquila_X"]
    W, sl, o = [], [], 0
    for d, n in enumerate(int(n) for n in gold["laquila_sizes"]):
        rep = ensure_cov_psd(np.cov(X[:, o:o + n], rowvar=0))
        cov = Covariance(data=laq["d%d_C" % d], pred_v=rep)
        W.append(cov.chol_inverse)
        sl.append(float(cov.log_pdet))
        np.testing.assert_allclose(sl[-1], float(gold["laquila_logpdet%d" % d]), rtol=1e-9)
        o += n
    return W, sl


def test_update_end_to_end_on_the_laquila_case(ctx, gold, reference_weights):
    from beat_amd.covariance import VelocityModelCovarianceUpdate
    prob, lay, host, covs = _laquila_problem(gold)
    f = prob.compile(ctx)
    ens = _ensemble_of(gold["laquila_G"])
    Q = _population(lay, prob.lower, prob.upper, 70)
    q_map = _q_map(gold, lay)
    L0 = np.asarray(f.batch(Q))
    upd = VelocityModelCovarianceUpdate(f, ens, covs, reference_crust_ind=0)
    # the stack: the fixture's X, and the reference variant's row is the model's own mu bit for bit
    X = upd.crust_synthetics(q_map).cpu().numpy()
    np.testing.assert_allclose(X, gold["laquila_X"], rtol=1e-12, atol=1e-12)
    mu = f.geodetic_residuals(q_map[None, :], residuals=False)
    assert np.array_equal(X[ens.index(0)], np.asarray(mu)[0])
    upd.update_weights(q_map)
    assert upd.n_updates == 1 and upd.n_host_route == 0 and upd.last_ms > 0
    L1 = np.asarray(f.batch(Q))
    Wr, slr = reference_weights
    for c in range(70):
        ref = _ffi_ref(host, lay, Q[c], Wr, slr)
        np.testing.assert_allclose(L1[c], ref, rtol=1e-6)                 # test_covariance_update_end_to_end's tolerances
        np.testing.assert_allclose(L1[c, -1], ref[-1], rtol=1e-8)
    assert not np.allclose(L0[:, -1], L1[:, -1])
    # log_pdet against the reference's own number; problem.geodetic and the Covariance objects follow
    g = f.problem.geodetic
    o = 0
    for d, n in enumerate(host["sizes"]):
        np.testing.assert_allclose(g.slog_pdets[d], float(gold["laquila_logpdet%d" % d]), rtol=1e-9)
        assert float(covs[d].slog_pdet.get_value()) == g.slog_pdets[d]
        Wd = g.weights[d].cpu().numpy()
        assert Wd.shape == (n, n) and not np.tril(Wd, -1).any()
        # |W r|^2 of the fixture's residual vectors with the reference's operator: c n u kappa(C) ~ 4 * 214 * 1.1e-16 * 1e3
        # = 1e-10 for the other factorisation order, 2.3e-10 for the raw instead of the repaired term -> 1e-8
        quad = np.array([np.sum(Wd.dot(r) ** 2) for r in gold["laquila_r%d" % d]])
        np.testing.assert_allclose(quad, gold["laquila_quad%d" % d], rtol=1e-8)
        # pred_v: the raw sample covariance, left on the device until read
        assert hasattr(covs[d]._terms["pred_v"], "is_cuda")
        pv = covs[d].pred_v
        assert isinstance(pv, np.ndarray) and np.array_equal(pv, pref.pred_covariance(X[:, o:o + n], [n])[0])
        o += n
    f.release()
    ens.release()


def test_update_drops_the_cached_observation_quads(ctx, gold):
    """after the update ``obs_quads`` and ``variance_reductions`` are bit for bit those of a model compiled fresh with the
    new weights (the cache was filled with the old ones before)"""
    from beat_amd.covariance import VelocityModelCovarianceUpdate
    from beat_amd.models import FFIProblem, GeodeticData
    prob, lay, host, covs = _laquila_problem(gold)
    f = prob.compile(ctx)
    Q = _population(lay, prob.lower, prob.upper, 9)
    old = f.obs_quads().copy()
    VelocityModelCovarianceUpdate(f, _ensemble_of(gold["laquila_G"]), covs).update_weights(_q_map(gold, lay))
    g = prob.geodetic
    fresh_geo = GeodeticData(g.gfs, g.data, g.odws, g.sizes, [w.cpu().numpy() for w in g.weights], g.slog_pdets, g.hypers)
    f2 = FFIProblem(lay, [], [], [], SLIPS, geodetic=fresh_geo, lower=prob.lower, upper=prob.upper).compile(ctx)
    new = f.obs_quads()
    assert np.array_equal(new, f2.obs_quads()) and not np.array_equal(new, old)
    assert np.array_equal(f.variance_reductions(Q), f2.variance_reductions(Q))
    assert np.array_equal(np.asarray(f.batch(Q)), np.asarray(f2.batch(Q)))
    f2.release()
    f.release()


def test_threshold_five_variants_install_nothing_six_do(ctx, gold):
    from beat_amd.covariance import VelocityModelCovarianceUpdate
    prob, lay, host, covs = _laquila_problem(gold)
    f = prob.compile(ctx)
    Q = _population(lay, prob.lower, prob.upper, 9)
    q_map = _q_map(gold, lay)
    L0 = np.asarray(f.batch(Q)).copy()
    upd = VelocityModelCovarianceUpdate(f, _ensemble_of(gold["laquila_G"][:5]), covs)
    upd.update_weights(q_map)
    assert upd.n_updates == 1 and np.array_equal(np.asarray(f.batch(Q)), L0)
    upd = VelocityModelCovarianceUpdate(f, _ensemble_of(gold["laquila_G"][:6]), covs)
    upd.update_weights(q_map)
    L1 = np.asarray(f.batch(Q))
    assert np.isfinite(L1).all() and not np.array_equal(L1, L0)
    f.release()


def test_indefinite_total_raises_and_leaves_the_weights(ctx, gold):
    """a dataset whose data covariance is -1e-3 I: the device factorisation flags the total (a return value, no fault),
    the host route fails like the reference's, LinAlgError names the dataset, nothing was installed; the next valid update
    succeeds"""
    from beat_amd.covariance import VelocityModelCovarianceUpdate
    prob, lay, host, covs = _laquila_problem(gold)
    f = prob.compile(ctx)
    Q = _population(lay, prob.lower, prob.upper, 9)
    q_map = _q_map(gold, lay)
    L0 = np.asarray(f.batch(Q)).copy()
    good = covs[1].data
    covs[1].data = -1e-3 * np.eye(good.shape[0])
    upd = VelocityModelCovarianceUpdate(f, _ensemble_of(gold["laquila_G"]), covs)
    with pytest.raises(np.linalg.LinAlgError, match="geodetic dataset 1"):
        upd.update_weights(q_map)
    assert upd.n_host_route == 1
    assert np.array_equal(np.asarray(f.batch(Q)), L0)
    covs[1].data = good.copy()
    upd.update_weights(q_map)
    assert upd.n_updates == 2 and upd.n_host_route == 1
    L1 = np.asarray(f.batch(Q))
    assert np.isfinite(L1).all() and not np.array_equal(L1, L0)
    f.release()


def test_update_geodetic_weights_checks_kind_and_size(ctx, gold):
    prob, lay, host, covs = _laquila_problem(gold)
    f = prob.compile(ctx)
    Q = _population(lay, prob.lower, prob.upper, 5)
    L0 = np.asarray(f.batch(Q)).copy()
    W, sl = host["W"], host["sl"]
    with pytest.raises(ValueError, match="for 2 geodetic datasets"):
        f.update_geodetic_weights(W[:1], sl[:1])
    with pytest.raises(ValueError, match="dataset 1 holds dense weights"):
        f.update_geodetic_weights([W[0], 2.0], sl)
    with pytest.raises(ValueError, match="dataset 0 holds dense weights"):
        f.update_geodetic_weights([W[1], W[1]], sl)
    assert np.array_equal(np.asarray(f.batch(Q)), L0)
    f.update_geodetic_weights([2.0 * W[0], _dev(W[1], ctx)], [sl[0] - 2 * 214 * np.log(2.0), sl[1]])
    L1 = np.asarray(f.batch(Q))
    assert np.array_equal(L1[:, 1], L0[:, 1]) and not np.array_equal(L1[:, 0], L0[:, 0])
    f.release()


def test_update_geodetic_weights_of_a_scalar_dataset(ctx, gold):
    """a dataset compiled with a scalar weight takes a scalar and refuses an operator; against the one-chain composition
    with w I at rtol = atol = 1e-9 (test_ffi_logp_batch_vs_oracle)"""
    prob, lay, host, covs = _laquila_problem(gold)
    n1 = host["sizes"][1]
    prob.geodetic.weights = [host["W"][0], 300.0]
    prob.geodetic.slog_pdets = [host["sl"][0], -2.0 * n1 * np.log(300.0)]
    f = prob.compile(ctx)
    Q = _population(lay, prob.lower, prob.upper, 5)
    with pytest.raises(ValueError, match="dataset 1 holds scalar weights"):
        f.update_geodetic_weights(host["W"], host["sl"])
    sl = [host["sl"][0], -2.0 * n1 * np.log(150.0)]
    f.update_geodetic_weights([host["W"][0], 150.0], sl)
    assert f.problem.geodetic.weights[1] == 150.0 and f.problem.geodetic.slog_pdets == sl
    L1 = np.asarray(f.batch(Q))
    for c in range(5):
        np.testing.assert_allclose(L1[c], _ffi_ref(host, lay, Q[c], [host["W"][0], 150.0 * np.eye(n1)], sl), rtol=1e-9, atol=1e-9)
    f.release()


# ------------------------------------------------------------------------------------------------- sampler
def test_sampler_runs_both_updates_every_stage(ctx):
    """smc_sample(update=CovarianceUpdates(noise, velocity)) on a small joint problem: 96 chains, 2 stages; both updates
    run once per stage and once after the initial stage (smc.py:459-503), all likelihoods finite"""
    import torch
    from beat_amd.covariance import CovarianceUpdates, NoiseCovarianceUpdate, VelocityModelCovarianceUpdate
    from beat_amd.sampler import SMC, smc_sample
    spec, prob, host, covs = joint_problem()
    f = prob.compile(ctx)
    lo, up = host["layout"].bounds(host["lower"], host["upper"])
    step = SMC(f, lo, up, n_chains=96, device=torch.device("cuda", 0), random_seed=4, tune_interval=3)
    noise = NoiseCovarianceUpdate(f)
    vel = VelocityModelCovarianceUpdate(f, crust_ensemble(prob.geodetic.gfs, spec.slip_varnames, 6), covs)
    seen = []
    pop, lp, betas = smc_sample(3, step, max_stages=2, update=CovarianceUpdates(noise, vel),
                                on_stage=lambda s: seen.append(s.likelihoods.copy()))
    assert noise.n_updates == vel.n_updates == len(seen) + 1 >= 2
    assert vel.n_host_route == 0
    assert all(np.isfinite(x).all() for x in seen) and np.isfinite(lp[:, -1]).all()
    f.release()


# ------------------------------------------------------------------------------------------------- sharded
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_shard(nproc, mode, out):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "BEATAMD_GF_SPLIT"):
        env.pop(k, None)
    env.update(BEATAMD_TEST_OUT=out, BEATAMD_TEST_MODE=mode, OMP_NUM_THREADS="1")
    worker = os.path.join(ROOT, "tests", "_shard_predcov_gpu_worker.py")
    if nproc == 1:
        cmd = [sys.executable, worker]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("SHARD_PREDCOV_WORKER_OK") == nproc, r.stdout[-2000:]
    return np.load(out)


def test_update_beside_a_target_sharded_wavemap(tmp_path):
    """the geodetic composite is replicated on every rank of a target-sharded model and every rank installs the same new
    operators: 2 ranks on one GPU give the likelihood vectors of the replicated model bit for bit, before and after the
    update, and the update moves the geodetic columns only"""
    rep = _run_shard(1, "replicated", str(tmp_path / "rep.npz"))
    two = _run_shard(2, "targets", str(tmp_path / "two.npz"))
    assert rep["after"].shape == two["after"].shape == (70, 8) and np.isfinite(rep["after"]).all()
    assert np.array_equal(rep["before"], two["before"]) and np.array_equal(rep["after"], two["after"])
    assert np.array_equal(rep["after"][:, :5], rep["before"][:, :5])
    assert not np.array_equal(rep["after"][:, 5], rep["before"][:, 5])
    assert not np.array_equal(rep["after"][:, 6], rep["before"][:, 6])
