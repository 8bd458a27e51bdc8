"""The geodetic non-Toeplitz data covariance on the device (csrc/noise2d.hip, beat_amd.covariance): the neighbourhood
statistic bit for bit against the numpy restatement of its one stated order (tests/noise2d_ref.py) at wavefront, block and
tile edges, alone and in a batch; against the reference's numbers (tests/golden/noise2d.npz); the update end to end against
the one-chain oracle composition with the reference's weights; and its rules -- a point without a neighbour, odw and
corrections, the velocity update in the same pass, the sampler."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise2d_ref as nref  # noqa: E402
from _shard_predcov_gpu_worker import crust_ensemble, joint_problem  # noqa: E402
from conftest import load_golden  # noqa: E402
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

SLIPS = ("uparr", "uperp")
NPATCH = 6
TILE = nref.NB_TILE


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.fixture(scope="module")
def gold():
    return load_golden("noise2d")


def _dev(a, ctx):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", ctx.device))


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _scene(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-20e3, 20e3, (n, 2)), 0.01 + 2e-3 * rng.standard_normal(n)


# ------------------------------------------------------------------------------------------------- kernel vs restatement
# sizes around the 64 lanes of a point's wavefront, the four points of a block and the 1024-point LDS tile; the smallest
# scenes at a fraction above 1 (every point a neighbour of every other), the others at a fraction that leaves some points
# few neighbours
EDGE_CASES = [(2, 1.5), (3, 1.5), (63, 0.3), (64, 0.3), (65, 0.3), (129, 0.25), (TILE - 1, 0.1), (TILE + 1, 0.1)]


@pytest.mark.parametrize("n,perc", EDGE_CASES)
def test_kernel_bitwise_vs_restatement(ctx, n, perc):
    coords, data = _scene(n, n)
    radius, counts, stds = nref.ball_rms(coords, data, perc)
    assert counts.max() >= 2
    got = ctx.ball_rms_batch(coords, data, [n], perc)                                   # host arrays
    assert all(isinstance(g, np.ndarray) for g in got) and got[1].dtype == np.int32
    assert got[0].shape == (1,) and got[1].shape == (n,) and got[2].shape == (n,)
    assert got[0][0] == radius and np.array_equal(got[1], counts) and _same(got[2], stds), (n, perc)
    dgot = ctx.ball_rms_batch(_dev(coords, ctx), _dev(data, ctx), [n], perc)            # device arrays
    assert all(g.is_cuda for g in dgot)
    assert dgot[0].cpu().numpy()[0] == radius and np.array_equal(dgot[1].cpu().numpy(), counts)
    assert _same(dgot[2].cpu().numpy(), stds)


def test_two_points_apart_have_no_neighbour(ctx):
    """n = 2 at a fraction below 1: each point alone in its ball, count 1, NaN"""
    coords, data = _scene(2, 2)
    radius, counts, stds = ctx.ball_rms_batch(coords, data, [2], 0.5)
    assert np.array_equal(counts, [1, 1]) and np.isnan(stds).all()
    assert _same(stds, nref.ball_rms(coords, data, 0.5)[2])


def test_batch_and_alone_give_the_same_bits(ctx):
    """datasets of 2, 65 and 33 points in one call: the restatement's bits, and every dataset alone gives the same bits as
    inside the batch (the order depends on the point and its dataset's size alone); host and device inputs"""
    sizes = [2, 65, 33]
    parts = [_scene(n, 100 + n) for n in sizes]
    coords, data = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    perc = 0.6
    want = nref.ball_rms_batch(coords, data, sizes, perc)
    got = ctx.ball_rms_batch(coords, data, sizes, perc)
    dgot = [g.cpu().numpy() for g in ctx.ball_rms_batch(_dev(coords, ctx), _dev(data, ctx), sizes, perc)]
    for w, g, d in zip(want, got, dgot):
        assert _same(g, w) and _same(d, w)
    o = 0
    for i, n in enumerate(sizes):
        r, k, s = ctx.ball_rms_batch(coords[o:o + n], data[o:o + n], [n], perc)
        assert r[0] == got[0][i] and np.array_equal(k, got[1][o:o + n]) and _same(s, got[2][o:o + n])
        o += n


def test_entry_refuses_bad_arguments(ctx):
    c, d = np.zeros((4, 2)), np.zeros(4)
    with pytest.raises(ValueError, match="dataset 1 has 0 points"):
        ctx.ball_rms_batch(c, d, [4, 0], 0.2)
    with pytest.raises(ValueError, match="1..65535 datasets"):
        ctx.ball_rms_batch(np.zeros((0, 2)), np.zeros(0), [], 0.2)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="max_dist_perc is not finite"):
            ctx.ball_rms_batch(c, d, [4], bad)
    with pytest.raises(ValueError, match="expected \\(4, 2\\) and \\(4,\\)"):
        ctx.ball_rms_batch(c, d[:3], [4], 0.2)


# ------------------------------------------------------------------------------------------------- kernel vs the reference
@pytest.mark.parametrize("case", ["n30", "n33", "laq0", "laq1", "n1024", "grid"])
def test_kernel_vs_fixture(ctx, gold, case):
    """the CPU test's tolerances: radius bit for bit, counts exact (the grid: every neighbour a tie), stds rtol 1e-12
    (>= 8 (count + 3) 2^-53 at count <= 1024), C_d to 1e-11 of max|C_d|"""
    from beat_amd import covariance as cov
    coords, res, perc = gold[case + "_coords"], gold[case + "_res"], float(gold[case + "_perc"])
    radius, counts, stds = ctx.ball_rms_batch(coords, res, [res.size], perc)
    assert radius[0] == float(gold[case + "_radius"])
    assert np.array_equal(counts, gold[case + "_counts"])
    print("%s: device stds vs the reference's: worst relative difference %.3g"
          % (case, float(np.abs(stds / gold[case + "_stds"] - 1.0).max())))
    np.testing.assert_allclose(stds, gold[case + "_stds"], rtol=1e-12, atol=0.0)
    assert np.array_equal(cov.k_nearest_neighbor_rms(coords, res, max_dist_perc=perc), stds)
    ref = nref.scaled_toeplitz(gold[case + "_coeffs"], gold[case + "_stds"])
    Cd = cov.non_toeplitz_covariance_2d(coords, res, perc)
    err = float(np.abs(Cd - ref).max() / np.abs(ref).max())
    print("%s: device C_d vs the reference's: worst |difference| / max|C_d| = %.3g" % (case, err))
    assert Cd.shape == ref.shape and err <= 1e-11
    T, s = cov.toeplitz_covariance_2d(coords, res, perc)
    assert np.array_equal(s, stds) and np.array_equal(T * s[:, None] * s[None, :], Cd)
    dC = cov.non_toeplitz_covariance_2d_batch(_dev(coords, ctx), _dev(res, ctx), [res.size], perc)[0]
    assert dC.is_cuda and np.array_equal(dC.cpu().numpy(), Cd)


# ------------------------------------------------------------------------------------------------- the update
def _problem(coords, residuals, odw=None, ramps=False, seed=11):
    """a geodetic FFI problem whose residual ``d - mu - corrections`` at the point ``q_map`` is ``residuals`` (one array per
    dataset): seeded libraries, data = G.T slips (+ ramp) + residual, unit-scaled weights to start from ->
    (problem, layout, host arrays, Covariance objects, q_map)"""
    from beat_amd.ffi import GeodeticGFLibrary, GeodeticGFLibraryConfig
    from beat_amd.heart import Covariance
    from beat_amd.models import FFIProblem, GeodeticData, ParameterLayout, RampConfig
    rng = np.random.default_rng(seed)
    sizes = [r.size for r in residuals]
    nobs = sum(sizes)
    gfs, Gs = {}, []
    for v in SLIPS:
        gg = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=(NPATCH, nobs), component=v))
        gg.setup(NPATCH, nobs, allocate=True)
        gg._gfmatrix[:] = 0.02 * rng.standard_normal((NPATCH, nobs))
        gfs[v] = gg
        Gs.append(np.array(gg._gfmatrix))
    names = ["scene_%d" % d for d in range(len(sizes))]
    corrs, free = None, []
    if ramps:
        corrs = []
        for d in range(len(sizes)):
            c = RampConfig(dataset_names=names, enabled=True).init_correction()
            c.setup_correction(coords[d][:, 1], coords[d][:, 0], None, None, names[d])
            corrs.append([c])
            free += c.correction_names
    lay = ParameterLayout(OrderedDict([(v, NPATCH) for v in SLIPS] + [(n, 1) for n in free] + [("h_SAR", 1)]))
    lower = dict(uparr=0.0, uperp=0.0, h_SAR=-1.0, **dict((n, -2e-4) for n in free))
    upper = dict(uparr=3.0, uperp=3.0, h_SAR=1.0, **dict((n, 2e-4) for n in free))
    q_map = np.zeros(lay.size)
    mu = np.zeros(nobs)
    for G, v in zip(Gs, SLIPS):
        s = rng.uniform(0.0, 3.0, NPATCH)
        q_map[lay.offsets[v]:lay.offsets[v] + NPATCH] = s
        mu += G.T @ s
    for n in free:
        q_map[lay.offsets[n]] = rng.uniform(-1e-4, 1e-4)
    data = mu + np.concatenate(residuals)
    if ramps:
        pt = lay.rmap(q_map)
        data += np.concatenate([c[0].get_displacements(None, point=pt) for c in corrs])
    odw = np.ones(nobs) if odw is None else odw
    covs = [Covariance(data=4e-6 * np.eye(n)) for n in sizes]
    W = [c.chol_inverse for c in covs]
    sl = [float(c.log_pdet) for c in covs]
    geo = GeodeticData(gfs, data, odw, sizes, W, sl, [("h_SAR", 0)] * len(sizes), corrections=corrs)
    prob = FFIProblem(lay, [], [], [], SLIPS, geodetic=geo, lower=lower, upper=upper)
    host = dict(Gs=Gs, data=data, odw=odw, sizes=sizes, W=W, sl=sl, corrections=corrs)
    return prob, lay, host, covs, q_map


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


def _laquila(gold, **kw):
    return _problem([gold["laq0_coords"], gold["laq1_coords"]], [gold["laq0_res"], gold["laq1_res"]], **kw)


def test_the_lone_point(ctx, gold):
    """NaN at the lone point's index only; the update raises the reference's ValueError naming the dataset and leaves
    weights, likelihoods and the Covariance objects bitwise what they were"""
    from beat_amd.covariance import GeodeticNoiseCovarianceUpdate
    coords, res = gold["lone_coords"], gold["lone_res"]
    _, counts, stds = ctx.ball_rms_batch(coords, res, [res.size], float(gold["lone_perc"]))
    assert np.array_equal(counts, gold["lone_counts"]) and np.array_equal(np.isnan(stds), gold["lone_nan"])
    assert np.array_equal(np.nonzero(np.isnan(stds))[0], [17])
    # behind a scene that is fine at this fraction (the fixture's laq0 case)
    prob, lay, host, covs, q_map = _problem([gold["laq0_coords"], coords], [gold["laq0_res"], res])
    f = prob.compile(ctx)
    Q = _population(lay, prob.lower, prob.upper, 4)
    L0 = np.asarray(f.batch(Q)).copy()
    W0 = [w.copy() for w in host["W"]]
    datas = [c._terms["data"] for c in covs]
    upd = GeodeticNoiseCovarianceUpdate(f, [gold["laq0_coords"], coords], covs, float(gold["lone_perc"]))
    with pytest.raises(ValueError, match="Estimated Non-Toeplitz covariance matrix for dataset 1 contains Nan! "
                                         "Please increase 'max_dist_perc'!"):
        upd.update_weights(q_map)
    assert upd.n_updates == 0
    assert np.array_equal(np.asarray(f.batch(Q)), L0)
    for d in range(2):
        assert np.array_equal(np.asarray(f.problem.geodetic.weights[d]), W0[d])
        assert covs[d]._terms["data"] is datas[d] and float(covs[d].slog_pdet.get_value()) == host["sl"][d]
    f.release()


def test_update_end_to_end_on_the_laquila_sized_scenes(ctx, gold):
    """after update_weights at the seeded point: slog_pdet against the reference's at rtol 1e-9; the likelihood vectors of
    4 chains against the one-chain oracle with heart.Covariance(data=C_d of the fixture).chol_inverse at rtol 1e-6, like at
    1e-8 (test_gpu_predcov.py's tolerances)"""
    from beat_amd.covariance import GeodeticNoiseCovarianceUpdate
    from beat_amd.heart import Covariance
    prob, lay, host, covs, q_map = _laquila(gold)
    f = prob.compile(ctx)
    Q = _population(lay, prob.lower, prob.upper, 4)
    L0 = np.asarray(f.batch(Q)).copy()
    upd = GeodeticNoiseCovarianceUpdate(f, [gold["laq0_coords"], gold["laq1_coords"]], covs, 0.2)
    res = upd.residuals(q_map).cpu().numpy()
    np.testing.assert_allclose(res, np.concatenate([gold["laq0_res"], gold["laq1_res"]]), rtol=0, atol=1e-15)
    upd.update_weights(q_map)
    assert upd.n_updates == 1 and upd.n_host_route == 0 and upd.last_ms > 0
    Wr, slr = [], []
    for c in ("laq0", "laq1"):
        ref = Covariance(data=nref.scaled_toeplitz(gold[c + "_coeffs"], gold[c + "_stds"]))
        Wr.append(ref.chol_inverse)
        slr.append(float(ref.log_pdet))
        np.testing.assert_allclose(slr[-1], float(gold[c + "_logpdet"]), rtol=1e-9)
    L1 = np.asarray(f.batch(Q))
    for c in range(4):
        ref = _ffi_ref(host, lay, Q[c], Wr, slr)
        np.testing.assert_allclose(L1[c], ref, rtol=1e-6)
        np.testing.assert_allclose(L1[c, -1], ref[-1], rtol=1e-8)
    assert not np.allclose(L0[:, -1], L1[:, -1])
    g = f.problem.geodetic
    for d, c in enumerate(("laq0", "laq1")):
        np.testing.assert_allclose(g.slog_pdets[d], float(gold[c + "_logpdet"]), rtol=1e-9)
        assert float(covs[d].slog_pdet.get_value()) == g.slog_pdets[d]
        # cov.data: the new term, left on the device until read
        assert hasattr(covs[d]._terms["data"], "is_cuda")
        Cd = covs[d].data
        ref = nref.scaled_toeplitz(gold[c + "_coeffs"], gold[c + "_stds"])
        assert isinstance(Cd, np.ndarray) and np.abs(Cd - ref).max() <= 1e-11 * np.abs(ref).max()
    f.release()


def test_residual_has_no_odw_and_takes_the_ramp_off(ctx, gold):
    """odw != 1 and a ramp on each scene: the estimated C_d is bit for bit the one of the hand-formed d - mu - ramp (mu
    the model's own, the ramp's columns times the point's coefficients, added in column order), and not the one of the
    weighted residual"""
    from beat_amd import covariance as cov
    rng = np.random.default_rng(8)
    odw = 0.5 + rng.random(419)
    coords = [gold["laq0_coords"], gold["laq1_coords"]]
    prob, lay, host, covs, q_map = _laquila(gold, odw=odw, ramps=True)
    f = prob.compile(ctx)
    upd = cov.GeodeticNoiseCovarianceUpdate(f, coords, covs, 0.2)
    upd.update_weights(q_map)
    assert upd.n_host_route == 0
    mu = np.asarray(f.geodetic_residuals(q_map[None, :], residuals=False))[0]
    hand = host["data"] - mu
    o = 0
    for d, n in enumerate(host["sizes"]):
        c = host["corrections"][d][0]
        B = c.basis()
        coef = [q_map[lay.offsets[name]] for name in c.correction_names]
        ramp = B[:, 0] * coef[0]
        for k in (1, 2):
            ramp = ramp + B[:, k] * coef[k]
        hand[o:o + n] = hand[o:o + n] - ramp
        o += n
    assert np.array_equal(upd.residuals(q_map).cpu().numpy(), hand)
    # the residual is the fixture's up to the rounding of forming data = mu + ramp + residual on the host
    np.testing.assert_allclose(hand, np.concatenate([gold["laq0_res"], gold["laq1_res"]]), rtol=0, atol=1e-15)
    want = cov.non_toeplitz_covariance_2d_batch(np.concatenate(coords), hand, host["sizes"], 0.2)
    weighted = cov.non_toeplitz_covariance_2d_batch(np.concatenate(coords), hand * odw, host["sizes"], 0.2)
    for d in range(2):
        assert np.array_equal(covs[d].data, want[d])
        assert not np.array_equal(covs[d].data, weighted[d])
        np.testing.assert_allclose(f.problem.geodetic.slog_pdets[d], float(gold["laq%d_logpdet" % d]), rtol=1e-9)
    f.release()


def test_velocity_in_the_same_pass_vs_the_sequential_updates(ctx, gold):
    """``velocity=``: data term, pred_v from the ensemble at the same point, ONE factorisation per dataset -- operators and
    log-determinants bitwise those of CovarianceUpdates(noise, velocity), which factorises twice (counted through the
    context's kernel timing)"""
    from beat_amd.covariance import CovarianceUpdates, GeodeticNoiseCovarianceUpdate, VelocityModelCovarianceUpdate
    coords = [gold["laq0_coords"], gold["laq1_coords"]]
    out = []
    ctx.enable_timing(True)
    try:
        for fused in (True, False):
            prob, lay, host, covs, q_map = _laquila(gold)
            f = prob.compile(ctx)
            ens = crust_ensemble(prob.geodetic.gfs, SLIPS, 7)
            vel = VelocityModelCovarianceUpdate(f, ens, covs)
            if fused:
                upd = GeodeticNoiseCovarianceUpdate(f, coords, covs, 0.2, velocity=vel)
            else:
                upd = CovarianceUpdates(GeodeticNoiseCovarianceUpdate(f, coords, covs, 0.2), vel)
            ctx.synchronize()
            ctx.reset_timing()
            upd.update_weights(q_map)
            ctx.synchronize()
            nchol = ctx.kernel_time("chol_inverse")[1]
            g = f.problem.geodetic
            out.append(dict(W=[w.cpu().numpy() for w in g.weights], sl=list(g.slog_pdets), nchol=nchol,
                            data=[c.data for c in covs], pv=[c.pred_v for c in covs],
                            slog=[float(c.slog_pdet.get_value()) for c in covs], vel=vel, upd=upd))
            f.release()
            ens.release()
    finally:
        ctx.enable_timing(False)
    one, two = out
    assert one["nchol"] == 2 and two["nchol"] == 4
    assert one["vel"].n_updates == two["vel"].n_updates == 1 and one["upd"].n_updates == 1
    assert one["upd"].n_host_route == 0 and two["vel"].n_host_route == 0
    for d in range(2):
        assert np.array_equal(one["W"][d], two["W"][d]) and one["sl"][d] == two["sl"][d] == one["slog"][d] == two["slog"][d]
        assert np.array_equal(one["data"][d], two["data"][d]) and np.array_equal(one["pv"][d], two["pv"][d])
        assert np.isfinite(one["W"][d]).all() and not np.tril(one["W"][d], -1).any()
        # pred_v moved the weights: not the data term's factorisation alone
        assert one["sl"][d] != float(gold["laq%d_logpdet" % d])


def test_velocity_accepts_a_device_resident_data_term(ctx, gold):
    """the base of the velocity update with ``Covariance.data`` on the device is that tensor itself (no pred_g): no host
    round trip, and the operators are bitwise those from the same matrices as host arrays"""
    import torch
    from beat_amd.covariance import VelocityModelCovarianceUpdate
    from beat_amd.heart import Covariance
    prob, lay, host, covs, q_map = _problem([gold["n30_coords"], gold["n33_coords"]], [gold["n30_res"], gold["n33_res"]])
    f = prob.compile(ctx)
    ens = crust_ensemble(prob.geodetic.gfs, SLIPS, 7)
    VelocityModelCovarianceUpdate(f, ens, covs).update_weights(q_map)
    W_host = [w.cpu().numpy() for w in f.problem.geodetic.weights]
    dev_terms = [_dev(c.data, ctx) for c in covs]
    dcovs = [Covariance() for _ in covs]
    for c, t in zip(dcovs, dev_terms):
        c.data = t
    vel = VelocityModelCovarianceUpdate(f, ens, dcovs)
    base = vel._bases(torch.device("cuda", ctx.device))
    assert all(b is t for b, t in zip(base, dev_terms))
    vel.update_weights(q_map)
    assert all(c._terms["data"] is t for c, t in zip(dcovs, dev_terms))            # still on the device: never read
    for d in range(2):
        assert np.array_equal(f.problem.geodetic.weights[d].cpu().numpy(), W_host[d])
    f.release()
    ens.release()


# ------------------------------------------------------------------------------------------------- sampler
def test_sampler_runs_the_update_every_stage(ctx):
    """smc_sample(update=GeodeticNoiseCovarianceUpdate) on the small joint problem: 96 chains, 3 stages; the update runs
    once per stage and once after the initial stage, all likelihoods finite, cov.data readable as numpy afterwards"""
    import torch
    from beat_amd.covariance import GeodeticNoiseCovarianceUpdate
    from beat_amd.sampler import SMC, smc_sample
    spec, prob, host, covs = joint_problem()
    sizes = prob.geodetic.sizes
    rng = np.random.default_rng(12)
    coords = [rng.uniform(-20e3, 20e3, (n, 2)) for n in sizes]
    for c, n in zip(coords, sizes):                  # every point has a neighbour: counts depend on the coordinates alone
        assert nref.ball_rms(c, np.arange(float(n)), 0.5)[1].min() >= 3
    f = prob.compile(ctx)
    lo, up = host["layout"].bounds(host["lower"], host["upper"])
    step = SMC(f, lo, up, n_chains=96, device=torch.device("cuda", 0), random_seed=4, tune_interval=3)
    upd = GeodeticNoiseCovarianceUpdate(f, coords, covs, 0.5)
    seen = []
    pop, lp, betas = smc_sample(3, step, max_stages=3, update=upd, on_stage=lambda s: seen.append(s.likelihoods.copy()))
    assert upd.n_updates == len(seen) + 1 >= 3
    assert all(np.isfinite(x).all() for x in seen) and np.isfinite(lp[:, -1]).all()
    for cov, n in zip(covs, sizes):
        Cd = cov.data
        assert isinstance(Cd, np.ndarray) and Cd.shape == (n, n) and np.isfinite(Cd).all()
        assert np.isfinite(float(cov.slog_pdet.get_value()))
    f.release()
