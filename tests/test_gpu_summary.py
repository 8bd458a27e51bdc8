"""Posterior diagnostics on the device (csrc/summary.hip, beat_amd/summary.py): variance reductions against the one-chain
composition of the existing oracle functions, the cached denominators and their invalidation, the geodetic residuals of
both composites, standardized residuals against numpy and the reference's numbers (tests/golden/summary.npz), the
running ensemble moments against the numpy restatement (tests/summary_ref.py), and ``result_ensemble`` end to end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import summary_ref as sref  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from oracle import problem_oracle  # noqa: E402
from test_gpu_hypers import _check_chains, _dev, _expected_llks, _geom_parts, _specs  # noqa: E402

pytestmark = pytest.mark.gpu

VARIANTS = [("scalar_nn", "plain"), ("toeplitz_ml", "band"), ("toeplitz_ml", "dense"), ("toeplitz_ml", "prewhitened")]


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


def _compiled(ctx, name, variant):
    """the problems of tests/test_gpu_hypers.py::_specs in the four ways a wavemap's weight set is evaluated"""
    from beat_amd.synthetic import build_problem
    spec = _specs()[name]
    prob, host = build_problem(spec)
    if variant == "dense":
        rng = np.random.default_rng(11)
        W = np.asarray(host["weights"]) + 0.05 * rng.standard_normal(np.shape(host["weights"]))
        host["weights"] = prob.wavemaps[0].weights = W
    f = prob.compile(ctx, prewhiten=(variant == "prewhitened"))
    if variant == "band":
        assert ctx.weights_band(f._wsets[0]) == 1
    elif variant == "dense":
        assert ctx.weights_band(f._wsets[0]) == -1
    elif variant == "prewhitened":
        assert prob.wavemaps[0].is_prewhitened
    return spec, prob, host, f


def _host_denominators(host):
    """|W_k d_k|^2 per dataset from the host weights, the data and godw"""
    spec = host["spec"]
    out = [sref.quad(host["weights"][t], host["data"][t]) for t in range(spec.T)]
    o = 0
    for n, W in zip(spec.geodetic_nobs or (), host.get("gW", ())):
        out.append(sref.quad(W, (host["gdata"] * host["godw"])[o:o + n]))
        o += n
    return np.array(out)


# ------------------------------------------------------------------------------------------------- 1 variance reductions
@pytest.mark.parametrize("C", [1, 63, 64, 530])
@pytest.mark.parametrize("name,variant", VARIANTS)
def test_1_variance_reductions_vs_one_chain_composition(ctx, name, variant, C):
    from beat_amd.synthetic import draw_population
    spec, prob, host, f = _compiled(ctx, name, variant)
    try:
        ndata = spec.T + len(spec.geodetic_nobs)
        assert f.ndata == ndata and len(f.dataset_names) == ndata
        Q = draw_population(spec, host["layout"], host["lower"], host["upper"], C)
        got = f.variance_reductions(Q)
        assert isinstance(got, np.ndarray) and got.shape == (C, ndata)
        dev = f.variance_reductions(_dev(Q, ctx))
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)
        Q2 = Q.copy()
        for k in host["layout"].varsizes:
            if k.startswith("h_"):
                o = host["layout"].offsets[k]
                Q2[:, o:o + host["layout"].varsizes[k]] = 123.0
        assert np.array_equal(f.variance_reductions(Q2), got)
        denom = _host_denominators(host)
        worst = 0.0
        for c in _check_chains(C):
            ratio = _expected_llks(host, Q[c])[:ndata] / denom
            worst = max(worst, float(np.max(np.abs((1.0 - got[c]) - ratio) / np.abs(ratio))))
            np.testing.assert_allclose(1.0 - got[c], ratio, rtol=1e-9)
        print("variance_reductions %s/%s C=%d: worst relative difference of 1 - VR %.3g" % (name, variant, C, worst))
    finally:
        f.release()


# ------------------------------------------------------------------------------------------------- 2 denominators
@pytest.mark.parametrize("name,variant", VARIANTS)
def test_2_obs_quads_are_wset_quad_on_the_data(ctx, name, variant):
    spec, prob, host, f = _compiled(ctx, name, variant)
    try:
        got = f.obs_quads()
        assert got.shape == (f.ndata,) and np.array_equal(got, f.obs_quads())
        wm, g = prob.wavemaps[0], prob.geodetic
        parts = [ctx.wset_quad_batch(f._wsets[0], wm.data[None])[0]]          # (a pre-whitened wavemap: its whitened data)
        dw, o = g.data * g.odws, 0
        for k, n in enumerate(g.sizes):
            parts.append(ctx.wset_quad_batch(f._geo_wsets[k], np.ascontiguousarray(dw[o:o + n]).reshape(1, 1, n))[0])
            o += n
        assert np.array_equal(got, np.concatenate(parts))
        np.testing.assert_allclose(got, _host_denominators(host), rtol=1e-9)
        import torch
        out = torch.empty(f.ndata, dtype=torch.float64, device="cuda:%d" % ctx.device)
        ctx.ffi_obs_quads(f.model_id, f.ndata, out=out)
        assert np.array_equal(out.cpu().numpy(), got)
    finally:
        f.release()


# ------------------------------------------------------------------------------------------------- 3 the reference's numbers
def test_3_fixture_through_the_device(ctx, golden):
    """weight sets from the reference's chol_inverse, wset_quad_batch on its r and d: 1 - nom / denom against the
    reference's variance reduction, absolute 1e-9 * max(1, nom / denom)"""
    g = golden("summary")
    worst = 0.0
    for key, n in sref.fixture_cases(g):
        W = np.ascontiguousarray(g[key + "_chol_inverse"]).reshape(1, n, n)
        ws = ctx.weights_create_dense(W, [0.0])
        try:
            X = np.stack([g[key + "_r"], g[key + "_d"]]).reshape(2, 1, n)
            q = ctx.wset_quad_batch(ws, X)
            assert q.shape == (2, 1)
            vr = 1.0 - q[0, 0] / q[1, 0]
            for i in range(len(g["hps"])):
                tol = 1e-9 * max(1.0, g[key + "_nom"][i] / g[key + "_denom"][i])
                worst = max(worst, abs(vr - g[key + "_vr"][i]) / tol)
                assert abs(vr - g[key + "_vr"][i]) <= tol, (key, i)
        finally:
            ctx.weights_destroy(ws)
    print("fixture through the device: worst |VR - reference| / tolerance = %.3g" % worst)


# ------------------------------------------------------------------------------------------------- 4 cache invalidation
@pytest.mark.parametrize("name,kind", [("scalar_nn", "scalar"), ("toeplitz_ml", "dense"), ("scalar_nn", "data")])
def test_4_cached_denominators_follow_weights_and_data(ctx, name, kind):
    from beat_amd.synthetic import build_problem, draw_population
    spec = _specs()[name]
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], 65)
    before, dq_before = f.variance_reductions(Q), f.obs_quads()
    rng = np.random.default_rng(5)
    prob2, _ = build_problem(spec)
    wm2 = prob2.wavemaps[0]
    if kind == "data":
        new = host["data"] + rng.standard_normal(host["data"].shape)
        ctx.ffi_model_update_data(f.model_id, 0, new)
        wm2.data = np.ascontiguousarray(new)
    else:
        w = np.asarray(host["weights"])
        new = w * (1.0 + 0.3 * rng.random(w.shape))        # (scalar: per dataset; dense: per entry, zeros stay zeros)
        f.update_weights(0, new, host["slog"])
        wm2.weights = new
    after, dq_after = f.variance_reductions(Q), f.obs_quads()
    f2 = prob2.compile(ctx)
    try:
        assert np.array_equal(dq_after, f2.obs_quads()) and not np.array_equal(dq_after[:spec.T], dq_before[:spec.T])
        assert np.array_equal(after, f2.variance_reductions(Q))
        if kind != "scalar":     # (a scalar weight cancels in the ratio up to rounding)
            assert not np.allclose(after[:, :spec.T], before[:, :spec.T], rtol=1e-6)
        assert np.array_equal(after[:, spec.T:], before[:, spec.T:])       # the geodetic columns did not move
    finally:
        f.release()
        f2.release()


# ------------------------------------------------------------------------------------------------- 5 geodetic composites
@pytest.mark.parametrize("C", [1, 530])
def test_5_ffi_geodetic_composite_with_ramps(ctx, C):
    from test_gpu_corrections import SLIPS, _corrected, _draw, _ffi_problem, _ramp, scenes
    sc = scenes()
    names = [s["name"] for s in sc]
    corrs = [[_ramp(names, s["name"], s["north"], s["east"])] for s in sc]
    free = [n for cs in corrs for c in cs for n in c.correction_names]
    prob, lay, host = _ffi_problem(sc, corrs, free)
    f = prob.compile(ctx)
    try:
        Q = _draw(lay, prob.lower, prob.upper, C, np.random.default_rng(5 + C))
        vr, res, mu = f.variance_reductions(Q), f.geodetic_residuals(Q), f.geodetic_residuals(Q, residuals=False)
        nobs = host["data"].size
        assert vr.shape == (C, 2) and res.shape == (C, nobs) and mu.shape == (C, nobs)
        dw, o, denom = host["data"] * host["odw"], 0, []
        for n, W in zip(host["sizes"], host["W"]):
            denom.append(sref.quad(W, dw[o:o + n]))
            o += n
        np.testing.assert_allclose(f.obs_quads(), denom, rtol=1e-9)
        for c in _check_chains(C):
            pt = lay.rmap(Q[c])
            m = np.zeros(nobs)
            for G, v in zip(host["Gs"], SLIPS):
                m += orc.geo_stack(G, pt[v])
            parts = _corrected((host["data"] - m) * host["odw"], host["sizes"], corrs, lambda n: pt[n][0])
            ref = np.concatenate(parts)
            np.testing.assert_allclose(mu[c], m, rtol=1e-9, atol=1e-9 * np.abs(m).max())
            np.testing.assert_allclose(res[c], ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())
            ratio = np.array([sref.quad(W, r) for W, r in zip(host["W"], parts)]) / denom
            np.testing.assert_allclose(1.0 - vr[c], ratio, rtol=1e-9)
        dres = f.geodetic_residuals(_dev(Q, ctx))
        assert dres.is_cuda and np.array_equal(dres.cpu().numpy(), res)
    finally:
        f.release()


@pytest.mark.parametrize("C", [1, 530])
def test_5_geometry_composite(ctx, C):
    from beat_amd.synthetic import build_geometry_problem
    prob, lay, lower, upper = build_geometry_problem(sizes=(60, 41))
    f = prob.compile(ctx)
    try:
        lo, up = lay.bounds(lower, upper)
        Q = lo + (up - lo) * np.random.default_rng(C).random((C, lay.size))
        vr, res, mu = f.variance_reductions(Q), f.geodetic_residuals(Q), f.geodetic_residuals(Q, residuals=False)
        assert vr.shape == (C, 2) and res.shape == (C, 101) and f.dataset_names == ["geo_like_0", "geo_like_1"]
        dw, o, denom = prob.data * prob.odws, 0, []
        for n, W in zip(prob.sizes, prob.weights):
            denom.append(sref.quad(W, dw[o:o + n]))
            o += n
        np.testing.assert_allclose(f.obs_quads(), denom, rtol=1e-9)
        # residual and synthetics are one kernel's two stores: the same mu
        np.testing.assert_allclose((prob.data - mu) * prob.odws, res, rtol=1e-12, atol=1e-12 * np.abs(res).max())
        for c in list(_check_chains(C))[::7] if C > 64 else range(C):
            parts = _geom_parts(prob, lay, Q[c])
            ref = np.concatenate(parts)
            np.testing.assert_allclose(res[c], ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())
            ratio = np.array([sref.quad(W, r) for W, r in zip(prob.weights, parts)]) / denom
            np.testing.assert_allclose(1.0 - vr[c], ratio, rtol=1e-9)
    finally:
        f.release()


def test_5_noop_corrections_are_the_uncorrected_model(ctx):
    from test_gpu_corrections import _draw, _ffi_problem, scenes
    sc = scenes()
    prob0, lay, _ = _ffi_problem(sc, None, [])
    prob1, _, _ = _ffi_problem(sc, [[], []], [])
    f0, f1 = prob0.compile(ctx), prob1.compile(ctx)
    try:
        Q = _draw(lay, prob0.lower, prob0.upper, 70, np.random.default_rng(2))
        assert np.array_equal(f0.variance_reductions(Q), f1.variance_reductions(Q))
        assert np.array_equal(f0.geodetic_residuals(Q), f1.geodetic_residuals(Q))
        assert np.array_equal(f0.obs_quads(), f1.obs_quads())
    finally:
        f0.release()
        f1.release()


# ------------------------------------------------------------------------------------------------- 6 flagged chains
def test_6_chain_outside_the_library_grid_is_nan_and_raises(ctx):
    from beat_amd.synthetic import build_problem, draw_population
    spec = _specs()["scalar_nn"]
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    try:
        Q = draw_population(spec, host["layout"], host["lower"], host["upper"], 5)
        Q[2, host["layout"].offsets["durations"]] = 1e3
        Qd = _dev(Q, ctx)
        llks = f.update_llks(Qd)
        with pytest.raises(IndexError) as want:
            ctx.synchronize()
        got = f.variance_reductions(Qd)
        with pytest.raises(IndexError) as have:
            ctx.synchronize()
        assert str(have.value) == str(want.value)
        got = got.cpu().numpy()
        assert np.isnan(got[2]).all() and np.isfinite(np.delete(got, 2, axis=0)).all()
        assert np.isnan(llks.cpu().numpy()[2]).all()
        with pytest.raises(IndexError):
            f.variance_reductions(Q)
    finally:
        f.release()


# ------------------------------------------------------------------------------------------------- 7 standardized residuals
def _operators(kind, T, N, rng):
    if kind == "scalar":
        return 0.5 + rng.random(T)
    S = rng.standard_normal((T, N, N)) / np.sqrt(N)
    if kind == "lower":
        S = np.tril(S) + 2.0 * np.eye(N)
    return np.ascontiguousarray(S)


@pytest.mark.parametrize("C", [1, 65, 530])
@pytest.mark.parametrize("N", [1, 33, 64, 130])
@pytest.mark.parametrize("kind", ["scalar", "lower", "full"])
def test_7_standardize_batch_vs_numpy(ctx, kind, N, C):
    T = 3
    rng = np.random.default_rng(1000 * N + C)
    S = _operators(kind, T, N, rng)
    R = rng.standard_normal((C, T, N))
    hp = rng.uniform(-2.3, 1.7, (C, T))
    for h in (None, hp):
        ref = sref.standardize_batch(S, R, h)
        got = ctx.standardize_batch(S, R, h)
        assert isinstance(got, np.ndarray) and got.shape == (C, T, N)
        assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max()
        dev = ctx.standardize_batch(_dev(S, ctx), _dev(R, ctx), None if h is None else _dev(h, ctx))
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)


def test_7_standardize_batch_vs_reference(ctx, golden):
    """the reference's inv(cov.chol(exp(2 hp))) . r: datasets = the fixture's covariance kinds, chains = its three hp"""
    g = golden("summary")
    hps = g["hps"]
    for n in g["sizes"]:
        keys = ["%s_%d" % (k, n) for k in g["kinds"]]
        S = np.stack([np.linalg.inv(sref.fixture_covariance(g, k).chol()) for k in keys])
        R = np.ascontiguousarray(np.broadcast_to(np.stack([g[k + "_r"] for k in keys]), (len(hps), len(keys), n)))
        hp = np.ascontiguousarray(np.broadcast_to(hps[:, None], (len(hps), len(keys))))
        got = ctx.standardize_batch(S, R, hp)
        for c in range(len(hps)):
            for t, k in enumerate(keys):
                ref = g[k + "_z_%d" % c]
                assert np.abs(got[c, t] - ref).max() <= 1e-9 * np.abs(ref).max(), (k, c)


def test_7_standardized_residuals_of_a_model(ctx):
    from beat_amd.heart import Covariance
    from beat_amd.synthetic import build_problem, draw_population
    spec = _specs()["toeplitz_ml"]
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    try:
        C = 70
        Q = draw_population(spec, host["layout"], host["lower"], host["upper"], C)
        covs = []
        for W in host["weights"]:
            Cm = np.linalg.inv(W.T @ W)
            covs.append(Covariance(data=0.5 * (Cm + Cm.T)))
        got = f.standardized_residuals(Q, covs)
        assert got.shape == (C, spec.T, spec.N)
        lay = host["layout"]
        for c in _check_chains(C):
            _, ex = problem_oracle.forward(host, Q[c])
            r = host["data"] - ex["synthetics"]
            for t, (hname, hidx) in enumerate(host["hypers"]):
                h = Q[c, lay.offset(hname, hidx)]
                ref = np.linalg.inv(covs[t].chol(np.exp(2.0 * h))) @ r[t]
                assert np.abs(got[c, t] - ref).max() <= 1e-9 * np.abs(ref).max()
        # the geodetic datasets: inv(chol(C_k)) on the composite's residual
        gcovs = []
        for W in host["gW"]:
            Cm = np.linalg.inv(W.T @ W)
            gcovs.append(Covariance(data=0.5 * (Cm + Cm.T)))
        zg = f.standardized_residuals(Q, gcovs, "geodetic")
        res = f.geodetic_residuals(Q)
        o = 0
        for k, n in enumerate(spec.geodetic_nobs):
            h = Q[:, lay.offset(*host["ghyp"][k])]
            ref = np.exp(-h)[:, None] * (res[:, o:o + n] @ np.linalg.inv(gcovs[k].chol()).T)
            assert zg[k].shape == (C, n) and np.abs(zg[k] - ref).max() <= 1e-9 * np.abs(ref).max()
            o += n
    finally:
        f.release()
    prob2, _ = build_problem(spec)
    f2 = prob2.compile(ctx, prewhiten=True)
    try:
        with pytest.raises(ValueError, match="pre-whitened"):
            f2.standardized_residuals(Q, covs)
    finally:
        f2.release()


# ------------------------------------------------------------------------------------------------- 8 ensemble moments
@pytest.mark.parametrize("M", [1, 63, 64, 65, 99, 390])
@pytest.mark.parametrize("C", [1, 2, 65, 530])
def test_8_ensemble_moments(ctx, C, M):
    rng = np.random.default_rng(100 * C + M)
    X = rng.standard_normal((C, M)) * 10.0 ** rng.uniform(-2, 2, M) + rng.uniform(-50, 50, M)
    state, n = ctx.ensemble_moments_update(X)
    assert n == C and state.shape == (5, M)
    mean, std, mn, mx = ctx.ensemble_moments_finish(state, n)
    assert np.array_equal(mn, X.min(0)) and np.array_equal(mx, X.max(0))
    rmean, rstd = sref.two_pass(X)
    bound = sref.moments_bound(X)
    print("ensemble_moments C=%d M=%d: worst |difference| / bound: mean %.3g, std %.3g; equal to the numpy recurrence: %s"
          % (C, M, (np.abs(mean - rmean) / bound).max(), (np.abs(std - rstd) / bound).max(),
             np.array_equal(state, sref.welford_update(X)[0])))
    assert np.all(np.abs(mean - rmean) <= bound) and np.all(np.abs(std - rstd) <= bound)
    dstate, dn = ctx.ensemble_moments_update(_dev(X, ctx))
    assert dstate.is_cuda and dn == C and np.array_equal(dstate.cpu().numpy(), state)
    for a, b in zip(ctx.ensemble_moments_finish(dstate, dn), (mean, std, mn, mx)):
        assert np.array_equal(a.cpu().numpy(), b)
    if C == 530:
        for Xs in (X, _dev(X, ctx)):
            st, seen = None, 0
            for a, b in ((0, 1), (1, 65), (65, 530)):
                st, seen = ctx.ensemble_moments_update(Xs[a:b], st, seen)
            assert seen == C and np.array_equal(st if isinstance(st, np.ndarray) else st.cpu().numpy(), state)


def test_8_nan_poisons_its_column_only(ctx):
    X = np.random.default_rng(0).standard_normal((9, 6))
    X[3, 2] = np.nan
    state, n = ctx.ensemble_moments_update(X)
    mean, std, _, _ = ctx.ensemble_moments_finish(state, n)
    assert np.isnan(mean[2]) and np.isnan(std[2])
    assert np.isfinite(np.delete(mean, 2)).all() and np.isfinite(np.delete(std, 2)).all()


# ------------------------------------------------------------------------------------------------- 9 result_ensemble
def test_9_result_ensemble(ctx):
    from beat_amd.summary import ensemble_indices, posterior_variance_reductions, result_ensemble
    from beat_amd.synthetic import build_problem, draw_population
    spec = _specs()["toeplitz_ml"]
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    try:
        n, E = 530, 7
        pop = draw_population(spec, host["layout"], host["lower"], host["upper"], n)
        best = pop[17]
        idx, vr, moments = result_ensemble(f, pop, best, E, keep_synthetics=True)
        assert np.array_equal(idx, ensemble_indices(n, E)) and idx.size == 7 and idx.max() < n
        assert vr.shape == (E + 1, f.ndata)
        rows = np.concatenate([[17], idx])
        assert np.array_equal(vr, 100.0 * f.variance_reductions(pop[rows]))          # the same batch: the same bits
        # against the whole population in one batch (test 1's values): the stacking kernel and with it the order of
        # the sums is chosen by the batch size; both sides are within 1e-9 of the one-chain composition in 1 - VR
        allvr = f.variance_reductions(pop)
        np.testing.assert_allclose(1.0 - vr / 100.0, 1.0 - allvr[rows], rtol=2e-9)
        byhand = np.concatenate([f.variance_reductions(pop[a:a + 100]) for a in range(0, n, 100)])
        assert np.array_equal(posterior_variance_reductions(f, pop, batch=100), byhand)
        np.testing.assert_allclose(1.0 - byhand, 1.0 - allvr, rtol=2e-9)
        syn = f.synthetics(_dev(pop[idx], ctx))
        state, seen = ctx.ensemble_moments_update(syn.view(E, -1))
        ref = [a.cpu().numpy().reshape(spec.T, spec.N) for a in ctx.ensemble_moments_finish(state, seen)]
        m = moments[0]
        for key, r in zip(("mean", "std", "min", "max"), ref):
            assert m[key].shape == (spec.T, spec.N) and np.array_equal(m[key], r)
        assert np.array_equal(m["synthetics"], syn.cpu().numpy())
        np.testing.assert_allclose(m["mean"], m["synthetics"].mean(0), rtol=0,
                                   atol=E * 2.0 ** -52 * np.abs(m["synthetics"]).max())
        _, _, lean = result_ensemble(f, pop, best, E)
        assert "synthetics" not in lean[0] and np.array_equal(lean[0]["mean"], m["mean"])
    finally:
        f.release()
