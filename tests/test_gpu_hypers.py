"""Hyper-parameter estimation on the device (csrc/hyper.hip, beat_amd/models/hypers.py): the cached misfits against
the one-chain composition of the existing oracle functions, the hyper model against the full model at a fixed source
point and against the numpy restatement (tests/hyper_ref.py, pinned to the reference's numbers by
tests/test_hypers_host.py), the one-launch chain against the step-by-step path bit for bit, its law, and
``estimate_hypers`` end to end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hyper_ref as href  # noqa: E402
from oracle import okada_oracle as ok  # noqa: E402
from oracle import problem_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

LOG_2PI = np.log(2.0 * np.pi)


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


def _dev(a, ctx, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to("cuda:%d" % ctx.device)


def _check_chains(C):
    return range(C) if C <= 64 else sorted(set(list(range(0, C, 41)) + [63, 64, 65, C - 2, C - 1]))


# ------------------------------------------------------------------------------------------------- G1 update_llks
def _specs():
    from beat_amd.synthetic import SyntheticSpec
    return {
        # scalar covariance, station shifts, nearest neighbour, geodetic composite, Laplacian with two slip variables
        "scalar_nn": SyntheticSpec((5,), (4,), (1.0,), T=3, N=33, D=3, S=40, slip_varnames=("uparr", "uperp"),
                                   covariance="scalar", station_shifts=True, geodetic_nobs=(9, 14), laplacian=True,
                                   hp_specific=True),
        # the "exponential" Toeplitz structure (bidiagonal operator), multilinear, station shifts
        "toeplitz_ml": SyntheticSpec((4,), (5,), (1.0,), T=3, N=64, D=3, S=40, slip_varnames=("uparr", "uperp"),
                                     covariance="toeplitz", station_shifts=True, geodetic_nobs=(21, 17),
                                     interpolation="multilinear"),
    }


def _expected_llks(host, q):
    """numpy |W r|^2 per dataset on the residuals of the existing oracle functions, |L s_v|^2 per slip variable"""
    spec, lay = host["spec"], host["layout"]
    _, ex = problem_oracle.forward(host, q)
    pt = lay.rmap(np.asarray(q))
    out = []
    if spec.T > 0:
        r = host["data"] - ex["synthetics"]
        for t in range(spec.T):
            W = host["weights"][t]
            wr = W * r[t] if np.ndim(W) == 0 else W @ r[t]
            out.append(float(wr @ wr))
    if spec.geodetic_nobs:
        res = (host["gdata"] - ex["mu"]) * host["godw"]
        o = 0
        for n, W in zip(spec.geodetic_nobs, host["gW"]):
            wr = W @ res[o:o + n]
            out.append(float(wr @ wr))
            o += n
    if spec.laplacian:
        for v in spec.slip_varnames:
            ls = host["L"] @ pt[v]
            out.append(float(ls @ ls))
    return np.array(out)


@pytest.mark.parametrize("C", [1, 63, 64, 530])
@pytest.mark.parametrize("name,variant", [("scalar_nn", "plain"), ("toeplitz_ml", "band"), ("toeplitz_ml", "dense"),
                                          ("toeplitz_ml", "prewhitened")])
def test_g1_update_llks_vs_one_chain_composition(ctx, name, variant, C):
    from beat_amd.synthetic import build_problem, draw_population
    spec = _specs()[name]
    prob, host = build_problem(spec)
    if variant == "dense":
        # operators with entries everywhere (no band, not triangular): the dense W through the matrix-core quadratic form
        rng = np.random.default_rng(11)
        W = np.asarray(host["weights"]) + 0.05 * rng.standard_normal(np.shape(host["weights"]))
        host["weights"] = prob.wavemaps[0].weights = W
    f = prob.compile(ctx, prewhiten=(variant == "prewhitened"))
    try:
        # the path the weight set takes is decided by its kind and its detected band (model.cpp wset_quad / ffi_logp_device)
        wm = prob.wavemaps[0]
        if variant == "plain":
            assert np.ndim(wm.weights) == 1 and not wm.is_prewhitened
        elif variant == "band":
            assert ctx.weights_band(f._wsets[0]) == 1
        elif variant == "dense":
            assert ctx.weights_band(f._wsets[0]) == -1
        else:
            assert wm.is_prewhitened and np.ndim(wm.weights) == 1 and np.all(np.asarray(wm.weights) == 1.0)
        Q = draw_population(spec, host["layout"], host["lower"], host["upper"], C)
        nterm = spec.T + len(spec.geodetic_nobs or ()) + (len(spec.slip_varnames) if spec.laplacian else 0)
        assert f.nterm == nterm
        got = f.update_llks(Q)
        assert isinstance(got, np.ndarray) and got.shape == (C, nterm)
        dev = f.update_llks(_dev(Q, ctx))
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)
        # the hyper-parameter entries are not read
        Q2 = Q.copy()
        for k in host["layout"].varsizes:
            if k.startswith("h_"):
                o = host["layout"].offsets[k]
                Q2[:, o:o + host["layout"].varsizes[k]] = 123.0
        assert np.array_equal(f.update_llks(Q2), got)
        worst = 0.0
        for c in _check_chains(C):
            ref = _expected_llks(host, Q[c])
            worst = max(worst, float(np.max(np.abs(got[c] - ref) / np.abs(ref))))
            np.testing.assert_allclose(got[c], ref, rtol=1e-9)
        print("update_llks %s/%s C=%d: worst relative difference %.3g" % (name, variant, C, worst))
    finally:
        f.release()


def test_g1_chain_outside_the_library_grid_is_nan_and_raises(ctx):
    from beat_amd.synthetic import build_problem, draw_population
    spec = _specs()["scalar_nn"]
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], 5)
    o = host["layout"].offsets["durations"]
    Q[2, o] = 1e3
    Qd = _dev(Q, ctx)
    got = f.update_llks(Qd)
    with pytest.raises(IndexError):
        ctx.synchronize()
    got = got.cpu().numpy()
    assert np.isnan(got[2]).all() and np.isfinite(np.delete(got, 2, axis=0)).all()
    f.release()


def _geom_parts(prob, lay, q):
    """the corrected weighted residual of the geometry composite, dataset by dataset (as tests/test_gpu_corrections.py
    composes it from the existing oracle functions)"""
    from test_gpu_corrections import _corrected
    pt = lay.rmap(q)
    mu = np.zeros(prob.east.size)
    for s, kind in enumerate(prob.sources):
        def val(name):
            if name in lay.offsets:
                return pt[name][s if lay.varsizes[name] > 1 else 0]
            return np.atleast_1d(prob.fixed.get(name, 0.0))[min(s, np.size(prob.fixed.get(name, 0.0)) - 1)]
        if kind == "mogi":
            ue, un, uz = ok.mogi(prob.east, prob.north, val("east_shift"), val("north_shift"), val("depth"), val("slip"),
                                 prob.nu)
        else:
            ue, un, uz = ok.rect_source(prob.east, prob.north, val("east_shift"), val("north_shift"), val("depth"),
                                        val("strike"), val("dip"), val("rake"), val("length"), val("width"), val("slip"),
                                        val("opening_fraction"), prob.nu)
        mu += (un * prob.los[:, 0] + ue * prob.los[:, 1]) + uz * prob.los[:, 2]
    res = (prob.data - mu) * prob.odws
    return _corrected(res, prob.sizes, prob.corrections, lambda n: pt[n][0] if n in lay.offsets else float(prob.fixed[n]))


def test_g1_update_llks_geometry_composite_with_ramps(ctx):
    from test_gpu_corrections import _draw, _geometry_problem
    rng = np.random.default_rng(77)
    prob, lay, lower, upper = _geometry_problem(rng, (60, 41), True, (True, True))
    f = prob.compile(ctx)
    C = 70
    Q = _draw(lay, lower, upper, C, rng)
    Q[:, lay.offset("slip", 1)] *= 1e6
    got = f.update_llks(Q)
    assert got.shape == (C, 2)
    for c in range(0, C, 3):
        ref = [float((W @ r) @ (W @ r)) for W, r in zip(prob.weights, _geom_parts(prob, lay, Q[c]))]
        np.testing.assert_allclose(got[c], ref, rtol=1e-9)       # the tolerance of tests/test_geometry.py
    f.release()


@pytest.mark.parametrize("C", [1, 63, 64, 530])
def test_g1_update_llks_ffi_geodetic_with_ramps(ctx, C):
    """a geodetic composite with ramps on full-covariance scenes of a few hundred points (the small-dataset kernel with
    its misfit-only store: whole and ragged 16-chain tiles)"""
    from test_gpu_corrections import SLIPS, _corrected, _draw, _ffi_problem, _ramp, scenes
    from oracle import oracle as orc
    sc = scenes()
    names = [s["name"] for s in sc]
    corrs = [[_ramp(names, s["name"], s["north"], s["east"])] for s in sc]
    free = [n for cs in corrs for c in cs for n in c.correction_names]
    prob, lay, host = _ffi_problem(sc, corrs, free)
    f = prob.compile(ctx)
    Q = _draw(lay, prob.lower, prob.upper, C, np.random.default_rng(5 + C))
    got = f.update_llks(Q)
    assert got.shape == (C, 2)
    for c in _check_chains(C):
        pt = lay.rmap(Q[c])
        mu = np.zeros(host["data"].size)
        for G, v in zip(host["Gs"], SLIPS):
            mu += orc.geo_stack(G, pt[v])
        parts = _corrected((host["data"] - mu) * host["odw"], host["sizes"], corrs, lambda n: pt[n][0])
        ref = [float((W @ r) @ (W @ r)) for W, r in zip(host["W"], parts)]
        np.testing.assert_allclose(got[c], ref, rtol=1e-9)
    f.release()


# ------------------------------------------------------------------------------------------------- G2
@pytest.mark.parametrize("name", ["scalar_nn", "toeplitz_ml"])
def test_g2_hyper_model_is_the_full_model_at_a_fixed_source_point(ctx, name):
    from beat_amd.models import HyperModel
    from beat_amd.synthetic import build_problem, draw_population
    spec = _specs()[name]
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    hm = HyperModel(f)
    C = 130
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], C)     # h random inside the box
    LL = f.batch(Q)
    llks = f.update_llks(Q)
    hm.set_llks(llks)
    H = np.ascontiguousarray(Q[:, hm.full_index])
    LH = hm.batch(H)
    assert LH.shape == (C, hm.nllk)
    h = H[:, hm.hp_index]
    mag = 0.5 * (np.abs(hm.slog) + np.abs(hm.M * 2 * h) + hm.M * LOG_2PI + np.exp(-2 * h) * llks)
    bound = 16 * 2.0 ** -53 * mag
    nd = int((hm.kind == 0).sum())
    full = LH[:, :nd] - 0.5 * hm.M[:nd] * LOG_2PI
    worst = float(np.max(np.abs(full - LL[:, :nd]) / bound[:, :nd]))
    assert np.all(np.abs(full - LL[:, :nd]) <= bound[:, :nd])
    if spec.laplacian:
        lap = LH[:, nd:hm.nterm].sum(1)
        assert LL.shape[1] == nd + 2
        assert np.all(np.abs(lap - LL[:, nd]) <= bound[:, nd:].sum(1))
    print("hyper model vs full model (%s): worst |difference| / bound = %.3g" % (name, worst))
    hm.release()
    f.release()


# ------------------------------------------------------------------------------------------------- G3
@pytest.mark.parametrize("tag", ["shared", "specific"])
@pytest.mark.parametrize("C", [1, 64, 530])
def test_g3_hyper_logp_vs_numpy(ctx, golden, tag, C):
    from beat_amd.models import HyperModel
    g = golden("hypers")
    typs, names, Hfix, hp_index = href.fixture_tables(g, tag)
    n = len(typs)
    nh = Hfix.shape[1]
    # the fixture's datasets in two composites plus two Laplacian terms on an extra hyper-parameter
    M = np.concatenate([g["hn_samples"], [350, 350]])
    slog = np.concatenate([g["hn_slog"], [12.5, 12.5]])
    kind = np.concatenate([np.zeros(n, dtype=np.int32), [1, 1]])
    hpi = np.concatenate([hp_index, [nh, nh]])
    ends = [5, n, n + 2]
    hm = HyperModel.from_tables(nh + 1, M, slog, kind, hpi, ends, ctx=ctx)
    rng = np.random.default_rng(C)
    H = rng.uniform(-5.0, 5.0, (C, nh + 1))
    llks = 10.0 ** rng.uniform(-3.0, 7.0, (C, n + 2))
    hm.set_llks(llks)
    got = hm.batch(H)
    ref = href.logp(M, slog, kind, hpi, ends, H, llks)
    np.testing.assert_allclose(got, ref, rtol=1e-12)
    # device tensors give the same bits; NaN misfit -> NaN like, the other terms untouched
    llks[0, 3] = np.nan
    hm.set_llks(_dev(llks, ctx))
    got2 = hm.batch(_dev(H, ctx)).cpu().numpy()
    assert np.isnan(got2[0, 3]) and np.isnan(got2[0, -1])
    keep = np.ones(got.shape, dtype=bool)
    keep[0, 3] = keep[0, -1] = False
    assert np.array_equal(got2[keep], got[keep])
    hm.release()


# ------------------------------------------------------------------------------------------------- G4 .. G6
PROPOSALS = {0: "Normal", 1: "Cauchy", 2: "Laplace"}


def _chain_setup(ctx, nh, C, kind, first_chain=0, seed=12345, tune_interval=50):
    """HyperModel + BatchedMetropolis on the inputs of hyper_ref.chain_case; -> (hm, step, H, L) on the device"""
    import torch

    from beat_amd.models import HyperModel
    from beat_amd.sampler.metropolis import BatchedMetropolis
    model, llk, lower, upper = href.chain_case(nh)
    hm = HyperModel.from_tables(nh, *model, lower=lower, upper=upper, ctx=ctx)
    rng = np.random.default_rng(1)
    H0 = (lower + (upper - lower) * rng.random((first_chain + C, nh)))[first_chain:]
    hm.set_llks(_dev(np.broadcast_to(llk, (C, nh)).copy(), ctx))
    dev = torch.device("cuda", ctx.device)
    step = BatchedMetropolis(hm, lower, upper, C, device=dev, tune=tune_interval > 0, tune_interval=max(1, tune_interval),
                             scale=0.05, seed=seed, first_chain=first_chain)
    step.set_proposal(None, PROPOSALS[kind])
    H = _dev(H0, ctx)
    L = step.evaluate(H)
    return hm, step, H, L, H0


def _run(step, H, L, n_steps, bt, use_chain_batch):
    import torch
    step.use_chain_batch = use_chain_batch
    ndraws = -(-n_steps // bt)
    trace = torch.full((ndraws, H.shape[0], H.shape[1] + L.shape[1]), float("nan"), dtype=torch.float64, device=H.device)
    n_acc = torch.zeros((), dtype=torch.int64, device=H.device)
    step.run(H, L, 1.0, n_steps, n_acc, trace=trace, buffer_thinning=bt)
    return trace, n_acc


def _state(step, H, L, trace, n_acc):
    return dict(H=H.cpu().numpy(), L=L.cpu().numpy(), scaling=step.scaling.cpu().numpy(),
                acc=step.accepted_since_tune.cpu().numpy(), n_acc=int(n_acc.item()), trace=trace.cpu().numpy(),
                sut=step.steps_until_tune, total=step.n_steps_total)


def _assert_same(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("nh", [1, 3, 70])
@pytest.mark.parametrize("C", [1, 65, 530])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_g4_one_launch_equals_step_by_step(ctx, kind, C, nh):
    n_steps, bt = 257, 3
    hm, step, H, L, H0 = _chain_setup(ctx, nh, C, kind)
    before = H.clone()
    # step by step: draw, propose, k_hyper_logp, accept, tune -- and count what the branches saw
    import torch
    step.use_chain_batch = False
    trace_s = torch.full((-(-n_steps // bt), C, nh + hm.nllk), float("nan"), dtype=torch.float64, device=H.device)
    n_acc_s = torch.zeros((), dtype=torch.int64, device=H.device)
    inbox = 0
    for s in range(n_steps):
        step.step(H, L, 1.0, n_acc_s)
        inbox += int(hm._inb.sum().item())
        if (n_steps - 1 - s) % bt == 0:
            trace_s[(s - (n_steps - 1) % bt) // bt] = torch.cat([H, L], dim=1)
    slow = _state(step, H, L, trace_s, n_acc_s)
    out_share, acc_share = 1.0 - inbox / float(n_steps * C), slow["n_acc"] / float(n_steps * C)
    print("kind %d C %d nh %d: %.1f %% out of the box, %.1f %% accepted" % (kind, C, nh, 100 * out_share, 100 * acc_share))
    assert out_share >= 0.05 and acc_share >= 0.05
    # the same through BatchedMetropolis.run on the step path (the trace rule of the eager loop)
    hm1, step1, H1, L1, _ = _chain_setup(ctx, nh, C, kind)
    assert torch.equal(H1, before)
    tr1, na1 = _run(step1, H1, L1, n_steps, bt, use_chain_batch=False)
    _assert_same(slow, _state(step1, H1, L1, tr1, na1))
    # ONE launch
    hm2, step2, H2, L2, _ = _chain_setup(ctx, nh, C, kind)
    tr2, na2 = _run(step2, H2, L2, n_steps, bt, use_chain_batch=True)
    fast = _state(step2, H2, L2, tr2, na2)
    assert not np.isnan(fast["trace"]).any()
    _assert_same(slow, fast)
    for m in (hm, hm1, hm2):
        m.release()


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_g5_first_steps_equal_the_numpy_chain(ctx, kind):
    nh, C, n_steps = 3, 65, 40
    hm, step, H, L, H0 = _chain_setup(ctx, nh, C, kind)
    trace, n_acc = _run(step, H, L, n_steps, 1, use_chain_batch=True)
    model, llk, lower, upper = href.chain_case(nh)
    ref = href.chain(model, H0, np.broadcast_to(llk, (C, nh)), lower, upper, kind, np.ones(nh), seed=12345, n_steps=n_steps,
                     scaling=0.05, tune_interval=50)
    got = trace.cpu().numpy()
    prev = np.concatenate([H0[None], got[:-1, :, :nh]])
    moved = np.any(got[:, :, :nh] != prev, axis=2)
    assert np.array_equal(moved, ref["accepted"])
    assert int(n_acc.item()) == ref["n_accepted"] > 0
    np.testing.assert_allclose(got, ref["trace"], rtol=1e-12)
    hm.release()


@pytest.mark.parametrize("kind", [0, 2])
def test_g6_keyed_streams_split_by_chains_and_by_steps(ctx, kind):
    nh, C, n, bt = 3, 64, 130, 3
    hm, step, H, L, _ = _chain_setup(ctx, nh, C, kind)
    tr, na = _run(step, H, L, 2 * n, bt, use_chain_batch=True)
    whole = _state(step, H, L, tr, na)
    # chains [0, C/2) and [C/2, C) in two calls
    parts = []
    for a in (0, C // 2):
        hm_p, st_p, H_p, L_p, _ = _chain_setup(ctx, nh, C // 2, kind, first_chain=a)
        tr_p, na_p = _run(st_p, H_p, L_p, 2 * n, bt, use_chain_batch=True)
        parts.append(_state(st_p, H_p, L_p, tr_p, na_p))
        hm_p.release()
    for k in ("H", "L", "scaling", "acc"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
    assert np.array_equal(np.concatenate([p["trace"] for p in parts], axis=1), whole["trace"])
    assert parts[0]["n_acc"] + parts[1]["n_acc"] == whole["n_acc"]
    # 2n steps in one call == n + n with step0 and the carried tuning state (130 is no multiple of the interval)
    hm2, st2, H2, L2, _ = _chain_setup(ctx, nh, C, kind)
    tr_a, na_a = _run(st2, H2, L2, n, 1, use_chain_batch=True)
    assert st2.n_steps_total == n and st2.steps_until_tune == 50 - n % 50
    tr_b, na_b = _run(st2, H2, L2, n, 1, use_chain_batch=True)
    hm3, st3, H3, L3, _ = _chain_setup(ctx, nh, C, kind)
    tr_w, na_w = _run(st3, H3, L3, 2 * n, 1, use_chain_batch=True)
    two, one = _state(st2, H2, L2, tr_b, na_b), _state(st3, H3, L3, tr_w, na_w)
    assert np.array_equal(np.concatenate([tr_a.cpu().numpy(), two["trace"]]), one["trace"])
    assert int(na_a.item()) + two["n_acc"] == one["n_acc"]
    for k in ("H", "L", "scaling", "acc", "sut", "total"):
        assert np.array_equal(two[k], one[k]), k
    assert np.array_equal(one["trace"][(2 * n - 1) % bt::bt], whole["trace"])
    for m in (hm, hm2, hm3):
        m.release()


@pytest.mark.parametrize("nh,nterm,waves", [(300, 600, 2), (700, 1024, 1), (1024, 1024, 1)])
def test_g4_long_models_up_to_the_kernel_limit(ctx, nh, nterm, waves):
    """models whose chain state no longer fits four to a workgroup: two chains per workgroup, one chain per workgroup
    with more than 64 KB of LDS, and the limit itself (1024 hyper-parameters, 1024 terms) -- bit for bit the step path"""
    import torch

    from beat_amd.models import HyperModel
    from beat_amd.sampler.metropolis import BatchedMetropolis
    lds = lambda w: nterm * 24 + nh * 24 + w * (nh * 16 + nterm * 24)      # hyper_chain_lds (csrc/hyper.hip)
    assert max(w for w in (4, 2, 1) if w == 1 or lds(w) <= 64 * 1024) == waves and (lds(1) > 64 * 1024) == (nh >= 700)
    n_steps, bt, C = 120, 7, 5
    rng = np.random.default_rng(nh + nterm)
    M = rng.integers(30, 501, nterm)
    u = rng.uniform(-1.0, 3.0, nh)
    hpi = (np.arange(nterm) % nh).astype(np.int32)
    llk = M * np.exp(2.0 * u[hpi])                    # every term of a hyper-parameter has its mode at u
    kind = (np.arange(nterm) % 5 == 4).astype(np.int32)
    ends = [nterm // 3, nterm]
    lower, upper = u - 0.1, u + 0.1
    H0 = lower + (upper - lower) * rng.random((C, nh))
    res = []
    for use in (False, True):
        hm = HyperModel.from_tables(nh, M, np.full(nterm, 3.0), kind, hpi, ends, lower=lower, upper=upper, ctx=ctx)
        assert hm.chain_applicable()
        hm.set_llks(_dev(np.broadcast_to(llk, (C, nterm)).copy(), ctx))
        step = BatchedMetropolis(hm, lower, upper, C, device=torch.device("cuda", ctx.device), tune=True, tune_interval=10,
                                 scale=0.05, seed=99)
        step.set_proposal(None, "Normal")
        H = _dev(H0, ctx)
        L = step.evaluate(H)
        tr, na = _run(step, H, L, n_steps, bt, use_chain_batch=use)
        res.append(_state(step, H, L, tr, na))
        hm.release()
    _assert_same(res[0], res[1])
    moved = np.any(res[0]["H"] != H0, axis=1)
    print("nh %d nterm %d: %d moves in %d steps x %d chains, scaling %s" % (nh, nterm, res[0]["n_acc"], n_steps, C, res[0]["scaling"]))
    assert res[0]["n_acc"] > 0 and moved.any() and not np.isnan(res[1]["trace"]).any()


def test_g4_beyond_the_kernel_limits_the_step_path_is_taken(ctx):
    """more terms than a chain's wavefront holds: the entry refuses with a message, BatchedMetropolis.run steps"""
    import torch

    from beat_amd.models import HyperModel
    from beat_amd.sampler.metropolis import BatchedMetropolis
    nterm, nh, C = 1100, 2, 5
    rng = np.random.default_rng(2)
    M = rng.integers(30, 501, nterm)
    llk = M * np.exp(2.0 * rng.uniform(0.0, 1.0, nterm))
    hm = HyperModel.from_tables(nh, M, np.zeros(nterm), np.zeros(nterm, dtype=np.int32), np.arange(nterm) % nh, [nterm],
                                lower=[-3.0, -3.0], upper=[3.0, 3.0], ctx=ctx)
    assert not hm.chain_applicable()
    hm.set_llks(_dev(np.broadcast_to(llk, (C, nterm)).copy(), ctx))
    dev = torch.device("cuda", ctx.device)
    step = BatchedMetropolis(hm, hm.lower, hm.upper, C, device=dev, tune_interval=5, scale=0.05, seed=3)
    step.set_proposal(None, "Normal")
    H = _dev(rng.uniform(0.0, 1.0, (C, nh)), ctx)
    L = step.evaluate(H)
    np.testing.assert_allclose(L.cpu().numpy(), href.logp(M, np.zeros(nterm), np.zeros(nterm, dtype=int), np.arange(nterm) % nh,
                                                          [nterm], H.cpu().numpy(), np.broadcast_to(llk, (C, nterm))), rtol=1e-12)
    with pytest.raises(ValueError, match="step-by-step"):
        hm.chain_batch(H, L, 3, step.scaling, step.accepted_since_tune, step.lower, step.upper, 0, step.uscale, 3, 0, 0, 5, 5)
    n_acc = torch.zeros((), dtype=torch.int64, device=dev)
    step.run(H, L, 1.0, 12, n_acc)
    assert step.n_steps_total == 12 and int(n_acc.item()) > 0
    hm.release()


# ------------------------------------------------------------------------------------------------- G7 law
@pytest.mark.parametrize("M,llk", [(120, 250.0), (419, 9e4), (35, 3.0)])
def test_g7_law_of_one_term(ctx, M, llk):
    """with x = exp(-2h) the target is Gamma(M/2, rate llk/2): E[h] = -(psi(M/2) - ln(llk/2)) / 2, sd = sqrt(psi'(M/2)) / 2"""
    import torch
    from scipy.special import digamma, polygamma

    from beat_amd.models import HyperModel
    from beat_amd.sampler.metropolis import BatchedMetropolis
    C, n_steps = 512, 4000
    hm = HyperModel.from_tables(1, [M], [0.0], [0], [0], [1], lower=[-20.0], upper=[20.0], ctx=ctx)
    hm.set_llks(_dev(np.full((C, 1), llk), ctx))
    dev = torch.device("cuda", ctx.device)
    step = BatchedMetropolis(hm, [-20.0], [20.0], C, device=dev, tune=True, tune_interval=50, scale=1.0, seed=4242)
    step.set_proposal(None, "Normal")
    H = _dev(np.random.default_rng(8).uniform(-20.0, 20.0, (C, 1)), ctx)
    L = step.evaluate(H)
    trace, n_acc = _run(step, H, L, n_steps, 1, use_chain_batch=True)
    h = trace[n_steps // 2:, :, 0].cpu().numpy()
    mean, sd = -0.5 * (digamma(M / 2.0) - np.log(llk / 2.0)), 0.5 * np.sqrt(polygamma(1, M / 2.0))
    print("M %d llk %g: (mean - E[h]) / sd = %.4f, std / sd = %.4f, accepted %.1f %%"
          % (M, llk, (h.mean() - mean) / sd, h.std() / sd, 100.0 * int(n_acc.item()) / (C * n_steps)))
    assert abs(h.mean() - mean) <= 0.25 * sd
    assert 0.8 <= h.std() / sd <= 1.25
    hm.release()


# ------------------------------------------------------------------------------------------------- G8 end to end
def test_g8_estimate_hypers_end_to_end(ctx, tmp_path):
    from beat_amd.backend import NumpyChain
    from beat_amd.models import HyperModel, estimate_hypers
    from beat_amd.models.hypers import hyper_bounds
    from beat_amd.synthetic import SyntheticSpec, build_problem
    spec = SyntheticSpec((5,), (4,), (1.0,), T=3, N=33, D=3, S=25, slip_varnames=("uparr", "uperp"), geodetic_nobs=(9, 14),
                         laplacian=True, hp_specific=True)
    prob, host = build_problem(spec)
    for k in host["layout"].varsizes:
        if k.startswith("h_"):
            host["lower"][k], host["upper"][k] = -12.0, 12.0     # the box the estimate replaces
    f = prob.compile(ctx)
    C, n_steps = 64, 2000
    res = {}
    # (thinned: 2000 steps leave 667 draws, burn 0.3 of THOSE = 200, every third kept)
    for mode, use, kw in (("launch", True, {}), ("steps", False, {}),
                          ("thinned", True, dict(buffer_thinning=3, burn=0.3, thin=3))):
        home = str(tmp_path / mode)
        hm = HyperModel(f)
        bounds, trace = estimate_hypers(f, hm, n_chains=C, n_steps=n_steps, homepath=home, use_chain_batch=use, **kw)
        res[mode] = (bounds, trace.cpu().numpy(), home, hm.llks.cpu().numpy())
        # the bounds are the reference's arithmetic (hyper_bounds, pinned to the fixture by the CPU tests) on the trace
        tr = res[mode][1]
        assert tr.shape[0] == -(-n_steps // kw.get("buffer_thinning", 1))
        for name in hm.names:
            o, n = hm.layout.offsets[name], hm.layout.varsizes[name]
            assert bounds[name] == hyper_bounds(tr[:, :, o:o + n], burn=kw.get("burn", 0.5), thin=kw.get("thin", 2)), name
        if mode == "thinned":
            # every third draw of the full run, counted from the last one
            assert np.array_equal(tr, res["launch"][1][(n_steps - 1) % 3::3])
            d = tr[200::3, :, :hm.nh]
            assert bounds["h_laplacian"][0] == np.floor(d[:, :, -1].min()) - 2.0
        if mode == "launch":
            assert list(bounds) == hm.names == ["h_any_P_0_Z", "h_SAR", "h_laplacian"]
            modes = 0.5 * np.log(hm.llks.cpu().numpy() / hm.M)       # one term per hyper-parameter entry ...
            for name, (lower, upper, test) in bounds.items():
                assert lower == int(lower) and upper == int(upper) and test == (lower + upper) / 2.0
                terms = [k for k in range(hm.nterm) if hm.layout.offsets[name] <= hm.hp_index[k]
                         < hm.layout.offsets[name] + hm.layout.varsizes[name]]
                m = modes[:, terms]
                if name == "h_laplacian":                                 # ... but two on h_laplacian
                    ll = hm.llks.cpu().numpy()[:, terms]
                    m = 0.5 * np.log(ll.sum(1) / hm.M[terms].sum())
                assert lower <= m.min() and upper >= m.max(), (name, lower, upper, m.min(), m.max())
                assert -12.0 < lower and upper < 12.0
            # the chain files, read back through the backend, are the device trace
            tr = trace.cpu().numpy()
            assert tr.shape == (n_steps, C, hm.nh + hm.nllk)
            for c in (0, 17, C - 1):
                ch = NumpyChain.load(os.path.join(home, "hypers", "stage_1", "chain-%d.bin" % c))
                o = 0
                for name in hm.names:
                    n = hm.layout.varsizes[name]
                    assert np.array_equal(ch.get_values(name), tr[:, c, o:o + n])
                    o += n
                assert np.array_equal(ch.get_values("like"), tr[:, c, -1])
                assert np.array_equal(ch.get_values("seis_like"), tr[:, c, hm.nh:hm.nh + 3])
                assert np.array_equal(ch.get_values("laplacian_like"), tr[:, c, hm.nh + 5:hm.nh + 7])
        hm.release()
    assert res["launch"][0] == res["steps"][0]
    assert np.array_equal(res["launch"][1], res["steps"][1])
    for c in range(C):
        a = open(os.path.join(res["launch"][2], "hypers", "stage_1", "chain-%d.bin" % c), "rb").read()
        b = open(os.path.join(res["steps"][2], "hypers", "stage_1", "chain-%d.bin" % c), "rb").read()
        assert a == b
    f.release()
