"""The polarity composite on the GPU (csrc/polarity.hip): the w -> beta kernel bit for bit numpy.interp; m6, amplitudes and
likelihood columns against 50-digit mpmath values (tests/golden/polarity.npz) within the bounds derived in
tests/polarity_ref.py; the model against the one-chain host composition; batching, graph replay, parked chains, a geodetic
composite beside it; 40 fused steps; two ranks on one GPU; a short SMC run.

Observed on an MI355X (printed by the tests): see DESIGN.md section 7, row a24."""
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

import polarity_ref as pref
from beat_amd import polarity_binding as pb
from conftest import ROOT, load_golden
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

KINDS = ("mtqt", "mt", "dc")
WAVES = ("any_P", "any_SV", "any_SH")
VARS = {"mtqt": ("w", "v", "kappa", "sigma", "h"), "mt": ("mnn", "mee", "mdd", "mne", "mnd", "med"), "dc": ("strike", "dip", "rake")}
C38 = 3.0 * np.pi / 8.0
BOX = {"w": (-C38, C38), "v": (-1.0 / 3.0, 1.0 / 3.0), "kappa": (0.0, 2.0 * np.pi), "sigma": (-np.pi / 2.0, np.pi / 2.0),
       "h": (0.0, 1.0), "strike": (0.0, 360.0), "dip": (0.0, 90.0), "rake": (-180.0, 180.0)}
BOX.update({k: (-1.0, 1.0) for k in VARS["mt"]})


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


def _rw(g):
    return np.concatenate([g["rw_" + w] for w in WAVES], axis=1)


def _all_sampled(kind):
    nv = len(VARS[kind])
    off = -np.ones(6, dtype=np.int64)
    off[:nv] = np.arange(nv)
    return off, np.zeros(6)


# ------------------------------------------------------------------------------------------------- kernels vs references
def test_w_to_beta_is_numpy_interp_bit_for_bit(ctx):
    import torch
    g = load_golden("polarity")
    U, B = g["u_mapping"], g["beta_mapping"]
    w = np.concatenate([g["w_to_beta_w"], C38 - U, C38 - U[::7] * (1 + 2.0 ** -52), [C38 + 1.0, -C38 - 1.0, np.nan],
                        np.linspace(-C38, C38, 4099), np.nextafter(C38 - U[::13], 10.0)])
    want = np.interp(C38 - w, U, B)
    got = pb.w_to_beta_batch(ctx, w)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(got[:g["w_to_beta"].size], g["w_to_beta"])
    dev = pb.w_to_beta_batch(ctx, torch.from_numpy(w).cuda())
    assert np.array_equal(dev.cpu().numpy(), want, equal_nan=True)


@pytest.mark.parametrize("kind", KINDS)
def test_m6_vs_mpmath(ctx, kind):
    g = load_golden("polarity")
    P = np.ascontiguousarray(g["P_" + kind])
    off, fix = _all_sampled(kind)
    m = pb.mt6_batch(ctx, P, kind, off, fix)
    err = np.abs(m - g["mp_m6_" + kind])
    print("%s: m6 on the device %.2f units of 2^-53 from mpmath (reference %.2f; bound K = %g), %.2f from the restatement"
          % (kind, err.max() / pref.U2, float(g["ref_m6_units_" + kind]), pref.K_M6,
             np.abs(m - pref.m6(kind, P)).max() / pref.U2))
    assert m.shape == (P.shape[0], 6) and np.all(err <= pref.bound_m6())
    # rows are independent: one row alone, and a fixed slot in place of a sampled one
    assert np.array_equal(pb.mt6_batch(ctx, P[5:6], kind, off, fix), m[5:6])
    off2, fix2 = off.copy(), fix.copy()
    off2[1], fix2[1] = -1, P[9, 1]
    assert np.array_equal(pb.mt6_batch(ctx, P[9:10], kind, off2, fix2), m[9:10])


def test_zero_tensor_is_nan_like_the_reference(ctx):
    off, fix = _all_sampled("mt")
    m = pb.mt6_batch(ctx, np.zeros((3, 6)), "mt", off, fix)
    assert np.isnan(m).all()


@pytest.mark.parametrize("kind", KINDS)
def test_amplitudes_vs_mpmath(ctx, kind):
    g = load_golden("polarity")
    rw = _rw(g)
    n = g["mp_amp_" + kind].shape[0]
    P = np.ascontiguousarray(g["P_" + kind][:n])
    off, fix = _all_sampled(kind)
    amp = pb.polarity_amplitudes_batch(ctx, P, kind, off, fix, rw)
    bd = pref.bound_amplitudes(rw)[None]
    err = np.abs(amp - g["mp_amp_" + kind])
    ok = bd[0] > 0
    print("%s: amplitudes at most %.4f of their bound from mpmath" % (kind, (err[:, ok] / bd[:, ok]).max()))
    assert amp.shape == (n, rw.shape[1]) and np.all(err <= bd)


def _fixture_problem(kind, g):
    """every source variable sampled, the three maps of the fixture sharing one sampled sigma"""
    from beat_amd.models import ParameterLayout, PolarityMap, PolarityProblem
    n = g["takeoff"].size
    lay = ParameterLayout(OrderedDict([(v, 1) for v in VARS[kind]] + [("h_pol", 1)]))
    maps = [PolarityMap(w, g["takeoff"], g["azimuth"], g["obs"][i * n:(i + 1) * n]) for i, w in enumerate(WAVES)]
    return PolarityProblem(lay, kind, maps, hypers=["h_pol"] * 3, gamma=float(g["gamma"])), lay


@pytest.mark.parametrize("kind", KINDS)
def test_llk_columns_vs_mpmath(ctx, kind):
    g = load_golden("polarity")
    prob, lay = _fixture_problem(kind, g)
    f = prob.compile(ctx)
    rw = _rw(g)
    n = g["mp_llk_" + kind].shape[1]
    worst = 0.0
    for k, sg in enumerate(g["sigmas"]):
        Q = np.concatenate([g["P_" + kind][:n], np.full((n, 1), sg)], axis=1)
        LL = f.batch(Q)
        want = g["mp_llk_" + kind][k]
        bd = pref.bound_llk(rw, g["mp_amp_" + kind][:n], want, float(g["gamma"]), sg)
        err = np.abs(LL[:, :-1] - want)
        worst = max(worst, float((err / bd).max()))
        assert LL.shape == (n, rw.shape[1] + 1) and np.all(err <= bd), (kind, sg, float((err / bd).max()))
        like = np.zeros(n)
        for s in range(rw.shape[1]):
            like = like + LL[:, s]
        assert np.array_equal(LL[:, -1], like)                  # `like` is the serial sum of the composite's columns
    print("%s: llk at most %.4f of its bound from mpmath (E = %g)" % (kind, worst, pref.E_LLK))
    assert f.out_names == ["polarity_like", "like"]
    out = f(Q[0])
    assert len(out) == 2 and np.array_equal(out[0], LL[0, :-1]) and out[1] == LL[0, -1]
    f.release()


# ------------------------------------------------------------------------------------------------- model level
def _model(kind, n_t, seed):
    """two maps (any_P of n_t stations, its sigma sampled; any_SH of n_t stations, its sigma fixed), source variables mixed"""
    from beat_amd.models import ParameterLayout, PolarityMap, PolarityProblem
    rng = np.random.default_rng(seed)
    sampled = {"mtqt": ("w", "kappa", "sigma", "h"), "mt": ("mnn", "mdd", "mne", "mnd", "med"), "dc": ("strike", "rake")}[kind]
    fixed = {"mtqt": {"v": 0.11}, "mt": {"mee": -0.4}, "dc": {"dip": 63.0}}[kind]
    lay = ParameterLayout(OrderedDict([(v, 1) for v in sampled] + [("h_any_P_pol_0", 1)]))
    maps = [PolarityMap(w, rng.uniform(0.0, np.pi, n_t), rng.uniform(0.0, 2.0 * np.pi, n_t), rng.choice([-1, 1], n_t))
            for w in ("any_P", "any_SH")]
    lower = {v: BOX[v][0] for v in sampled}
    upper = {v: BOX[v][1] for v in sampled}
    lower["h_any_P_pol_0"], upper["h_any_P_pol_0"] = 0.02, 2.0
    fixed = dict(fixed, h_any_SH_pol_1=0.3)
    prob = PolarityProblem(lay, kind, maps, fixed=fixed, lower=lower, upper=upper)
    return prob, lay, lower, upper


def _host(prob, Q):
    off, fix = prob.source_tables()
    hoff, hfix = prob.hyper_tables()
    return pref.forward(prob.source_kind, Q, off, fix, prob.radiation_weights(), prob.observations(),
                        [m.n_t for m in prob.maps], prob.gamma, hoff, hfix)


def _draw(lay, lower, upper, C, rng):
    lo, up = lay.bounds(lower, upper)
    return lo + (up - lo) * rng.random((C, lay.size))


@pytest.mark.parametrize("n_t", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", KINDS)
def test_model_vs_one_chain_host_composition(ctx, kind, n_t):
    prob, lay, lower, upper = _model(kind, n_t, 100 + n_t)
    f = prob.compile(ctx)
    assert f.nllk == 2 * n_t + 1 and f._llk_index == 1
    rng = np.random.default_rng(n_t)
    for C in (1, 63, 64, 65, 530):
        Q = _draw(lay, lower, upper, C, rng)
        LL = f.batch(Q)
        assert LL.shape == (C, 2 * n_t + 1)
        np.testing.assert_allclose(LL, _host(prob, Q), rtol=1e-9)
    amp = f.polarity_synthetics(Q)
    m6 = f.moment_tensors(Q)
    off, fix = prob.source_tables()
    ref6 = pref.m6(kind, pref.source_params(kind, Q, off, fix))
    assert np.all(np.abs(m6 - ref6) <= 2 * pref.bound_m6())
    np.testing.assert_allclose(amp, pref.amplitudes(prob.radiation_weights(), ref6), rtol=0, atol=4 * pref.bound_amplitudes(
        prob.radiation_weights()).max())
    f.release()


def test_bitwise_batching_and_device_tensors(ctx):
    """calls of 1 + 64 + 465 chains are one call of 530, host arrays and device tensors alike"""
    import torch
    for kind in KINDS:
        prob, lay, lower, upper = _model(kind, 65, 7)
        f = prob.compile(ctx)
        Q = _draw(lay, lower, upper, 530, np.random.default_rng(3))
        LL = f.batch(Q)
        parts = np.concatenate([f.batch(np.ascontiguousarray(Q[a:b])) for a, b in ((0, 1), (1, 65), (65, 530))])
        assert np.array_equal(parts, LL)
        Qd = torch.from_numpy(Q).cuda()
        assert np.array_equal(f.batch(Qd).cpu().numpy(), LL)
        assert np.array_equal(f.moment_tensors(Qd).cpu().numpy(), f.moment_tensors(Q))
        assert np.array_equal(f.polarity_synthetics(Qd[65:]).cpu().numpy(), f.polarity_synthetics(Q)[65:])
        f.release()


def test_c_abi_rejects_bad_tables(ctx):
    from beat_amd import _lib
    L = _lib.FfiLayout()
    L.nparams, L.nvar = 4, 0
    for i in range(4):
        L.slip_off[i] = -1
    for fld in ("durations_off", "velocities_off", "nuc_strike_off", "nuc_dip_off", "time_off", "h_laplacian_off"):
        setattr(L, fld, -1)
    mid = ctx.ffi_model_create(L, [], [], [])
    rw, obs = np.ones((6, 3)), np.ones(3)
    ok = dict(kind="dc", param_off=[0, 1, 2, -1, -1, -1], param_fixed=np.zeros(6), n_t=[3], rw=rw, obs=obs, gamma=0.2,
              hp_off=[3], hp_fixed=[0.0])
    for bad, msg in ((dict(param_off=[0, 1, 4, -1, -1, -1]), "outside q"), (dict(hp_off=[4]), "outside q"),
                     (dict(gamma=0.7), "gamma"), (dict(n_t=[0], rw=np.ones((6, 0)), obs=np.ones(0)), "no station"),
                     (dict(n_t=[1] * 9, rw=np.ones((6, 9)), obs=np.ones(9), hp_off=[3] * 9, hp_fixed=[0.0] * 9), "polarity maps")):
        with pytest.raises(ValueError, match=msg):
            pb.ffi_model_add_polarity(ctx, mid, **dict(ok, **bad))
    with pytest.raises(ValueError, match="no composite"):
        ctx.ffi_logp_batch(mid, np.zeros((1, 4)), 1)
    pb.ffi_model_add_polarity(ctx, mid, **ok)
    assert ctx.ffi_model_nllk(mid) == 4
    with pytest.raises(ValueError, match="already has a polarity composite"):
        pb.ffi_model_add_polarity(ctx, mid, **ok)
    for call in (lambda: ctx.ffi_llks_batch(mid, np.zeros((2, 4))), lambda: ctx.ffi_variance_reductions_batch(mid, np.zeros((2, 4)), 1),
                 lambda: ctx.ffi_obs_quads(mid, 1)):
        with pytest.raises(ValueError, match="no Gaussian misfit"):
            call()
    ctx.ffi_model_destroy(mid)


# ------------------------------------------------------------------------------------------------- beside a geodetic composite
def _joint(seed):
    """a rectangular dislocation seen by two SAR scenes and by P / SH polarities: strike and dip shared (degrees), the
    location fixed; -> the geodetic problem alone and the joint one, over one layout"""
    from beat_amd.models import GeodeticGeometryProblem, ParameterLayout, PolarityMap, PolarityProblem
    from test_geometry import _problem as _gproblem
    rng = np.random.default_rng(seed)
    sizes = (60, 41)
    base, _, lower0, upper0 = _gproblem(rng, sizes)
    sampled = ("dip", "length", "slip", "strike", "width", "h_SAR", "h_any_P_pol_0")
    lay = ParameterLayout(OrderedDict((v, 1) for v in sampled))
    lower = {v: lower0[v] for v in sampled[:-1]}
    upper = {v: upper0[v] for v in sampled[:-1]}
    lower["h_any_P_pol_0"], upper["h_any_P_pol_0"] = 0.02, 2.0
    fixed = dict(base.fixed, depth=3.0, east_shift=0.5, north_shift=-1.0, h_any_SH_pol_1=0.3)

    def geo():
        return GeodeticGeometryProblem(lay, base.sources, base.east, base.north, base.los, base.data, base.odws, sizes,
                                       base.weights, base.slog_pdets, base.hypers, fixed=fixed, lower=lower, upper=upper)
    maps = [PolarityMap(w, rng.uniform(0.0, np.pi, 65), rng.uniform(0.0, 2.0 * np.pi, 65), rng.choice([-1, 1], 65))
            for w in ("any_P", "any_SH")]
    joint = PolarityProblem(lay, "dc", maps, fixed=fixed, lower=lower, upper=upper, geodetic=geo())
    return geo(), joint, lay, lower, upper


def test_beside_a_geodetic_composite_the_geodetic_columns_keep_their_bits(ctx):
    geo, joint, lay, lower, upper = _joint(11)
    fg, fj = geo.compile(ctx), joint.compile(ctx)
    assert fj.out_names == ["geo_like", "polarity_like", "like"] and fj._llk_index == 2 and fj.nllk == 2 + 130 + 1
    Q = _draw(lay, lower, upper, 530, np.random.default_rng(12))
    Lg, Lj = fg.batch(Q), fj.batch(Q)
    assert np.array_equal(Lj[:, :2], Lg[:, :2])
    np.testing.assert_allclose(Lj[:, 2:-1], _host(joint, Q)[:, :-1], rtol=1e-9)
    sg = (0.0 + Lj[:, 0]) + Lj[:, 1]
    sp = np.zeros(530)
    for s in range(130):
        sp = sp + Lj[:, 2 + s]
    assert np.array_equal(Lj[:, -1], (0.0 + sg) + sp)          # the serial sum over both groups
    out = fj(Q[3])
    assert [np.size(o) for o in out] == [2, 130, 1]
    fg.release()
    fj.release()


# ------------------------------------------------------------------------------------------------- fused step
@pytest.mark.parametrize("kind", ["mtqt", "dc"])
def test_fused_step_against_the_host_decision_sequence(ctx, kind):
    """40 Metropolis steps through the fused step: every step's decisions and likelihood bookkeeping equal the host
    composition chain by chain; a proposal that leaves the prior box is parked and rejected, its rows untouched"""
    prob, lay, lower, upper = _model(kind, 65, 21)
    f = prob.compile(ctx)
    lo, up = lay.bounds(lower, upper)
    rng = np.random.default_rng(17)
    C = 24
    Q = _draw(lay, lower, upper, C, rng)
    L = f.batch(Q)
    beta = 0.7
    n_acc = 0
    for step in range(40):
        delta = rng.standard_normal((C, lay.size)) * (up - lo) * 0.05
        parked = step % C
        delta[parked] = 0.0
        delta[parked, lay.size - 1] = 9.0           # sigma alone leaves [0.02, 2] at every scaling >= 0.5
        scaling = rng.uniform(0.5, 1.5, C)
        log_u = np.log(rng.random(C))
        Q0, L0 = Q.copy(), L.copy()
        acc = f.astep_batch(Q, L, delta, scaling, lo, up, log_u, beta)
        qs = Q0 + delta * scaling[:, None]
        inside = np.all((qs >= lo) & (qs <= up), axis=1)
        lps = _host(prob, qs)
        for c in range(C):
            a_ref = bool(inside[c]) and orc.metrop_accept(beta, lps[c, -1], L0[c, -1], log_u[c])
            assert bool(acc[c]) == a_ref, (step, c)
            if a_ref:
                np.testing.assert_array_equal(Q[c], qs[c])
                np.testing.assert_allclose(L[c], lps[c], rtol=1e-9)
            else:
                assert np.array_equal(Q[c], Q0[c]) and np.array_equal(L[c], L0[c])
            n_acc += a_ref
        assert acc[parked] == 0 and not inside[parked]
    assert 0 < n_acc < 40 * C
    np.testing.assert_allclose(f.batch(Q), L, rtol=1e-12)
    f.release()


def test_fused_step_graph_replay_equals_the_eager_loop(ctx):
    """graph replay bitwise the eager loop, the chain count changing between captures"""
    import torch
    from beat_amd.sampler import SMC
    prob, lay, lower, upper = _model("mtqt", 65, 31)
    f = prob.compile(ctx)
    lo, up = lay.bounds(lower, upper)
    dev = torch.device("cuda", 0)
    for n_chains in (128, 320):
        out = {}
        for use_graph in (False, True):
            step = SMC(f, lo, up, n_chains=n_chains, tune_interval=7, device=dev, random_seed=2, use_graph=use_graph)
            Q = step.initialize_population()
            L = step.stepper.evaluate(Q)
            step.select_end_points(Q, L)
            step.transition()
            step.stage += 1
            Q, L = step.sample_stage(40)
            torch.cuda.synchronize()
            out[use_graph] = (Q.cpu().numpy(), L.cpu().numpy(), list(step.stage_acceptance))
        (Qa, La, acca), (Qb, Lb, accb) = out[False], out[True]
        assert np.array_equal(Qa, Qb) and np.array_equal(La, Lb) and acca == accb
        assert np.isfinite(La[:, -1]).all() and 0.0 < acca[-1] < 1.0
        np.testing.assert_allclose(La[5], _host(prob, Qa[5:6])[0], rtol=1e-9)
    f.release()


# ------------------------------------------------------------------------------------------------- ranks
def _run_ranks(nproc, out):
    from test_gpu_dist import _free_port
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(BEATAMD_TEST_OUT=out, OMP_NUM_THREADS="1")
    worker = os.path.join(ROOT, "tests", "_polarity_gpu_worker.py")
    if nproc == 1:
        cmd = [sys.executable, worker]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("POLARITY_GPU_WORKER_OK") == nproc, r.stdout[-2000:]
    return np.load(out)


def test_two_ranks_on_one_gpu_equal_one_rank(tmp_path):
    one = _run_ranks(1, str(tmp_path / "w1.npz"))
    two = _run_ranks(2, str(tmp_path / "w2.npz"))
    for k in ("betas", "pop", "lp"):
        assert np.array_equal(one[k], two[k]), k
    assert np.isfinite(one["lp"]).all() and one["pop"].shape[0] == 256


# ------------------------------------------------------------------------------------------------- end to end
def e2e_problem():
    """noise-free P polarities of a known double couple at 60 seeded stations, sigma fixed at the example project's 0.05.
    Stations are drawn until 60 have |amplitude| >= 0.15 = 3 sigma at the truth: there every station's p is 0.8 to 1e-3,
    so like(truth) = 60 log 0.8 + O(1e-2), while a point that misses one sign has p <= 0.5 there:
    like <= 59 log 0.8 + log 0.5 -- 0.47 below.  (Also used by tests/_polarity_gpu_worker.py.)"""
    from beat_amd import heart
    from beat_amd.models import ParameterLayout, PolarityMap, PolarityProblem
    rng = np.random.default_rng(2020)
    truth = np.array([[120.0, 55.0, -70.0]])
    m = pref.m6("dc", truth)
    ts, azs = [], []
    while len(ts) < 60:
        t, az = rng.uniform(0.0, np.pi), rng.uniform(0.0, 2.0 * np.pi)
        if abs(pref.amplitudes(heart.radiation_weights_p(np.array([t]), np.array([az])), m)[0, 0]) >= 0.15:
            ts.append(t)
            azs.append(az)
    t, az = np.array(ts), np.array(azs)
    obs = np.sign(pref.amplitudes(heart.radiation_weights_p(t, az), m)[0]).astype(np.int16)
    lay = ParameterLayout(OrderedDict([("strike", 1), ("dip", 1), ("rake", 1)]))
    lower = dict(strike=0.0, dip=0.0, rake=-180.0)
    upper = dict(strike=360.0, dip=90.0, rake=180.0)
    prob = PolarityProblem(lay, "dc", [PolarityMap("any_P", t, az, obs)], fixed={"h_any_P_pol_0": 0.05}, lower=lower, upper=upper)
    return prob, lay, lower, upper, truth, obs


def test_smc_map_point_reproduces_every_observed_polarity(ctx):
    import torch
    from beat_amd.sampler import SMC, smc_sample
    prob, lay, lower, upper, truth, obs = e2e_problem()
    f = prob.compile(ctx)
    lo, up = lay.bounds(lower, upper)
    lt = f.batch(truth)[0, -1]
    assert abs(lt - 60 * np.log(0.8)) < 2e-2
    step = SMC(f, lo, up, n_chains=256, tune_interval=10, device=torch.device("cuda", 0), random_seed=5)
    pop, lp, betas = smc_sample(20, step)
    assert betas[-1] == 1.0 and np.isfinite(lp).all() and np.all((pop >= lo) & (pop <= up))
    like = lp[:, -1] if np.ndim(lp) == 2 else lp
    imap = int(np.argmax(like))
    amp = f.polarity_synthetics(np.ascontiguousarray(pop[imap:imap + 1]))[0]
    print("MAP (strike, dip, rake) = %s, like %.4f (truth %.4f); stations with the observed sign: %d / 60"
          % (np.round(pop[imap], 2).tolist(), like[imap], lt, int((np.sign(amp) == obs).sum())))
    assert np.all(np.sign(amp) == obs)
    f.release()
