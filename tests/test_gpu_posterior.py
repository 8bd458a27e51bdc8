"""The device samplers against posteriors known in closed form (tests/posterior_ref.py): what the parity tests of the single
kernels cannot see -- whether the COMPOSITION of draws, box test, forward model, tempered accept, parking, grouping,
graph replay and exchange samples the density it is meant to sample.

Chains start at independent exact draws of the target; after n_steps steps of a correct sampler the end states are again
independent exact draws, and the five statistics of ``posterior_ref.posterior_statistics`` keep bounds that are derived,
not tuned: |z| <= 5, Pearson chi2 (9 degrees of freedom) <= 46.1.  The Philox streams are counter based: every case is
deterministic.  n_steps >= 20 integrated autocorrelation times of the slowest coordinate, measured on the host path
(``posterior_ref.SETTINGS``); step-size tuning is off; the acceptance rate must lie in [0.15, 0.5]; R = 4096 chains per
group, at which a variance error of 10 % fails statistic 3 (asserted per case on exact draws).  The host path with the same
settings is checked in tests/test_posterior_host.py, where every named mutation of a rule leaves the bounds.  The Poisson
family is left out: ``poisson(lam) - lam`` is not a symmetric proposal.

Two compiled FFI models with P = 4 patches whose ``like`` is the closed form (asserted on exact draws before any sampling,
within 8 M 2^-53 |like|):
  G  geodetic only, dense weights, two datasets sharing one hyper-parameter (G1: a single dataset)
  S  seismic only (nearest neighbour, scalar weights, T = 3, N = 32) with ONE duration and ONE start-time node that the
     whole box maps to: durations, velocities, nucleation point and time run through the rupture sweep and the stacking
     kernel of the fused step and change nothing; their proposals leave the box in a visible share of the steps
     (the parked-chain path)
"""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posterior_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

R = 4096
SEED = 20251021


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def models(ctx):
    """key -> (compiled model, closed form); the closed form IS the model, or the test is wrong"""
    out = {}
    for key, make in (("G", pr.model_G), ("G1", lambda: pr.model_G(nobs=pr.G1_NOBS)), ("S", pr.model_S)):
        spec, prob, host, post = make()
        f = prob.compile(ctx)
        worst = 0.0
        for beta in (1.0, min(pr.GROUP_BETAS)):
            worst = max(worst, pr.assert_formula_is_the_model(f, post, post.exact_draws(512, beta, np.random.default_rng(2))))
        print("model %s: |f.batch - closed form| <= %.3f x (8 M 2^-53 |like|)" % (key, worst))
        out[key] = (f, post)
    return out


def _settings(key, family):
    return pr.SETTINGS["G" if key == "G1" else key][family]


def _kernel(ctx, key):
    """the stacking kernel of the last launch (model S; the geodetic models stack with k_geo_stack alone)"""
    return ctx.last_kernel() if key == "S" else "k_geo_stack (no seismic stacking)"


def _report(ctx, what, acc, st, t0):
    print("%s: acceptance %.3f  %s  kernel %s  (%.2f s)" % (what, acc, pr.describe(st), _kernel(ctx, what.split()[0]), time.time() - t0))


def _fused(ctx, dev, models, key, family, beta, seed=SEED, C=R, **kw):
    f, post = models[key]
    c, rho, n_steps = _settings(key, family)
    Q0 = post.exact_draws(C, beta, np.random.default_rng(seed))
    return pr.run_chains(f, post, Q0, family, post.proposal(family, c, rho, beta), beta, n_steps, seed, device=dev, **kw)


CASES = [(k, fam, 1.0) for k in ("G", "S") for fam in pr.FAMILIES] + [("G1", "MultivariateNormal", 1.0),
                                                                        ("G", "MultivariateNormal", 0.4), ("S", "MultivariateNormal", 0.4)]


@pytest.mark.parametrize("key,family,beta", CASES)
def test_fused_step_eager_and_graph(ctx, dev, models, key, family, beta):
    """mstep_batch in the eager loop and replayed from a HIP graph: the same states to the bit, inside the bounds"""
    post = models[key][1]
    pr.assert_sensitive(post, R, beta)
    t0 = time.time()
    Q, acc, _ = _fused(ctx, dev, models, key, family, beta)
    st = pr.posterior_statistics(Q, post, beta)
    _report(ctx, "%s %s beta %.1f eager" % (key, family, beta), acc, st, t0)
    t0 = time.time()
    Qg, accg, _ = _fused(ctx, dev, models, key, family, beta, use_graph=True)
    _report(ctx, "%s %s beta %.1f graph" % (key, family, beta), accg, pr.posterior_statistics(Qg, post, beta), t0)
    pr.assert_within_bounds(st, "%s %s beta %g" % (key, family, beta))
    pr.assert_acceptance(acc, "%s %s" % (key, family))
    diff = np.flatnonzero((Q != Qg).any(1))
    assert diff.size == 0 and acc == accg, "graph replay differs from the eager loop in %d chains, first %s" % (diff.size, diff[:4])
    pr.assert_within_bounds(pr.posterior_statistics(Qg, post, beta), "%s %s beta %g graph" % (key, family, beta))


@pytest.mark.parametrize("key", ["G", "S"])
def test_per_chain_beta_ladder(ctx, dev, models, key):
    """4 temperatures x R chains in one call, one beta per chain: every temperature against its own beta"""
    f, post = models[key]
    betas = pr.ladder_betas()
    for b in betas:
        pr.assert_sensitive(post, R, b)
    c, rho, n_steps = _settings(key, "MultivariateNormal")
    Q0, chain_betas = pr.ladder_start(post, betas, R, np.random.default_rng(SEED + 1))
    t0 = time.time()
    Q, acc, acc_chain = pr.run_chains(f, post, Q0, "MultivariateNormal", post.proposal_cov(c, rho), chain_betas, n_steps,
                                      SEED + 1, device=dev)
    print("%s ladder: kernel %s (%.2f s)" % (key, _kernel(ctx, key), time.time() - t0))
    pr.check_ladder(Q, post, betas, R, acc_chain, "%s ladder" % key)


@pytest.mark.parametrize("key", ["G", "S"])
def test_grouped_proposals_per_temperature(ctx, dev, models, key):
    """set_group_proposals (mstep_batch_grouped): a factor per temperature.  A factor applied to the wrong run of chains
    keeps the density (the proposal stays symmetric) and leaves the acceptance band of a temperature (GROUP_C)"""
    f, post = models[key]
    for b in pr.GROUP_BETAS:
        pr.assert_sensitive(post, R, b)
    c, rho, n_steps = _settings(key, "MultivariateNormal")
    Q0, chain_betas = pr.ladder_start(post, pr.GROUP_BETAS, R, np.random.default_rng(SEED + 2))
    t0 = time.time()
    Q, acc, acc_chain = pr.run_chains(f, post, Q0, "MultivariateNormal", post.proposal_cov(c, rho), chain_betas, n_steps,
                                      SEED + 2, device=dev, groups=pr.group_factors(post, key))
    print("%s grouped: kernel %s (%.2f s)" % (key, _kernel(ctx, key), time.time() - t0))
    pr.check_ladder(Q, post, pr.GROUP_BETAS, R, acc_chain, "%s grouped" % key)


@pytest.mark.parametrize("key", ["G", "S"])
def test_unfused_route(ctx, dev, models, key):
    """ops.draw + astep_batch: the step in pieces"""
    post = models[key][1]
    pr.assert_sensitive(post, R, 1.0)
    t0 = time.time()
    Q, acc, _ = _fused(ctx, dev, models, key, "MultivariateNormal", 1.0, seed=SEED + 3, fused=False)
    st = pr.posterior_statistics(Q, post, 1.0)
    _report(ctx, "%s unfused" % key, acc, st, t0)
    pr.assert_within_bounds(st, "%s unfused" % key)
    pr.assert_acceptance(acc, "%s unfused" % key)


@pytest.mark.parametrize("plan", ["measured", "ws512"])
def test_model_S_skip_parked_on_and_off(ctx, dev, models, monkeypatch, plan):
    """the fused step with and without the skipping of parked proposals: the same states, inside the bounds -- with the
    group size the launcher measures, and with the 512-chain loader / consumer kernel, which drops whole wavefronts of
    parked chains from its gather"""
    post = models["S"][1]
    pr.assert_sensitive(post, R, 1.0)
    if plan == "ws512":
        monkeypatch.setenv("BEATAMD_GS_CG", "512")
        monkeypatch.setenv("BEATAMD_GS_WS", "1")
    res = {}
    for skip in ("1", "0"):
        monkeypatch.setenv("BEATAMD_SKIP_PARKED", skip)
        t0 = time.time()
        Q, acc, _ = _fused(ctx, dev, models, "S", "Normal", 1.0, seed=SEED + 4)
        st = pr.posterior_statistics(Q, post, 1.0)
        _report(ctx, "S %s BEATAMD_SKIP_PARKED=%s" % (plan, skip), acc, st, t0)
        if plan == "ws512":
            assert ctx.last_kernel().startswith("k_gfstack_ws<")
        pr.assert_within_bounds(st, "S skip_parked %s" % skip)
        pr.assert_acceptance(acc, "S skip_parked %s" % skip)
        res[skip] = (Q, acc)
    assert np.array_equal(res["1"][0], res["0"][0]) and res["1"][1] == res["0"][1]


SMALL_C, SMALL_SEEDS = 70, 59       # 59 x 70 = 4130 >= R chains


def test_model_S_small_batch_pooled_over_seeds(ctx, dev, models):
    """C = 70 chains per call: another stacking plan than at C = 4096 (printed: 128-chain against 256-chain groups of the
    lane <-> chain kernel; the streaming kernel takes over below 48 chains only).  59 seeds are pooled to reach R, each
    run as long as the 20 autocorrelation times ask for: this is the one case of the module that takes several seconds"""
    f, post = models["S"]
    assert SMALL_C * SMALL_SEEDS >= R
    pr.assert_sensitive(post, SMALL_C * SMALL_SEEDS, 1.0)
    t0 = time.time()
    Qs, accs = [], []
    for k in range(SMALL_SEEDS):
        Q, acc, _ = _fused(ctx, dev, models, "S", "Laplace", 1.0, seed=SEED + 100 + k, C=SMALL_C)
        Qs.append(Q)
        accs.append(acc)
    small = (ctx.last_kernel(), ctx.gf_plan(passes=False)["plan"])
    # the same chains replayed from a HIP graph: groups of <= 128 chains size their row buffers from the previous launch's
    # distinct-row count, read back through an event -- a read-back recorded INSIDE the capture invalidated it
    Qg, accg, _ = _fused(ctx, dev, models, "S", "Laplace", 1.0, seed=SEED + 100, C=SMALL_C, use_graph=True)
    assert np.array_equal(Qg, Qs[0]) and accg == accs[0]
    st = pr.posterior_statistics(np.concatenate(Qs), post, 1.0)
    _report(ctx, "S C=%d x %d seeds" % (SMALL_C, SMALL_SEEDS), float(np.mean(accs)), st, t0)
    _fused(ctx, dev, models, "S", "Laplace", 1.0, seed=SEED, C=R)
    print("plan at C = %d: %s | %s\nplan at C = %d: %s | %s" % ((SMALL_C,) + small + (R, ctx.last_kernel(), ctx.gf_plan(passes=False)["plan"])))
    assert small[0] != ctx.last_kernel()
    pr.assert_within_bounds(st, "S C=%d pooled" % SMALL_C)
    pr.assert_acceptance(float(np.mean(accs)), "S C=%d pooled" % SMALL_C)


@pytest.mark.parametrize("key", ["G", "S"])
def test_pt_sample_on_the_device(ctx, dev, models, key):
    """pt_sample(start = exact draws per temperature, every adaptation off): the beta = 1 replicas of the last round"""
    f, post = models[key]
    pr.assert_sensitive(post, R, 1.0)
    t0 = time.time()
    Q, like, swaps = pr.run_pt(f, post, "G" if key == "G1" else key, R, SEED + 5, device=dev)
    st = pr.posterior_statistics(Q, post, 1.0)
    print("%s pt_sample: swap acceptance %s  %s  kernel %s (%.2f s)" % (key, np.round(swaps, 3), pr.describe(st),
                                                                     _kernel(ctx, key), time.time() - t0))
    pr.assert_within_bounds(st, "%s pt_sample" % key)
    ref = post.like(Q)
    assert (np.abs(like - ref) <= 16.0 * post.M * 2.0 ** -53 * np.abs(ref)).all()
    assert all(0.05 < s < 0.95 for s in swaps)


# statistics 1-5 of the final population of run_smc on the HOST path (HostTarget of G's closed form), seeds 101 .. 108:
SMC_HOST = {101: (2.24, 10.7), 102: (2.51, 10.3), 103: (2.53, 15.1), 104: (2.40, 12.7), 105: (1.66, 13.9), 106: (1.90, 11.9),
            107: (2.93, 12.7), 108: (2.07, 6.2)}


def test_smc_sample_end_to_end_on_model_G(ctx, dev, models):
    """smc_sample with 2048 chains and 30 steps per stage from the prior box to beta = 1, end to end.  The final population
    is resampled and moved 30 steps: it is NOT independent, so no bound can be derived.  The bound is MEASURED on the host
    sampler at the same settings over 8 seeds and set to twice the largest value seen (8 seeds under-sample the tail):

        seed   1:mean  2:cov  3:r2   4:unif(h)  5:chi2 v  chi2 r2    largest |z|, chi2
        101    2.24    1.35   +1.31  +0.00      9.8       10.7       2.24  10.7
        102    2.00    2.51   +0.01  +0.30      5.6       10.3       2.51  10.3
        103    2.53    1.68   +0.20  +0.79      15.1      9.6        2.53  15.1
        104    1.16    2.15   +1.48  +2.40      12.7      6.8        2.40  12.7
        105    0.91    1.66   +0.64  -0.10      13.9      6.9        1.66  13.9
        106    1.90    1.51   -1.32  -1.00      6.6       11.9       1.90  11.9
        107    1.31    2.44   +2.93  +1.19      5.6       12.7       2.93  12.7
        108    2.07    1.89   +0.97  -0.01      5.6       6.2        2.07  6.2

    |z| <= 2 x 2.93 = 5.86 and chi2 <= 2 x 15.1 = 30.2 (tail 4e-4 at 9 degrees of freedom: 3.5 SE), both below the 10
    SE-equivalents beyond which the check would be left out."""
    f, post = models["G"]
    z_bound = 2.0 * max(v[0] for v in SMC_HOST.values())
    x_bound = 2.0 * max(v[1] for v in SMC_HOST.values())
    assert z_bound <= 10.0 and x_bound <= pr.chi2_bound()
    t0 = time.time()
    pop, betas = pr.run_smc(f, post, 101, device=dev)
    st = pr.posterior_statistics(pop, post, 1.0)
    z, x = pr.worst(st)
    print("G smc_sample: %d stages  %s (%.2f s)" % (len(betas), pr.describe(st), time.time() - t0))
    assert st["inside"] and z <= z_bound and x <= x_bound, pr.describe(st)
