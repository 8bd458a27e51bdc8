"""The host sampler path (BatchedMetropolis / pt_sample on HostTarget + HostOps) against posteriors known in closed form
(tests/posterior_ref.py): chains started at independent exact draws must end at independent exact draws, so the five
statistics of ``posterior_statistics`` keep their derived bounds (|z| <= 5, chi2 <= 46.1) -- and every named mutation of
a rule, applied by monkeypatch in its test only, must leave them.

The density is model G's (four slips, one hyper-parameter, from the host arrays of ``build_problem``) with two more
parameters that nothing reads, "H": their proposals leave the box often, which is the refuse-and-park path.  Run lengths
and proposal scales: ``posterior_ref.SETTINGS`` (n_steps >= 20 integrated autocorrelation times, measured).  The seeds
below were chosen once and are frozen.  The Poisson family is left out: ``poisson(lam) - lam`` is not symmetric.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posterior_ref as pr  # noqa: E402

R = 4096
SEED = 20251021


@pytest.fixture(scope="module")
def posts():
    G = pr.model_G()[3]
    return {"G": G, "G1": pr.model_G(nobs=pr.G1_NOBS)[3], "S": pr.model_S()[3], "H": G.with_free(2)}


@pytest.fixture(scope="module")
def H(posts):
    from beat_amd.sampler.hosttarget import HostTarget
    return posts["H"], HostTarget(posts["H"].like, posts["H"].nparams)


def _run(H, family, beta, seed=SEED, key="H", **kw):
    post, target = H
    c, rho, n_steps = pr.SETTINGS[key][family]
    Q0 = post.exact_draws(R, beta, np.random.default_rng(seed))
    Q, acc, _ = pr.run_chains(target, post, Q0, family, post.proposal(family, c, rho, beta), beta, n_steps, seed, **kw)
    st = pr.posterior_statistics(Q, post, beta)
    print("%s %s beta %.1f: acceptance %.3f  %s" % (post.name, family, beta, acc, pr.describe(st)))
    return st, acc


# ----------------------------------------------------------------------------- the reference checks itself
def test_models_meet_the_conditions_of_the_closed_form(posts):
    """the h box bites at both ends at every beta in use, the slip box lies >= 10 conditional standard deviations from m
    at the largest e^h / sqrt(beta), the Gamma shape is positive, and model S's grids send the whole box to node 0"""
    betas = sorted(set(pr.GROUP_BETAS) | set(pr.ladder_betas().tolist()))
    for key in ("G", "G1", "S"):
        post = posts[key]
        for b in betas:
            below, above = post.truncation(b)
            assert below > 0.01 and above > 0.01 and below + above < 0.9, (key, b, below, above)
        sd = post.slip_sd(min(betas))
        assert ((post.m - post.lower[post.slip_cols]) >= 10.0 * sd).all() and ((post.upper[post.slip_cols] - post.m) >= 10.0 * sd).all()
    spec, _, host, S = pr.model_S()
    assert spec.D == 1 and spec.S == 1 and S.free_cols.size == 11
    lay = host["layout"]
    du = slice(lay.offsets["durations"], lay.offsets["durations"] + 4)
    assert (np.rint((np.array([S.lower[du], S.upper[du]]) - spec.du_min) / spec.du_dt) == 0).all()
    # start times lie in [0, st_min] (sweep + time <= st_min: build_problem's axis check): index rint((t - st_min) / st_dt)
    assert np.rint((0.0 - spec.st_min) / spec.st_dt) == 0 and spec.st_min >= S.upper[lay.offsets["time"]]


@pytest.mark.parametrize("key", ["G", "G1", "S", "H"])
def test_exact_draws_pass_and_inflated_draws_fail(posts, key):
    post = posts[key]
    for beta in (1.0, 0.4) + tuple(pr.ladder_betas()[1:]) + pr.GROUP_BETAS[1:3]:
        pr.assert_sensitive(post, R, beta)          # fresh draws inside every bound, 10 % more variance outside
        st = pr.posterior_statistics(post.exact_draws(R, beta, np.random.default_rng(3)), post, beta)
        pr.assert_within_bounds(st, "%s beta %g" % (key, beta))
        # the formula is the density the draws come from: beta like + the Jacobian-free box is what the CDFs invert
        assert st["inside"]
    # draws of another temperature fail: the slips through statistic 3, h through statistic 4 or 5
    bad = pr.violations(pr.posterior_statistics(post.exact_draws(R, 1.0, np.random.default_rng(4)), post, 0.4))
    assert "z_r2" in bad and ("z_unif[h]" in bad or "chi2_unif[h]" in bad), bad
    assert pr.chi2_bound() == pytest.approx(46.1, abs=0.05)


def test_statistics_match_their_definitions(posts):
    """statistics 1-5 restated with plain loops on a small sample"""
    from scipy.stats import chi2, gamma
    post, beta = posts["H"], 0.7
    Q = post.exact_draws(200, beta, np.random.default_rng(9))
    st = pr.posterior_statistics(Q, post, beta)
    L = np.linalg.cholesky(post.A)
    w = np.array([np.sqrt(beta) * np.exp(-q[post.h_col]) * (L.T @ (q[post.slip_cols] - post.m)) for q in Q])
    assert st["z_mean"] == pytest.approx(np.sqrt(200) * max(abs(w[:, i].mean()) for i in range(4)), rel=1e-9)
    zc = max(abs((w[:, i] * w[:, j]).mean() - (i == j)) / (np.sqrt(2) if i == j else 1.0) for i in range(4) for j in range(4))
    assert st["z_cov"] == pytest.approx(np.sqrt(200) * zc, rel=1e-9)
    r2 = (w ** 2).sum(1)
    assert st["z_r2"] == pytest.approx((r2.mean() - 4) / np.sqrt(8 / 200.0), rel=1e-9)
    g = gamma(0.5 * (beta * post.M - 4), scale=2.0 / (beta * post.r0))
    lo, hi = g.cdf(np.exp(-2 * post.upper[post.h_col])), g.cdf(np.exp(-2 * post.lower[post.h_col]))
    v = (g.cdf(np.exp(-2 * Q[:, post.h_col])) - lo) / (hi - lo)
    assert 0.0 <= v.min() and v.max() <= 1.0
    assert st["z_unif"]["h"] == pytest.approx(np.sqrt(12 * 200) * (v.mean() - 0.5), rel=1e-9, abs=1e-9)
    counts = [int(((v >= k / 10.0) & (v < (k + 1) / 10.0)).sum()) for k in range(10)]
    assert st["chi2_unif"]["h"] == pytest.approx(sum((c - 20.0) ** 2 / 20.0 for c in counts), rel=1e-9)
    edges = chi2.ppf(np.arange(1, 10) / 10.0, 4)
    counts = np.bincount(np.searchsorted(edges, r2), minlength=10)
    assert st["chi2_r2"] == pytest.approx(((counts - 20.0) ** 2 / 20.0).sum(), rel=1e-9)
    assert set(st["z_unif"]) == {"h", "q5", "q6"}


# ----------------------------------------------------------------------------- the host sampler keeps the posterior
@pytest.mark.parametrize("beta", [1.0, 0.4])
@pytest.mark.parametrize("family", pr.FAMILIES)
def test_host_metropolis_keeps_the_posterior(H, family, beta):
    st, acc = _run(H, family, beta)
    pr.assert_within_bounds(st, "%s beta %g" % (family, beta))
    pr.assert_acceptance(acc, family)


def _run_grouped(H, seed=SEED):
    post, target = H
    Q0, betas = pr.ladder_start(post, pr.GROUP_BETAS, R, np.random.default_rng(seed))
    c, rho, n_steps = pr.SETTINGS["H"]["MultivariateNormal"]
    Q, acc, acc_chain = pr.run_chains(target, post, Q0, "MultivariateNormal", post.proposal_cov(c, rho), betas, n_steps, seed,
                                      groups=pr.group_factors(post, "H"))
    return Q, acc_chain


def test_host_grouped_proposals_per_temperature(H):
    Q, acc_chain = _run_grouped(H)
    pr.check_ladder(Q, H[0], pr.GROUP_BETAS, R, acc_chain, "host grouped")


def test_host_pt_keeps_the_posterior(H):
    post, target = H
    Q, like, swaps = pr.run_pt(target, post, "H", R, SEED)
    st = pr.posterior_statistics(Q, post, 1.0)
    print("host pt_sample: swap acceptance %s  %s" % (np.round(swaps, 3), pr.describe(st)))
    pr.assert_within_bounds(st, "pt_sample")
    assert np.allclose(like, post.like(Q), rtol=1e-12)
    assert all(0.05 < s < 0.95 for s in swaps)       # the exchange is exercised in both directions


# ----------------------------------------------------------------------------- power: every mutation leaves a bound
def _mutated_astep(ignore_beta=False, clamp=False):
    def astep_batch(self, Q0, L0, delta, scaling, lower, upper, log_u, beta, accepted=None):
        import torch
        q = Q0 + delta * scaling[:, None]
        inb = ((q >= lower) & (q <= upper)).all(1)
        if clamp:       # the proposal is moved onto the box instead of being refused
            q = torch.minimum(torch.maximum(q, lower), upper)
            inb = torch.ones_like(inb)
        qe = torch.where(inb[:, None], q, Q0)
        lp = self.batch(qe)
        b = beta if hasattr(beta, "shape") and getattr(beta, "ndim", 0) else float(beta)
        if ignore_beta:
            b = 1.0
        mr = b * (lp[:, -1] - L0[:, -1])
        acc = inb & torch.isfinite(mr) & (log_u < mr)
        Q0[acc] = q[acc]
        L0[acc] = lp[acc]
        if accepted is None:
            accepted = torch.zeros(Q0.shape[0], dtype=torch.int32)
        accepted.copy_(acc.to(torch.int32))
        return accepted
    return astep_batch


def test_the_unmutated_restatement_is_the_host_rule(H, monkeypatch):
    """the rule the mutations start from is HostTarget.astep_batch itself: same states from the same draws"""
    from beat_amd.sampler.hosttarget import HostTarget
    post, target = H
    Q0 = post.exact_draws(256, 0.4, np.random.default_rng(1))
    prop = post.proposal("MultivariateNormal", 1.0, 0.2, 0.4)
    a = pr.run_chains(target, post, Q0, "MultivariateNormal", prop, 0.4, 40, 5)
    monkeypatch.setattr(HostTarget, "astep_batch", _mutated_astep())
    b = pr.run_chains(target, post, Q0, "MultivariateNormal", prop, 0.4, 40, 5)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def test_mutation_beta_ignored_in_accept(H, monkeypatch):
    from beat_amd.sampler.hosttarget import HostTarget
    monkeypatch.setattr(HostTarget, "astep_batch", _mutated_astep(ignore_beta=True))
    st, _ = _run(H, "MultivariateNormal", 0.4)
    assert pr.violations(st), pr.describe(st)


def test_mutation_clamp_instead_of_refuse(H, monkeypatch):
    from beat_amd.sampler.hosttarget import HostTarget
    monkeypatch.setattr(HostTarget, "astep_batch", _mutated_astep(clamp=True))
    st, _ = _run(H, "MultivariateNormal", 1.0)
    assert pr.violations(st), pr.describe(st)


@pytest.mark.parametrize("mutation", ["sign flipped", "always accepted"])
def test_mutation_swap_rule(H, monkeypatch, mutation):
    from beat_amd.sampler import pt
    if mutation == "sign flipped":
        monkeypatch.setattr(pt, "propose_chain_swap", lambda b1, b2, l1, l2, log_u: log_u < (b1 - b2) * (l1 - l2))
    else:
        monkeypatch.setattr(pt, "propose_chain_swap", lambda b1, b2, l1, l2, log_u: np.ones_like(log_u, dtype=bool))
    post, target = H
    Q, _, swaps = pr.run_pt(target, post, "H", R, SEED)
    st = pr.posterior_statistics(Q, post, 1.0)
    print("swap %s: swap acceptance %s  %s" % (mutation, np.round(swaps, 3), pr.describe(st)))
    assert pr.violations(st), pr.describe(st)


def test_mutation_permutation_not_applied_to_the_likelihoods(H, monkeypatch):
    """the swapped states travel, their likelihood vectors stay behind"""
    from beat_amd.sampler import pt
    post, target = H
    exchange = pt.parallel.exchange_rows

    def states_only(X, perm, n_total, gather=None):
        out = exchange(X, perm, n_total, gather=gather)
        out[:, post.nparams:] = X[:, post.nparams:]
        return out
    monkeypatch.setattr(pt.parallel, "exchange_rows", states_only)
    Q, _, swaps = pr.run_pt(target, post, "H", R, SEED)
    st = pr.posterior_statistics(Q, post, 1.0)
    print("likelihoods not permuted: %s" % pr.describe(st))
    assert pr.violations(st), pr.describe(st)


def test_mutation_grouped_factor_of_the_neighbouring_group(H, monkeypatch):
    """group g + 1 steps with the factor of group g.  The proposal stays symmetric, so the density is kept (checked); the
    bound that breaks is the acceptance band of a temperature (posterior_ref.GROUP_C)"""
    from beat_amd.sampler.ops import HostOps
    draw = HostOps.draw

    def shifted(self, factor, n_chains, seed, step, first_chain=0, df=0, groups=None):
        if groups:
            factor = factor.roll(1, 0)
        return draw(self, factor, n_chains, seed, step, first_chain=first_chain, df=df, groups=groups)
    monkeypatch.setattr(HostOps, "draw", shifted)
    Q, acc_chain = _run_grouped(H)
    with pytest.raises(AssertionError, match="acceptance"):
        pr.check_ladder(Q, H[0], pr.GROUP_BETAS, R, acc_chain, "shifted factors")
