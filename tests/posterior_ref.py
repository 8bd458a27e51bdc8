"""Closed-form posteriors for the sampler tests (tests/test_posterior_host.py, tests/test_gpu_posterior.py).

A distributed-slip model whose synthetics are linear in the n slips and whose datasets share ONE hyper-parameter h has

    like(s, h) = -1/2 [ slog + M (2 h + log 2 pi) + e^{-2h} ( r0 + (s - m)^T A (s - m) ) ]

(M data, slog the summed log determinants, A = B^T B with B the whitened design matrix, m the least-squares slip, r0 the
residual at m).  With a uniform prior box that cuts nothing off the slips, the density exp(beta like) on the box is

    u = e^{-2h}   ~  Gamma(shape (beta M - n) / 2, rate beta r0 / 2)  truncated to [e^{-2 h_hi}, e^{-2 h_lo}]
    s | h         ~  N(m, e^{2h} A^{-1} / beta)
    every parameter the likelihood does not read: independent, uniform on its box

(integrate the Gaussian in s: a factor (e^{2h} / beta)^{n/2}; then substitute u, dh = -du / (2u)).  Exact draws need
``scipy.stats.gamma.ppf``, standard normals and the Cholesky factor of A only.

Stationarity is then testable with DERIVED bounds: chains started at independent exact draws are, after any number of
steps of a correct sampler, again independent exact draws, so every statistic of ``posterior_statistics`` has a known law:

    w_c = sqrt(beta) e^{-h_c} L^T (s_c - m),  A = L L^T     ~ N(0, I_n)
    v_c = truncated-Gamma CDF of u_c (h), (x - lo) / (up - lo) (unused parameters)   ~ U(0, 1)

    1. sqrt(R) max_i |mean w_i|                                        each ~ N(0, 1)
    2. sqrt(R) max_ij |mean(w_i w_j) - delta_ij| / (sqrt 2 if i == j else 1)   each ~ N(0, 1) (var(w_i^2) = 2)
    3. (mean |w|^2 - n) / sqrt(2 n / R)                                ~ N(0, 1) (|w|^2 ~ chi2_n, variance 2 n)
    4. sqrt(12 R) (mean v - 1/2)  per uniform coordinate               ~ N(0, 1) (var U = 1/12)
    5. Pearson chi2 of v in 10 equal bins, and of |w|^2 in 10 bins at the chi2_n deciles: 9 degrees of freedom

Bounds: |z| <= 5 (two-sided tail 5.733e-7) and chi2 <= chi2.isf(5.733e-7, 9) = 46.1, the same tail probability.  They are
derived, not tuned.  The Poisson proposal family is left out of every posterior test: ``poisson(lam) - lam`` is not a
symmetric proposal, so Metropolis without the Hastings ratio does not keep these densities.
"""
import numpy as np

Z_BOUND = 5.0
TAIL = 5.733e-7          # two-sided normal tail beyond 5 SE
NBINS = 10
LOG_2PI = float(np.log(2.0 * np.pi))
FAMILIES = ("MultivariateNormal", "MultivariateCauchy", "Normal", "Cauchy", "Laplace")


def chi2_bound():
    from scipy.stats import chi2
    return float(chi2.isf(TAIL, NBINS - 1))


class QuadraticPosterior(object):
    """The density above on a box.  slip_cols (n,) / h_col: where s and h sit in a parameter row; every other column is
    read by nothing.  lower / upper: the box the SAMPLER is given (the test's own)."""

    def __init__(self, A, m, r0, M, slog, slip_cols, h_col, lower, upper, name=""):
        self.A, self.m = np.asarray(A, dtype=np.float64), np.asarray(m, dtype=np.float64)
        self.r0, self.M, self.slog = float(r0), int(M), float(slog)
        self.n = self.m.size
        self.slip_cols, self.h_col = np.asarray(slip_cols, dtype=np.int64), int(h_col)
        self.lower, self.upper = np.asarray(lower, dtype=np.float64).copy(), np.asarray(upper, dtype=np.float64).copy()
        self.nparams = self.lower.size
        used = set(self.slip_cols.tolist()) | {self.h_col}
        self.free_cols = np.array([c for c in range(self.nparams) if c not in used], dtype=np.int64)
        self.L = np.linalg.cholesky(self.A)
        self.Ainv = np.linalg.inv(self.A)
        self.name = name

    # -- the density
    def like(self, Q):
        Q = np.asarray(Q, dtype=np.float64)
        d = Q[:, self.slip_cols] - self.m
        h = Q[:, self.h_col]
        quad = self.r0 + ((d @ self.A) * d).sum(1)
        return -0.5 * (self.slog + self.M * (2.0 * h + LOG_2PI) + np.exp(-2.0 * h) * quad)

    def _gamma(self, beta):
        from scipy.stats import gamma
        shape = 0.5 * (beta * self.M - self.n)
        if not shape > 0.0:
            raise ValueError("beta M <= n: the marginal of h is not a Gamma law")
        g = gamma(shape, scale=2.0 / (beta * self.r0))
        u_lo, u_hi = np.exp(-2.0 * self.upper[self.h_col]), np.exp(-2.0 * self.lower[self.h_col])
        return g, float(g.cdf(u_lo)), float(g.cdf(u_hi))

    def truncation(self, beta):
        """-> (mass cut off below h_lo, mass cut off above h_hi) of the untruncated law of h"""
        g, F_lo, F_hi = self._gamma(beta)
        return 1.0 - F_hi, F_lo

    def h_cdf(self, h, beta):
        g, F_lo, F_hi = self._gamma(beta)
        return (g.cdf(np.exp(-2.0 * np.asarray(h))) - F_lo) / (F_hi - F_lo)

    def exact_draws(self, R, beta, rng, inflate=1.0):
        """R independent draws of exp(beta like) on the box; inflate: variance factor of s | h (sensitivity checks)"""
        g, F_lo, F_hi = self._gamma(beta)
        u = g.ppf(F_lo + rng.random(R) * (F_hi - F_lo))
        h = -0.5 * np.log(u)
        z = rng.standard_normal((R, self.n)) * np.sqrt(inflate)
        Q = self.lower + (self.upper - self.lower) * rng.random((R, self.nparams))
        Q[:, self.h_col] = h
        # w = sqrt(beta) e^{-h} L^T (s - m) = z
        Q[:, self.slip_cols] = self.m + (np.exp(h) / np.sqrt(beta))[:, None] * np.linalg.solve(self.L.T, z.T).T
        return Q

    def slip_sd(self, beta, h=None):
        """conditional standard deviations of s | h (h None: the top of the box)"""
        h = self.upper[self.h_col] if h is None else h
        return np.exp(h) / np.sqrt(beta) * np.sqrt(np.diag(self.Ainv))

    # -- proposals scaled to the posterior
    def h_moments(self, beta=1.0):
        g, F_lo, F_hi = self._gamma(beta)
        h = -0.5 * np.log(g.ppf(F_lo + (np.arange(2000) + 0.5) / 2000.0 * (F_hi - F_lo)))
        return float(h.mean()), float(h.std())

    def proposal_cov(self, c, rho, beta=1.0):
        """c^2 / beta x the beta = 1 posterior covariance of (s, h) (h at its mean), (rho x box width)^2 for the rest"""
        hm, hs = self.h_moments()
        cov = np.zeros((self.nparams, self.nparams))
        cov[np.ix_(self.slip_cols, self.slip_cols)] = c * c / beta * np.exp(2.0 * hm) * self.Ainv
        cov[self.h_col, self.h_col] = (c * hs) ** 2 / beta
        w = (self.upper - self.lower)[self.free_cols]
        cov[self.free_cols, self.free_cols] = (rho * w) ** 2
        return cov

    def proposal_scales(self, c, rho, beta=1.0):
        """per-parameter scales: c / sqrt(beta) x the conditional standard deviations of the slips (1 / sqrt(A_ii)) and
        of h, rho x the box width for the rest"""
        hm, hs = self.h_moments()
        sc = np.zeros(self.nparams)
        sc[self.slip_cols] = c / np.sqrt(beta) * np.exp(hm) / np.sqrt(np.diag(self.A))
        sc[self.h_col] = c / np.sqrt(beta) * hs
        sc[self.free_cols] = rho * (self.upper - self.lower)[self.free_cols]
        return sc

    def proposal(self, family, c, rho, beta=1.0):
        """what ``set_proposal`` takes for `family`, scaled to the posterior at `beta`"""
        return self.proposal_cov(c, rho, beta) if family.startswith("Multivariate") else self.proposal_scales(c, rho, beta)

    def with_free(self, k):
        """the same density with k more parameters that nothing reads, on the box [0, 1]"""
        return QuadraticPosterior(self.A, self.m, self.r0, self.M, self.slog, self.slip_cols, self.h_col,
                                  np.concatenate([self.lower, np.zeros(k)]), np.concatenate([self.upper, np.ones(k)]),
                                  name="%s+%d" % (self.name, k))


def posterior_statistics(Q, post, beta):
    """the five statistics of the module docstring for R rows Q that should be independent draws of `post` at `beta`
    -> dict(z_mean, z_cov, z_r2, z_unif {name: z}, chi2_unif {name: chi2}, chi2_r2, R)"""
    from scipy.stats import chi2
    Q = np.asarray(Q, dtype=np.float64)
    R, n = Q.shape[0], post.n
    h = Q[:, post.h_col]
    w = (np.sqrt(beta) * np.exp(-h))[:, None] * ((Q[:, post.slip_cols] - post.m) @ post.L)
    z_mean = float(np.sqrt(R) * np.abs(w.mean(0)).max())
    dev = (w.T @ w) / R - np.eye(n)
    z_cov = float(np.sqrt(R) * (np.abs(dev) / (1.0 + (np.sqrt(2.0) - 1.0) * np.eye(n))).max())
    r2 = (w * w).sum(1)
    z_r2 = float((r2.mean() - n) / np.sqrt(2.0 * n / R))

    def pearson(v):
        counts = np.bincount(np.clip((v * NBINS).astype(np.int64), 0, NBINS - 1), minlength=NBINS)
        e = R / float(NBINS)
        return float(((counts - e) ** 2 / e).sum())

    vs = {"h": post.h_cdf(h, beta)}
    for c in post.free_cols:
        vs["q%d" % c] = (Q[:, c] - post.lower[c]) / (post.upper[c] - post.lower[c])
    z_unif = {k: float(np.sqrt(12.0 * R) * (v.mean() - 0.5)) for k, v in vs.items()}
    chi2_unif = {k: pearson(v) for k, v in vs.items()}
    return dict(z_mean=z_mean, z_cov=z_cov, z_r2=z_r2, z_unif=z_unif, chi2_unif=chi2_unif,
                chi2_r2=pearson(chi2.cdf(r2, n)), R=R,
                inside=bool(((Q >= post.lower) & (Q <= post.upper)).all()))


def worst(st):
    """-> (largest |z| of statistics 1-4, largest chi2 of statistic 5)"""
    z = max([abs(st["z_mean"]), abs(st["z_cov"]), abs(st["z_r2"])] + [abs(v) for v in st["z_unif"].values()])
    return z, max([st["chi2_r2"]] + list(st["chi2_unif"].values()))


def describe(st):
    z, x = worst(st)
    ku = max(st["z_unif"], key=lambda k: abs(st["z_unif"][k]))
    kx = max(st["chi2_unif"], key=lambda k: st["chi2_unif"][k])
    return ("R=%d  1:mean %.2f  2:cov %.2f  3:r2 %+.2f  4:unif %+.2f (%s)  5:chi2 v %.1f (%s) r2 %.1f  | worst z %.2f chi2 %.1f"
            % (st["R"], st["z_mean"], st["z_cov"], st["z_r2"], st["z_unif"][ku], ku, st["chi2_unif"][kx], kx, st["chi2_r2"],
               z, x))


def violations(st):
    """names of the statistics outside their bound"""
    xb = chi2_bound()
    bad = [k for k in ("z_mean", "z_cov", "z_r2") if not abs(st[k]) <= Z_BOUND]
    bad += ["z_unif[%s]" % k for k, v in st["z_unif"].items() if not abs(v) <= Z_BOUND]
    bad += ["chi2_unif[%s]" % k for k, v in st["chi2_unif"].items() if not v <= xb]
    if not st["chi2_r2"] <= xb:
        bad.append("chi2_r2")
    if not st["inside"]:
        bad.append("outside the box")
    return bad


def assert_within_bounds(st, what=""):
    bad = violations(st)
    assert not bad, "%s: %s outside the derived bounds -- %s" % (what, bad, describe(st))


def assert_sensitive(post, R, beta, seed=7):
    """the sensitivity condition of a case: on R exact draws whose s | h variance is 10 % too large, statistic 3 leaves its
    bound (expected z = 0.1 sqrt(n R / 2)); the same draws without the inflation stay inside every bound"""
    st = posterior_statistics(post.exact_draws(R, beta, np.random.default_rng(seed), inflate=1.1), post, beta)
    assert st["z_r2"] > Z_BOUND, "R = %d cannot see a 10 %% variance error: z = %.2f" % (R, st["z_r2"])
    assert_within_bounds(posterior_statistics(post.exact_draws(R, beta, np.random.default_rng(seed)), post, beta), "exact draws")


# ----------------------------------------------------------------------------- the two compiled models
H_QUANTILES = (0.10, 0.88)      # the h box: between these quantiles of u = e^{-2h} at beta = 1 -- it bites at both ends
BOX_SD = 12.0                   # slip box: m +- BOX_SD conditional standard deviations at the top of the h box
BETA_MIN = 0.4                  # ... and the smallest beta any test uses


def _finish(host, B, d, M, slog, name, free_box):
    """QuadraticPosterior of whitened design matrix B (M, n) and data d (M,); free_box {parameter name: (lo, up)}"""
    from scipy.stats import gamma
    lay = host["layout"]
    A = B.T @ B
    m = np.linalg.lstsq(B, d, rcond=None)[0]
    res = d - B @ m
    r0 = float(res @ res)
    n = m.size
    g = gamma(0.5 * (M - n), scale=2.0 / r0)
    hname = [k for k in lay.varsizes if k.startswith("h_")][0]
    # u falls with h: the upper u quantile is the lower end of the h box (rounded: the box is the test's, not the model's)
    h_lo = np.round(-0.5 * np.log(g.ppf(H_QUANTILES[1])), 3)
    h_hi = np.round(-0.5 * np.log(g.ppf(H_QUANTILES[0])), 3)
    lower, upper = np.zeros(lay.size), np.zeros(lay.size)
    slip_cols = np.arange(lay.offsets["uparr"], lay.offsets["uparr"] + n)
    h_col = lay.offsets[hname]
    lower[h_col], upper[h_col] = h_lo, h_hi
    sd = np.exp(h_hi) / np.sqrt(BETA_MIN) * np.sqrt(np.diag(np.linalg.inv(A)))
    lower[slip_cols], upper[slip_cols] = m - BOX_SD * sd, m + BOX_SD * sd
    for k, (lo, up) in free_box.items():
        sl = slice(lay.offsets[k], lay.offsets[k] + lay.varsizes[k])
        lower[sl], upper[sl] = lo, up
    return QuadraticPosterior(A, m, r0, M, slog, slip_cols, h_col, lower, upper, name=name)


G1_NOBS = (16,)          # the single-dataset case


def model_G(nobs=(9, 11), seed=20251021):
    """geodetic only, P = 4 patches, dense weights, the datasets share h_SAR -> (spec, problem, host, posterior)"""
    from beat_amd.synthetic import SyntheticSpec, build_problem
    spec = SyntheticSpec((2,), (2,), (1.0,), T=0, N=0, geodetic_nobs=tuple(nobs), hp_specific=False, seed=seed)
    prob, host = build_problem(spec)
    G = host["gGs"][0]                                   # (P, nobs)
    rows, data, o = [], [], 0
    for k, W in zip(nobs, host["gW"]):
        odw = host["godw"][o:o + k]
        rows.append(W @ (odw[:, None] * G[:, o:o + k].T))
        data.append(W @ (odw * host["gdata"][o:o + k]))
        o += k
    post = _finish(host, np.vstack(rows), np.concatenate(data), int(sum(nobs)), float(np.sum(host["gslog"])),
                   "G%s" % (tuple(nobs),), {})
    return spec, prob, host, post


S_DU = (1.0, 1.0)        # duration node 0 and the sampling: the box 1 +- 0.3 rounds to node 0
S_ST_DT = 100.0          # start-time sampling: (t - st_min) / S_ST_DT in (-0.03, 0] rounds to node 0
S_VEL = (2.5, 4.0)
S_TIME = (0.0, 1.0)


def model_S(seed=20251022):
    """seismic only: nearest neighbour, scalar weights, T = 3, N = 32, P = 4, ONE duration node and ONE start-time node that
    every point of the box maps to: the synthetics are linear in the slips; durations, velocities, nucleation point and
    time pass through the rupture sweep and the stacking kernel and change nothing -> (spec, problem, host, posterior)"""
    from beat_amd.synthetic import SyntheticSpec, build_problem, max_sweep_time
    kw = dict(T=3, N=32, D=1, S=1, st_dt=S_ST_DT, du_min=S_DU[0], du_dt=S_DU[1], hp_specific=False, seed=seed,
              vel_bounds=S_VEL, time_bounds=S_TIME)
    st_min = np.ceil(10.0 * (max_sweep_time(SyntheticSpec((2,), (2,), (1.0,), **kw)) + S_TIME[1])) / 10.0
    spec = SyntheticSpec((2,), (2,), (1.0,), st_min=float(st_min), **kw)
    prob, host = build_problem(spec)                     # (checks that the start-time axis covers the rupture)
    assert 0.0 <= st_min < 0.03 * S_ST_DT
    G = host["Gs"][0][:, :, 0, 0, :]                     # (T, P, N)
    w = host["weights"]
    B = np.vstack([w[t] * G[t].T for t in range(spec.T)])
    d = np.concatenate([w[t] * host["data"][t] for t in range(spec.T)])
    lay = host["layout"]
    free = dict(durations=(S_DU[0] - 0.3 * S_DU[1], S_DU[0] + 0.3 * S_DU[1]), velocities=S_VEL,
                nucleation_strike=(host["lower"]["nucleation_strike"], host["upper"]["nucleation_strike"]),
                nucleation_dip=(host["lower"]["nucleation_dip"], host["upper"]["nucleation_dip"]), time=S_TIME)
    post = _finish(host, B, d, spec.T * spec.N, float(np.sum(host["slog"])), "S", free)
    assert set(lay.varsizes) == set(free) | {"uparr", "h_any_P_0_Z"}
    return spec, prob, host, post


def assert_formula_is_the_model(f, post, Q, c=8.0):
    """f.batch(Q)[:, -1] equals the closed form within c M 2^-53 |like|: if not, the TEST is wrong, not the sampler"""
    got = np.asarray(f.batch(np.ascontiguousarray(Q)))[:, -1]
    ref = post.like(Q)
    err = np.abs(got - ref)
    bound = c * post.M * 2.0 ** -53 * np.abs(ref)
    assert (err <= bound).all(), "model %s is not the closed form: worst error / bound %.3g" % (post.name, (err / bound).max())
    return float((err / bound).max())


# ----------------------------------------------------------------------------- proposal scales and run lengths
# (c, rho, n_steps) per density and family: the proposal is c / sqrt(beta) x the posterior scale of (s, h) and rho x the box
# width of the parameters nothing reads (``QuadraticPosterior.proposal``); n_steps >= 20 x the largest integrated
# autocorrelation time tau of any coordinate at beta = 1 and 0.4, MEASURED on the host path with ``autocorrelation_time``
# (1024 .. 2048 chains started at exact draws; tau and the acceptance rates at beta = 1 / 0.4 beside each entry).  Step-size
# tuning is off everywhere.  "H" is density G with two more parameters that nothing reads (the host tests).
SETTINGS = {
    "G": {"MultivariateNormal": (1.0, 0.0, 500),      # tau 21 / 23, acceptance 0.30 / 0.26
          "MultivariateCauchy": (0.6, 0.0, 900),      # tau 35 / 45, 0.34 / 0.31
          "Normal": (0.8, 0.0, 950),                  # tau 36 / 47, 0.40 / 0.35
          "Cauchy": (0.35, 0.0, 1250),                # tau 54 / 61, 0.32 / 0.30
          "Laplace": (0.6, 0.0, 900)},                # tau 36 / 45, 0.41 / 0.38
    "H": {"MultivariateNormal": (1.0, 0.2, 1150),     # tau 49 / 56, 0.21 / 0.18
          "MultivariateCauchy": (0.6, 0.12, 2050),    # tau 96 / 101, 0.28 / 0.26
          "Normal": (0.8, 0.2, 1200),                 # tau 49 / 59, 0.28 / 0.25
          "Cauchy": (0.35, 0.05, 1800),               # tau 89 / 87, 0.25 / 0.23
          "Laplace": (0.6, 0.14, 1200)},              # tau 48 / 58, 0.31 / 0.28
    # eleven parameters that nothing reads share the budget of proposals that may leave the box: tau is long
    "S": {"MultivariateNormal": (0.5, 0.13, 3400),    # tau 149 / 167, 0.18 / 0.16
          "MultivariateCauchy": (0.45, 0.08, 7400),   # tau 336 / 370, 0.20 / 0.19 (c 0.5, rho 0.11: acceptance 0.15 / 0.14)
          "Normal": (0.45, 0.13, 3600),               # tau 149 / 175, 0.19 / 0.18
          "Cauchy": (0.16, 0.03, 4300),               # tau 189 / 210, 0.20 / 0.19
          "Laplace": (0.35, 0.09, 3100)},             # tau 129 / 151, 0.22 / 0.21
}
ACCEPTANCE = (0.15, 0.5)


def assert_acceptance(rate, what=""):
    assert ACCEPTANCE[0] <= rate <= ACCEPTANCE[1], "%s: acceptance %.3f outside %s" % (what, rate, ACCEPTANCE)


# ----------------------------------------------------------------------------- running chains
def run_chains(target, post, Q0, family, proposal, beta, n_steps, seed, device=None, use_graph=False, groups=None,
               fused=True):
    """n_steps of BatchedMetropolis (step-size tuning off) from the rows Q0 -> (Q (C, nparams) host array, acceptance
    rate, acceptance rate per chain).  proposal: covariance / scales of `family`; groups: (G, K, nparams) factors for set_group_proposals;
    beta: scalar or (C,) array; fused False: ops.draw + astep_batch instead of the one-call step"""
    import torch
    from beat_amd.sampler.metropolis import BatchedMetropolis
    dev = device if device is not None else torch.device("cpu")
    C = Q0.shape[0]
    st = BatchedMetropolis(target, post.lower, post.upper, C, device=dev, tune=False, tune_interval=10 ** 9, seed=seed)
    st.set_proposal(proposal, family)
    if groups is not None:
        st.set_group_proposals(torch.from_numpy(np.ascontiguousarray(groups)).to(dev))
    Q = torch.from_numpy(np.array(Q0, dtype=np.float64, order="C", copy=True)).to(dev)     # (Q0 stays as it is)
    L = st.evaluate(Q).to(dev)
    b = torch.from_numpy(np.ascontiguousarray(beta, dtype=np.float64)).to(dev) if np.ndim(beta) else float(beta)
    n_acc = torch.zeros((), dtype=torch.int64, device=dev)
    if not fused:
        _run_unfused(st, Q, L, b, n_steps, n_acc)
    else:
        st.run(Q, L, b, n_steps, n_acc, use_graph=use_graph)
    st.ops.check()
    # the likelihood the chains carry is the likelihood of their state (within twice the formula check's bound)
    Qh = Q.cpu().numpy()
    carried, now = L[:, -1].cpu().numpy(), post.like(Qh)
    assert (np.abs(carried - now) <= 16.0 * post.M * 2.0 ** -53 * np.abs(now)).all(), "a chain carries a likelihood that is not its state's"
    return Qh, float(n_acc.item()) / (float(n_steps) * C), st.accepted_since_tune.cpu().numpy() / float(n_steps)


def _run_unfused(st, Q, L, beta, n_steps, n_acc):
    """the step in pieces (what BatchedMetropolis does for a target without mstep_batch)"""
    for _ in range(n_steps):
        if st.group_factors is not None:
            delta, log_u = st.ops.draw(st.group_factors, st.n_chains, st.seed, st.n_steps_total, df=st.df,
                                       groups=int(st.group_factors.shape[0]))
        elif st.kind is not None:
            delta, log_u = st.ops.draw_univariate(st.kind, st.uscale, st.n_chains, st.seed, st.n_steps_total)
        else:
            delta, log_u = st.ops.draw(st.factor, st.n_chains, st.seed, st.n_steps_total, df=st.df)
        st.target.astep_batch(Q, L, delta, st.scaling, st.lower, st.upper, log_u, beta, st._acc)
        n_acc += st._acc.sum()
        st.accepted_since_tune += st._acc
        st.n_steps_total += 1


# ----------------------------------------------------------------------------- several temperatures in one call
def ladder_betas(n_tempered=3):
    """the ladder pt_sample starts with: 1, then 1.2^-k (beta tuning off: it stays)"""
    from beat_amd.sampler.pt import TemperingManager
    return TemperingManager(1, n_tempered).betas.copy()


GROUP_BETAS = (1.0, 0.7, 0.5, 0.4)
# grouped proposals: group g steps with c_g / sqrt(beta_g) x the posterior scale, the c alternating between a small and a
# large value that both keep the acceptance inside its band.  Every symmetric proposal keeps the density, so a factor
# applied to the wrong run of chains shows in NO distributional statistic -- it shows in the acceptance rate per group:
# group 0 (beta 1, small c) stepping with the last group's factor (beta 0.4, large c) proposes 1.6 x large c
GROUP_C = {"G": (0.75, 1.25, 0.75, 1.25), "H": (0.45, 1.1, 0.45, 1.1), "S": (0.35, 0.5, 0.35, 0.5)}


def group_factors(post, key, betas=GROUP_BETAS, family="MultivariateNormal"):
    from beat_amd.sampler.base import covariance_factor
    rho = SETTINGS[key][family][1]
    return np.stack([covariance_factor(post.proposal_cov(c, rho, b)) for c, b in zip(GROUP_C[key], betas)])


def ladder_start(post, betas, R, rng):
    """-> (start points (len(betas) R, nparams): R exact draws per temperature, its own beta for every chain)"""
    return np.concatenate([post.exact_draws(R, b, rng) for b in betas]), np.repeat(np.asarray(betas, dtype=np.float64), R)


def check_ladder(Q, post, betas, R, acc_chain=None, what="", report=print):
    """the statistics of every temperature's R chains against its own beta (and its acceptance rate, where given)"""
    out = []
    for g, b in enumerate(betas):
        st = posterior_statistics(Q[g * R:(g + 1) * R], post, b)
        acc = float(acc_chain[g * R:(g + 1) * R].mean()) if acc_chain is not None else None
        report("%s beta %.4f%s: %s" % (what, b, "" if acc is None else " acceptance %.3f" % acc, describe(st)))
        out.append((st, acc))
    for g, (st, acc) in enumerate(out):
        assert_within_bounds(st, "%s temperature %d" % (what, g))
        if acc is not None:
            assert_acceptance(acc, "%s temperature %d" % (what, g))
    return out


PT_STEPS_PER_ROUND = 5      # far fewer than tau: what an exchange does wrong is still there when the next one comes


def run_pt(target, post, key, R, seed, device=None, steps_per_round=PT_STEPS_PER_ROUND, n_tempered=3):
    """pt_sample from exact draws of every temperature, every adaptation off -> the beta = 1 replicas after the last
    recorded round (R rows: the first and the last round are recorded), their likelihoods and the swap acceptance per
    pair.  The run is as long as SETTINGS asks for the family (whole rounds)"""
    from beat_amd.sampler.pt import pt_sample
    c, rho, n_steps = SETTINGS[key]["MultivariateNormal"]
    rounds = -(-n_steps // steps_per_round)
    betas = ladder_betas(n_tempered)
    start, _ = ladder_start(post, betas, R, np.random.default_rng(seed))
    s, ls, man = pt_sample(target, post.lower, post.upper, n_chains_posterior=1, n_chains_tempered=n_tempered, n_replicas=R,
                           n_samples=2 * R, swap_interval=(steps_per_round, steps_per_round), beta_tune_interval=10 ** 9,
                           proposal_cov=post.proposal_cov(c, rho), device=device, random_seed=seed, tune_interval=10 ** 9,
                           record_every=rounds - 1, update_proposal=False, start=start)
    assert s.shape == (2 * R, post.nparams) and np.array_equal(man.betas, betas) and man.loop_steps == rounds * steps_per_round
    swaps = [man.get_acceptance_swap(k) for k in range(n_tempered)]
    return s[-R:], ls[-R:, -1], swaps


SMC_CHAINS, SMC_STEPS = 2048, 30


def run_smc(target, post, seed, device=None):
    """one smc_sample run from the prior box to beta = 1 with the sampler's defaults -> (final population, betas)"""
    from beat_amd.sampler.smc import SMC, smc_sample
    step = SMC(target, post.lower, post.upper, n_chains=SMC_CHAINS, device=device, random_seed=seed)
    pop, lp, betas = smc_sample(SMC_STEPS, step)
    assert betas[-1] == 1.0 and pop.shape == (SMC_CHAINS, post.nparams)
    return pop, betas


def autocorrelation_time(trace):
    """integrated autocorrelation time 1 + 2 sum rho_k per coordinate from a stationary ensemble trace (steps, chains,
    coordinates): rho_k = the across-chain correlation of x_0 and x_k, summed until it first falls below 0.02"""
    x0 = trace[0] - trace[0].mean(0)
    s0 = x0.std(0)
    tau = np.ones(trace.shape[2])
    live = np.ones(trace.shape[2], bool)
    for k in range(1, trace.shape[0]):
        xk = trace[k] - trace[k].mean(0)
        rho = (x0 * xk).mean(0) / (s0 * xk.std(0))
        live &= rho > 0.02
        if not live.any():
            break
        tau[live] += 2.0 * rho[live]
    return tau
