"""The references of tests/sampler_ref.py are right, and the inputs of tests/test_gpu_sampler_edges.py are fair (CPU only).

Right: calc_beta_ref, resample_ref and the np.cov of population_factor_ref reproduce the arrays captured from the
reference's own methods (tests/golden/smc.npz); propose_ref + accept_ref agree with HostTarget.astep_batch.  (step_tune
against the golden tune table: tests/test_samplers_cpu.py.)

Fair: the functions below produce every input array of the GPU edge tests, and the conditions those tests lean on are
checked here, so that a failure on the GPU can only be the kernel's: the bisection never comes closer than 1e-10 to its
threshold (a float64 sum of n <= 4097 terms in [0, 1] is off by at most n 2^-53 = 4.6e-13 relative in any order and
cov_temp carries a few such errors: 1e-10 is more than 100 times that), numpy's float64 proposal factor stays inside
the error bound, and the intended edges (u == cum bit for bit, u beyond cum[n-1], q on / one ulp outside a bound, one
rounding != two roundings) are really in the arrays."""
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as sref  # noqa: E402
from conftest import load_golden  # noqa: E402

LD = np.longdouble
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ============================================================================= inputs of the GPU edge tests
# ----------------------------------------------------------------------------- tempering step
CALC_N = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049, 4097)
CALC_SCALE_BETA = ((50.0, 0.0), (3.0, 0.3), (400.0, 0.01))
CALC_CV = 1.0
NAMED_N = (65, 1025)
STAGE_DBETA = (0.0, 1e-3, 0.7)
MARGIN = 1e-10


def calc_lk(n, scale):
    rng = np.random.default_rng(1000 * n + int(scale))
    return rng.standard_normal(n) * scale - 1e3


def named_lk(kind, n):
    """-> (likelihoods, beta_in) of the named tempering cases"""
    if kind == "equal":
        return np.full(n, -123.456), 0.3
    if kind == "neginf":
        lk = calc_lk(n, 3.0)
        lk[[0, n // 2, n - 1]] = -INF
        return lk, 0.3
    if kind == "nan":
        lk = calc_lk(n, 3.0)
        lk[n // 3] = NAN
        return lk, 0.3
    if kind == "tie":   # n = 2: the weights underflow to [1, 0] at every midpoint, std / mean = 1.0 = cv exactly
        return np.array([0.0, -1e12]), 0.0
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def calc_case(n, scale, beta):
    lk = calc_lk(n, scale)
    return (lk,) + sref.calc_beta_ref(lk, beta, CALC_CV)


@functools.lru_cache(maxsize=None)
def named_case(kind, n):
    lk, beta = named_lk(kind, n)
    return (lk, beta) + sref.calc_beta_ref(lk, beta, CALC_CV)


def weight_rtol(lk, step):
    """(|step (l_i - l_max)| + 8) 2^-52 per weight: the rounding of the exponent's argument, one ulp of exp, the sum and
    the division"""
    lk = np.asarray(lk, dtype=np.float64)
    with np.errstate(all="ignore"):
        return (np.abs(step * (lk - np.nanmax(lk))) + 8.0) * 2.0 ** -52


# ----------------------------------------------------------------------------- resampling
RESAMPLE_N = (1, 2, 7, 8, 9, 1023, 1024, 1025, 4097)
AUX = (0.0, 0.5, 1.0 - 2.0 ** -53)
DYADIC_N = (8, 1024, 4096)


def random_weights(n, seed=0):
    w = np.random.default_rng(7000 + 10 * n + seed).random(n)
    return w / w.sum()


def dyadic_weights(n):
    """m_i / n, the integers m_i >= 0 summing to n on a quarter of the entries, the first one zero: every cumulative
    value and, with aux = 0, every u is a multiple of 1 / n, exact in float64 (n a power of two)"""
    rng = np.random.default_rng(8000 + n)
    support = 1 + rng.choice(n - 1, size=max(1, n // 4), replace=False)
    m = np.zeros(n, dtype=np.int64)
    m[support] = rng.multinomial(n, np.full(support.size, 1.0 / support.size))
    assert m.sum() == n and m[0] == 0 and (m == 0).sum() >= n // 2
    return m / float(n)


def onehot_weights(n, at):
    w = np.zeros(n)
    w[at] = 1.0
    return w


def short_weights(n):
    return random_weights(n, seed=1) * (1.0 - 2.0 ** -20)


def resample_cases():
    """-> list of (name, weights, aux)"""
    out = []
    for n in RESAMPLE_N:
        for aux in AUX:
            out.append(("random n=%d aux=%r" % (n, aux), random_weights(n), aux))
        out.append(("short n=%d" % n, short_weights(n), AUX[2]))
    for n in DYADIC_N:
        for aux in AUX:
            out.append(("dyadic n=%d aux=%r" % (n, aux), dyadic_weights(n), aux))
    for n in (9, 1025):
        for at in (0, n // 2, n - 1):
            for aux in AUX:
                out.append(("onehot n=%d at=%d aux=%r" % (n, at, aux), onehot_weights(n, at), aux))
    return out


# ----------------------------------------------------------------------------- proposal factor
FACTOR_SHAPES = ((2, 1), (3, 63), (5, 64), (4, 65), (7, 129), (257, 3), (1030, 65))
FACTOR_WEIGHTS = ("uniform", "normalised", "unnormalised", "zeros")
FACTOR_POPS = ("normal", "offset")


@functools.lru_cache(maxsize=None)
def factor_case(n, npar, wkind, pkind):
    """-> (X, w, F longdouble, cov longdouble, bound longdouble)"""
    rng = np.random.default_rng(9000 + 131 * n + npar + 7 * FACTOR_WEIGHTS.index(wkind) + FACTOR_POPS.index(pkind))
    X = rng.standard_normal((n, npar))
    if pkind == "offset":
        X = 1e8 + X
    if wkind == "uniform":
        w = np.full(n, 1.0 / n)
    else:
        w = rng.random(n) + 0.05
        if wkind == "unnormalised":
            w = w * 37.5
        else:
            if wkind == "zeros":
                w[rng.choice(n, size=n // 3, replace=False)] = 0.0
            w = w / w.sum()
    F, cov, _ = sref.population_factor_ref(X, w)
    return X, w, F, cov, sref.population_factor_bound(X, w)


def factor_cov_tolerance(F, bound):
    """what the per-entry bound e of F implies for F^T F: sum_i (|F_ij| e_ik + e_ij |F_ik| + e_ij e_ik)"""
    A = np.abs(F)
    return A.T @ bound + bound.T @ A + bound.T @ bound


# ----------------------------------------------------------------------------- propose
PROPOSE_NPARAMS = (1, 255, 256, 257, 513)
KFIX = 5            # the fixed parameter (lower == upper) of the batches with more than one parameter
FIXED_AT = 0.25


def _box(npar, fixed):
    k = np.arange(npar)
    lo = -1.0 - 0.25 * (k % 4)
    up = 2.0 + 0.5 * (k % 3)
    if fixed is not None:
        lo[fixed] = up[fixed] = FIXED_AT
    return lo, up


def propose_batches(npar):
    """-> list of batches dict(Q0, delta, scaling, lo, up, names, inside, on): one chain per case, dyadic bounds, starts
    and steps so that the intended q is reached exactly.  `on` lists (chain, k, bound, offset in ulps) of the components
    a case puts on (0) or one ulp outside (-1 below lower, +1 above upper) a bound.  One parameter cannot be free and
    fixed at once: its fixed-parameter chains form a batch of their own."""
    batches = []
    fixed = KFIX if npar > 1 else None
    lo, up = _box(npar, fixed)
    names, rows = [], []
    k_all = np.arange(npar)

    def base():
        q0 = 0.5 + 0.125 * (k_all % 5)
        d = ((k_all % 7) - 3.0) * 0.0625
        if fixed is not None:
            q0[fixed], d[fixed] = FIXED_AT, 0.0
        return q0, d, 2.0

    on = []

    def add(name, inside, hits=(), edit=None):
        q0, d, s = base()
        for (k, which, ulps) in hits:   # start half a unit inside the bound, step onto the target
            b = lo[k] if which == "lo" else up[k]
            t = b
            if ulps < 0:
                t = np.nextafter(b, -INF)
            if ulps > 0:
                t = np.nextafter(b, INF)
            q0[k] = b + 0.5 if which == "lo" else b - 0.5
            d[k] = (t - q0[k]) / s
            on.append((len(rows), k, which, ulps))
        if edit is not None:
            q0, d, s = edit(q0, d, s)
        names.append(name)
        rows.append((q0, d, s, inside))

    last = npar - 1
    add("inside", True)
    if npar > 1:
        add("on lower and on upper", True, hits=((1, "lo", 0), (last - 1, "up", 0)))
    else:
        add("on lower", True, hits=((0, "lo", 0),))
        add("on upper", True, hits=((0, "up", 0),))
    add("ulp below lower, k=0", False, hits=((0, "lo", -1),))
    add("ulp below lower, k=last", False, hits=((last, "lo", -1),))
    if npar > 256:
        add("ulp below lower, k=256", False, hits=((256, "lo", -1),))
    add("ulp above upper", False, hits=((npar // 2, "up", +1),))

    def with_delta(k, v):
        def edit(q0, d, s):
            d[k] = v
            return q0, d, s
        return edit
    add("delta NaN", False, edit=with_delta(min(1, last), NAN))
    add("delta +inf", False, edit=with_delta(max(last - 1, 0), INF))
    if fixed is not None:
        add("fixed parameter, delta 0", True)
        add("fixed parameter moved", False, edit=with_delta(fixed, 2.0 ** -40))

    def scaling_zero(q0, d, s):
        d = 1e300 * (1.0 + (k_all % 3))   # finite: delta * 0 = 0
        return q0, d, 0.0
    add("scaling 0", True, edit=scaling_zero)

    def two_roundings(q0, d, s):
        q0 = np.full(npar, -1.0)
        d = 1.0 + 2.0 ** -30 * (2 * (k_all % 50) + 1)
        if fixed is not None:
            q0[fixed], d[fixed] = FIXED_AT, 0.0
        return q0, d, 1.0 + 2.0 ** -30
    add("two roundings", True, edit=two_roundings)
    batches.append(_propose_batch(names, rows, lo, up, on))

    if npar == 1:
        lo, up = _box(1, 0)
        names, rows, on = [], [], []

        def base():     # noqa: F811 (the fixed batch's chains sit on the fixed value)
            return np.array([FIXED_AT]), np.array([0.0]), 2.0
        add("fixed parameter, delta 0", True)
        add("fixed parameter moved", False, edit=with_delta(0, 2.0 ** -40))
        add("fixed parameter, scaling 0", True, edit=lambda q0, d, s: (q0, np.array([1e300]), 0.0))
        batches.append(_propose_batch(names, rows, lo, up, on))
    return batches


def _propose_batch(names, rows, lo, up, on):
    return dict(names=names, lo=lo, up=up, on=on,
                Q0=np.ascontiguousarray(np.stack([r[0] for r in rows])),
                delta=np.ascontiguousarray(np.stack([r[1] for r in rows])),
                scaling=np.array([r[2] for r in rows], dtype=np.float64),
                inside=np.array([r[3] for r in rows], dtype=bool))


# ----------------------------------------------------------------------------- accept
ACCEPT_SHAPES = ((1, 1), (257, 2), (3, 257), (300, 300))
BETA = 0.37


def accept_case(npar, nllk):
    """-> dict(Q0, L0, Qprop, Lprop, inbounds, log_u, beta [C], names, accept [C] bool): one chain per rule"""
    rng = np.random.default_rng(6000 + 1000 * npar + nllk)
    spec = [  # name, l0, lp, log_u (callable of mr or a value), beta, inbounds, accepted
        ("better, ordinary log u", -10.5, -9.25, -0.3, BETA, 1, True),
        ("log u == mr", -10.5, -11.75, lambda mr: mr, BETA, 1, False),
        ("log u one ulp below mr", -10.5, -11.75, lambda mr: np.nextafter(mr, -INF), BETA, 1, True),
        ("lp NaN", -10.5, NAN, -1.0, BETA, 1, False),
        ("lp +inf", -10.5, INF, -1.0, BETA, 1, False),
        ("lp -inf", -10.5, -INF, -INF, BETA, 1, False),
        ("l0 -inf", -INF, -9.25, -1.0, BETA, 1, False),
        ("l0 NaN", NAN, -9.25, -1.0, BETA, 1, False),
        ("both -inf", -INF, -INF, -1.0, BETA, 1, False),
        ("beta 0, finite", -10.5, -2000.0, -0.5, 0.0, 1, True),
        ("beta 0, lp +inf", -10.5, INF, -0.5, 0.0, 1, False),
        ("log u -inf, finite mr", -10.5, -1e6, -INF, BETA, 1, True),
        ("outside the box, stale row", -1e6, 0.0, -INF, BETA, 0, False),
    ]
    C = len(spec)
    Q0, Qprop = rng.standard_normal((C, npar)), rng.standard_normal((C, npar))
    L0, Lprop = rng.standard_normal((C, nllk)), rng.standard_normal((C, nllk))
    log_u, beta = np.empty(C), np.empty(C)
    for c, (_, l0, lp, lu, b, _, _) in enumerate(spec):
        L0[c, -1], Lprop[c, -1], beta[c] = l0, lp, b
        with np.errstate(all="ignore"):
            mr = np.float64(b) * (np.float64(lp) - np.float64(l0))
        log_u[c] = lu(mr) if callable(lu) else lu
    Lprop[C - 1, :-1] = NAN     # the parked chain's row was not evaluated: whatever an earlier step left there
    return dict(Q0=Q0, L0=L0, Qprop=Qprop, Lprop=Lprop, log_u=log_u, beta=beta,
                inbounds=np.array([s[5] for s in spec], dtype=np.int32), names=[s[0] for s in spec],
                accept=np.array([s[6] for s in spec], dtype=bool))


# ----------------------------------------------------------------------------- like_assemble
ASSEMBLE_C = (1, 255, 256, 257)
ASSEMBLE = dict(nllk=9, dst_col=(4, 0, 2, -1, 5, 1, 3, -1), col0=3, n_rest=2, rest_dst0=6, group_end=(3, 6, 8),
                local_width=12)


def assemble_case(C):
    """-> (gathered [8, C], local [C, 12], flagged chains, chain with a NaN datum): two ranks of three data rows and a
    flag row each; values of mixed magnitude so that another summation order gives other bits"""
    rng = np.random.default_rng(5000 + C)
    mag = np.array([1e16, -1e16, 1.0, 1e-3])

    def values(shape):
        return mag[rng.integers(0, 4, shape)] * (0.5 + rng.random(shape))
    gathered = values((8, C))
    gathered[3], gathered[7] = 0.0, 0.0
    flagged = sorted({0, C // 2, C - 1})
    gathered[7, flagged] = NAN
    nan_datum = min(3, C - 1)
    gathered[1, nan_datum] = NAN
    local = values((C, ASSEMBLE["local_width"]))
    return gathered, local, flagged, nan_datum


# ============================================================================= the references are right
def test_references_reproduce_the_reference_golden():
    g = load_golden("smc")
    for k in range(int(g["ncase"])):
        lk, beta_in = g["c%d_lk" % k], float(g["c%d_beta_in" % k])
        b, w, _ = sref.calc_beta_ref(lk, beta_in, 1.0)
        assert b == float(g["c%d_beta" % k])
        gw = g["c%d_w" % k]
        err = np.abs(w - gw.astype(LD)) / gw.astype(LD)
        print("case %d: weights %.2e relative" % (k, float(err.max())))
        assert float(err.max()) <= 1e-15
        idx = sref.resample_ref(gw, float(np.ravel(g["c%d_aux" % k])[0]))
        assert np.array_equal(idx, g["c%d_idx" % k])
        F, cov, _ = sref.population_factor_ref(g["c%d_pop" % k], gw)
        # relative to the matrix (its largest entry): the golden is numpy's float64 np.cov bit for bit, and the float64
        # rounding of its own n-term sums is 1.1e-15 .. 7.9e-15 of a single small entry in these four cases (measured
        # against this long double evaluation), 2.6e-16 .. 5.8e-16 of the matrix
        gc = g["c%d_cov" % k].astype(LD)
        d = np.abs(cov - gc)
        print("case %d: cov %.2e of the matrix, %.2e of single entries" % (k, float(d.max() / np.abs(gc).max()),
                                                                         float((d / np.abs(gc)).max())))
        assert float(d.max() / np.abs(gc).max()) <= 1e-15
        # F^T F is that covariance: the two long double evaluations agree far below float64's resolution
        assert float(np.abs(F.T @ F - cov).max() / np.abs(cov).max()) <= 1e-17


def test_stage_weights_ref_is_the_formula():
    lk = calc_lk(65, 3.0)
    t = np.exp(0.7 * (lk - lk.max()))
    np.testing.assert_allclose(sref.stage_weights_ref(lk, 0.7).astype(np.float64), t / t.sum(), rtol=1e-15)
    assert np.array_equal(sref.stage_weights_ref(lk, 0.0), np.full(65, LD(1) / LD(65)))


@pytest.mark.parametrize("per_chain_beta", [False, True])
def test_propose_and_accept_refs_agree_with_host_target(per_chain_beta):
    import torch
    from beat_amd.sampler.hosttarget import HostTarget
    rng = np.random.default_rng(11)
    C, npar = 200, 4

    def fn(q):
        return -0.5 * (q * q).sum(1) + np.where(q[:, 0] > 1.0, NAN, 0.0)   # some proposals have no likelihood
    target = HostTarget(fn, npar)
    Q0 = rng.uniform(-1.5, 1.5, (C, npar))
    L0 = fn(Q0).reshape(C, 1)
    delta, scaling = rng.standard_normal((C, npar)), rng.uniform(0.1, 1.0, C)
    lo, up = np.full(npar, -1.5), np.full(npar, 1.5)
    log_u = np.log(rng.random(C))
    beta = rng.uniform(0.0, 1.0, C) if per_chain_beta else 0.6
    Qp, inb = sref.propose_ref(Q0, delta, scaling, lo, up)
    assert 20 < inb.sum() < C - 20
    Q1, L1, acc = sref.accept_ref(Q0, L0, Qp, fn(Qp).reshape(C, 1), inb, log_u, beta)
    assert 20 < acc.sum() < inb.sum()
    tq, tl = torch.from_numpy(Q0.copy()), torch.from_numpy(L0.copy())
    got = target.astep_batch(tq, tl, torch.from_numpy(delta), torch.from_numpy(scaling), torch.from_numpy(lo),
                             torch.from_numpy(up), torch.from_numpy(log_u),
                             torch.from_numpy(beta) if per_chain_beta else beta)
    assert np.array_equal(got.numpy(), acc)
    assert np.array_equal(bits(tq.numpy()), bits(Q1)) and np.array_equal(bits(tl.numpy()), bits(L1))


def test_like_assemble_ref_on_a_hand_case():
    gathered = np.array([[1.0], [2.0], [0.0], [4.0], [NAN]])
    local = np.array([[9.0, 8.0, 7.0]])
    LL = sref.like_assemble_ref(gathered, (1, 0, -1, 2, -1), local, 1, 2, 3, (2, 5), 6)
    assert LL[0, :5].tolist() == [2.0, 1.0, 4.0, 8.0, 7.0] and math.isnan(LL[0, 5])
    gathered[4, 0] = 0.0
    LL = sref.like_assemble_ref(gathered, (1, 0, -1, 2, -1), local, 1, 2, 3, (2, 5), 6)
    assert LL[0, 5] == (2.0 + 1.0) + (4.0 + 8.0 + 7.0)


def test_host_ops_calc_beta_refuses_a_closed_interval():
    from beat_amd.sampler.ops import HostOps
    lk = calc_lk(65, 3.0)
    for beta in (2.0 - 1e-6, 2.0, 3.0):
        with pytest.raises(ValueError):
            HostOps().calc_beta(lk, beta, 1.0)
        with pytest.raises(ValueError):
            sref.calc_beta_ref(lk, beta, 1.0)
    b, _ = HostOps().calc_beta(lk, 1.9, 1.0)
    assert b == sref.calc_beta_ref(lk, 1.9, 1.0)[0]


# ============================================================================= the inputs are fair
def test_bisection_margin_of_every_tempering_case():
    smallest = INF
    for n in CALC_N:
        for scale, beta in CALC_SCALE_BETA:
            lk, b, w, margin = calc_case(n, scale, beta)
            if n == 2 and margin < MARGIN:
                assert_two_chain_tie(lk, beta)
                continue
            smallest = min(smallest, float(margin))
            assert margin >= MARGIN, (n, scale, beta, margin)
    for n in NAMED_N:
        for kind in ("equal", "neginf"):
            margin = float(named_case(kind, n)[4])
            smallest = min(smallest, margin)
            assert margin >= MARGIN, (kind, n, margin)
    print("smallest |cov_temp - cv| over all bisections: %.3e" % smallest)


def assert_two_chain_tie(lk, beta):
    """Two chains and cv = 1: std / mean = (1 - t) / (1 + t) <= 1 with t the smaller of the two terms, so no margin can
    be kept towards the threshold -- (2, 50, 0.0) and (2, 400, 0.01) sit ON it.  What makes them fair instead: at every
    midpoint t is below 2^-64, so 1 + t = 1, mean = 0.5, both deviations 0.5 and std / mean = 1.0 exactly in float64 in
    any order and with any exp that is a few ulps off: the decision is the tie's (`>` is false), as in the named case"""
    path = []
    b = sref.calc_beta_ref(lk, beta, CALC_CV, path=path)[0]
    assert len(path) >= 20 and 2.0 - b <= 1e-6
    for mid, gap in path:
        t = np.exp((mid - beta) * (lk - lk.max()))
        assert gap == 0.0 and t.max() == 1.0 and t.min() < 2.0 ** -64, (mid, gap, t)


def test_named_tempering_cases_are_what_they_claim():
    lk, beta, b, w, margin = named_case("tie", 2)
    assert margin == 0.0 and np.array_equal(w, np.array([1, 0], dtype=LD))   # cov_temp == cv at every midpoint
    assert 2.0 - b <= 1e-6                                                   # `>` is false: the lower end moved up
    for n in NAMED_N:
        lk, beta, b, w, margin = named_case("nan", n)
        assert np.isnan(w).all() and np.isnan(margin) and 2.0 - b <= 1e-6    # every comparison false, as in numpy
        lk, beta, b, w, margin = named_case("equal", n)
        assert np.array_equal(w.astype(np.float64), np.full(n, 1.0 / n))
        lk, beta, b, w, margin = named_case("neginf", n)
        assert (w[[0, n // 2, n - 1]] == 0).all() and (np.delete(w, [0, n // 2, n - 1]) > 0).all()


def test_resample_cases_contain_their_edges():
    seen = {"tie": 0, "plateau": 0, "short": 0}
    for name, w, aux in resample_cases():
        u, cum = sref.resample_u_cum(w, aux)
        n = w.size
        if name.startswith("dyadic") and aux == 0.0:
            # every cumulative value below 1 is some u, bit for bit; the u between two of them lie on no plateau's edge
            assert np.isin(bits(cum[cum < 1.0]), bits(u)).all() and np.unique(cum).size >= 3, name
            assert w[0] == 0.0 and u[0] == cum[0] == 0.0
            assert (np.diff(cum) == 0).sum() >= n // 2 - 1      # plateaus
            idx = sref.resample_ref(w, aux)
            hit = np.isin(bits(u), bits(cum))
            assert hit.sum() >= 2 and (cum[idx[hit]] == u[hit]).all()
            assert idx[0] == 0 and (w[idx[1:]] > 0).all()       # the left-most index of a plateau: where it was reached
            seen["tie"] += 1
            seen["plateau"] += 1
        if name.startswith("short"):
            assert u[n - 1] > cum[n - 1], name
            assert sref.resample_ref(w, aux)[n - 1] == n - 1
            seen["short"] += 1
        assert abs(cum[-1] - 1.0) < 1e-5
        idx = sref.resample_ref(w, aux)     # the smallest j with u <= cum[j], or n - 1
        below = np.concatenate(([-INF], cum[:-1]))[idx]
        assert ((u <= cum[idx]) | (idx == n - 1)).all() and (below < u).all(), name
    assert seen["tie"] == len(DYADIC_N) and seen["short"] == len(RESAMPLE_N)


def test_factor_cases_numpy_float64_stays_inside_the_bound():
    worst = 0.0
    for n, npar in FACTOR_SHAPES:
        for wkind in FACTOR_WEIGHTS:
            for pkind in FACTOR_POPS:
                X, w, F, cov, bound = factor_case(n, npar, wkind, pkind)
                v1, v2 = w.sum(), (w * w).sum()
                mean = (w[:, None] * X).sum(0) / v1
                F64 = np.sqrt(w / (v1 - v2 / v1))[:, None] * (X - mean)
                assert np.isfinite(F64).all()
                err = np.abs(F64.astype(LD) - F)
                assert (err <= bound).all(), (n, npar, wkind, pkind)
                with np.errstate(all="ignore"):
                    worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0))))
                if wkind == "zeros":
                    assert (w == 0).sum() == n // 3 and (F[w == 0] == 0).all()
                # F^T F of the long double factor is the long double np.cov: the two evaluations differ by the 2^-11 of
                # the tolerance that long double has over float64, times small factors (measured: at most 0.005)
                assert (np.abs(F.T @ F - cov) <= 0.02 * factor_cov_tolerance(F, bound) + LD(1e-300)).all()
    print("numpy float64 factor: largest error / bound = %.3f" % worst)


def test_propose_cases_land_where_they_claim():
    for npar in PROPOSE_NPARAMS:
        batches = propose_batches(npar)
        names = sum((b["names"] for b in batches), [])
        for want in ("inside", "ulp below lower, k=0", "ulp below lower, k=last", "ulp above upper", "delta NaN",
                     "delta +inf", "fixed parameter, delta 0", "fixed parameter moved", "two roundings"):
            assert want in names, (npar, want)
        assert ("ulp below lower, k=256" in names) == (npar > 256)
        assert any(n.startswith("scaling 0") or n.endswith("scaling 0") for n in names)
        for b in batches:
            Q0, delta, s, lo, up = b["Q0"], b["delta"], b["scaling"], b["lo"], b["up"]
            Qp, inb = sref.propose_ref(Q0, delta, s, lo, up)
            assert np.array_equal(inb.astype(bool), b["inside"]), (npar, b["names"], inb)
            with np.errstate(all="ignore"):
                q = Q0 + delta * s[:, None]
            for (c, k, which, ulps) in b["on"]:
                bound = lo[k] if which == "lo" else up[k]
                target = bound if ulps == 0 else np.nextafter(bound, -INF if ulps < 0 else INF)
                assert bits(q[c, k]) == bits(target), (npar, b["names"][c], k)
                # every other component of that chain is strictly inside: the case hangs on this one alone
                others = np.delete(np.arange(npar), [k2 for (c2, k2, _, _) in b["on"] if c2 == c])
                assert ((q[c, others] >= lo[others]) & (q[c, others] <= up[others])).all()
            for c, name in enumerate(b["names"]):
                if name == "two roundings":
                    one = (delta[c].astype(LD) * LD(s[c]) + Q0[c].astype(LD)).astype(np.float64)   # exact, rounded once
                    free = lo != up
                    assert (bits(one[free]) != bits(q[c][free])).all()
                    assert ((one >= lo) & (one <= up)).all()      # a fused step would be inside too, with other bits
                if "fixed parameter" in name:
                    k = KFIX if npar > 1 else 0
                    assert lo[k] == up[k] and (q[c, k] == lo[k]) == b["inside"][c]
                if "scaling 0" in name:
                    assert np.array_equal(bits(q[c]), bits(Q0[c]))
            assert np.array_equal(bits(Qp[~b["inside"]]), bits(Q0[~b["inside"]]))


def test_accept_cases_are_what_they_claim():
    for npar, nllk in ACCEPT_SHAPES:
        a = accept_case(npar, nllk)
        Q1, L1, acc = sref.accept_ref(a["Q0"], a["L0"], a["Qprop"], a["Lprop"], a["inbounds"], a["log_u"], a["beta"])
        assert np.array_equal(acc.astype(bool), a["accept"]), list(zip(a["names"], acc))
        with np.errstate(all="ignore"):
            mr = a["beta"] * (a["Lprop"][:, -1] - a["L0"][:, -1])
        i = a["names"].index("log u == mr")
        assert bits(a["log_u"][i]) == bits(mr[i]) and math.isfinite(mr[i])
        assert a["log_u"][i + 1] < mr[i + 1] and np.nextafter(a["log_u"][i + 1], INF) == mr[i + 1]
        # the infinite-ratio chains would be accepted by `log u < mr` alone: only the finiteness rule rejects them
        for name in ("lp +inf", "l0 -inf"):
            i = a["names"].index(name)
            assert mr[i] == INF and a["log_u"][i] < mr[i] and not acc[i]
        i = a["names"].index("outside the box, stale row")
        assert a["inbounds"][i] == 0 and mr[i] > 0 and a["log_u"][i] < mr[i]    # inside the box it would be taken
        assert nllk == 1 or np.isnan(a["Lprop"][i, :-1]).all()


def test_assemble_cases_depend_on_the_summation_order():
    for C in ASSEMBLE_C:
        gathered, local, flagged, nan_datum = assemble_case(C)
        A = ASSEMBLE
        LL = sref.like_assemble_ref(gathered, A["dst_col"], local, A["col0"], A["n_rest"], A["rest_dst0"], A["group_end"],
                                    A["nllk"])
        assert sorted(d for d in A["dst_col"] if d >= 0) == list(range(6))
        assert np.isnan(LL[flagged, -1]).all() and np.isnan(LL[nan_datum, -1])
        assert not np.isnan(LL[flagged, :6]).any() or nan_datum in flagged      # flagged chains keep their data columns
        ok = ~np.isnan(LL[:, -1])
        assert ok.sum() == C - len(set(flagged) | {nan_datum})
        if C > 1:
            running = np.zeros(C)
            for k in range(8):
                running = running + LL[:, k]                # one running sum over all composites
            assert (running[ok] != LL[ok, -1]).sum() > C // 8
