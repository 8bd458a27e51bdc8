"""The sampler-step kernels at their decision edges, against the plain references of tests/sampler_ref.py: the tempering
bisection and importance weights (k_smc_calc_beta: one to five trips per thread of its 1024-thread workgroup, -inf and NaN
likelihoods, exact ties, a strided column), systematic resampling (k_smc_resample: the 8-wide prefix and its tail, u on a
cumulative value, plateaus of zero weights, u beyond the last cumulative value), the proposal factor (k_pop_factor: 63 ..
129 columns, fewer rows than row groups, zero weights, a large mean), and the Metropolis step in pieces that
models/sharded.py runs (k_propose, k_accept, k_like_assemble), step-size tuning and the row gather.

Every input comes from tests/test_sampler_ref_host.py, which checks on the CPU that the arrays hold the edges they are
meant to hold.  Decisions (beta, indices, flags, accepted rows) are compared exactly, rows through their uint64 bits; real
numbers against long double with the bounds derived there and in the tests below."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as sref  # noqa: E402
import test_sampler_ref_host as cases  # noqa: E402
from test_sampler_ref_host import bits  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
INF = float("inf")


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


def dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(torch.device("cuda", 0))


def host(t):
    return t.cpu().numpy()


# ----------------------------------------------------------------------------- tempering step
def _check_weights(w, w_ref, lk, step, what):
    """weight i within (|step (l_i - l_max)| + 8) 2^-52 relative of the long double weight (atol 1e-300: denormal
    weights), an infinite exponent's weight exactly zero, the sum within n 2^-52 of 1"""
    n = lk.size
    assert w.dtype == np.float64 and w.shape == (n,)
    gone = np.isneginf(lk)
    assert (w[gone] == 0.0).all(), what
    rtol = cases.weight_rtol(lk, step)[~gone]
    err = np.abs(w[~gone].astype(LD) - w_ref[~gone])
    allowed = rtol * np.abs(w_ref[~gone]) + LD(1e-300)
    assert (err <= allowed).all(), (what, float((err / allowed).max()))
    assert abs(w.sum() - 1.0) <= n * 2.0 ** -52, (what, w.sum() - 1.0)
    return float((err / allowed).max())


@pytest.mark.parametrize("n", cases.CALC_N)
def test_calc_beta_and_stage_weights_vs_reference(ctx, n):
    worst = 0.0
    for scale, beta_in in cases.CALC_SCALE_BETA:
        lk, b_ref, w_ref, margin = cases.calc_case(n, scale, beta_in)
        b, w = ctx.smc_calc_beta(lk, beta_in, cases.CALC_CV)
        assert b == b_ref, (n, scale, beta_in, b, b_ref)
        worst = max(worst, _check_weights(w, w_ref, lk, b_ref - beta_in, "calc_beta n=%d scale=%g" % (n, scale)))
        for dbeta in cases.STAGE_DBETA:
            ws = ctx.smc_stage_weights(lk, dbeta)
            if dbeta == 0.0:
                assert np.array_equal(ws, np.full(n, 1.0 / n))
            worst = max(worst, _check_weights(ws, sref.stage_weights_ref(lk, dbeta), lk, dbeta,
                                              "stage_weights n=%d scale=%g dbeta=%g" % (n, scale, dbeta)))
    print("n=%d: largest weight error / bound %.3f" % (n, worst))


@pytest.mark.parametrize("n", cases.NAMED_N)
def test_calc_beta_named_cases(ctx, n):
    import torch
    # all likelihoods equal: every term is exp(0), the weights are 1 / n to the bit
    lk, beta_in, b_ref, w_ref, _ = cases.named_case("equal", n)
    b, w = ctx.smc_calc_beta(lk, beta_in, cases.CALC_CV)
    assert b == b_ref and np.array_equal(w, np.full(n, 1.0 / n))
    # three chains without likelihood: weight exactly 0, the others as the reference
    lk, beta_in, b_ref, w_ref, _ = cases.named_case("neginf", n)
    b, w = ctx.smc_calc_beta(lk, beta_in, cases.CALC_CV)
    assert b == b_ref
    _check_weights(w, w_ref, lk, b_ref - beta_in, "three -inf, n=%d" % n)
    for dbeta in cases.STAGE_DBETA[1:]:     # dbeta = 0 is 0 * inf there
        _check_weights(ctx.smc_stage_weights(lk, dbeta), sref.stage_weights_ref(lk, dbeta), lk, dbeta, "three -inf, stage")
    # one NaN likelihood: numpy's maximum propagates it, every comparison of the bisection is false and every weight
    # NaN; the kernel's maximum drops it (block_max_waveorder) and must still end there
    lk, beta_in, b_ref, w_ref, _ = cases.named_case("nan", n)
    b, w = ctx.smc_calc_beta(lk, beta_in, cases.CALC_CV)
    assert b == b_ref and np.isnan(w).all() and np.isnan(w_ref).all()
    if n == 1025:   # the `like` column of a likelihood matrix, stride 5
        from beat_amd.sampler.ops import DeviceOps
        lk, b_ref, w_ref, _ = cases.calc_case(1025, 3.0, 0.3)
        L = torch.full((1025, 5), float("nan"), dtype=torch.float64, device="cuda:0")
        L[:, -1] = dev(lk)
        b, w = DeviceOps(ctx).calc_beta(L[:, -1], 0.3, cases.CALC_CV)
        assert b == b_ref
        _check_weights(host(w), w_ref, lk, b_ref - 0.3, "strided column")
        ws = DeviceOps(ctx).stage_weights(L[:, -1], 0.7)
        _check_weights(host(ws), sref.stage_weights_ref(lk, 0.7), lk, 0.7, "strided column, stage")


def test_calc_beta_exact_tie(ctx):
    """n = 2, the weights underflow to [1, 0]: std / mean == 1.0 == cv at every midpoint and `>` is false"""
    lk, beta_in, b_ref, w_ref, margin = cases.named_case("tie", 2)
    b, w = ctx.smc_calc_beta(lk, beta_in, cases.CALC_CV)
    assert margin == 0.0 and b == b_ref and np.array_equal(w, np.array([1.0, 0.0]))


def test_calc_beta_refuses_a_closed_interval(ctx):
    """beta >= 2 - 1e-6: the reference's loop never runs and it has nothing to return; EINVAL here, not 0 / 0 weights"""
    from beat_amd.sampler.ops import DeviceOps, HostOps
    lk = cases.calc_lk(65, 3.0)
    for beta in (2.0 - 1e-6, 2.0, 2.5, float("nan")):
        with pytest.raises(ValueError):
            ctx.smc_calc_beta(lk, beta, 1.0)
        with pytest.raises(ValueError):
            DeviceOps(ctx).calc_beta(dev(lk), beta, 1.0)
        with pytest.raises(ValueError):
            HostOps().calc_beta(lk, beta, 1.0)
    b, w = ctx.smc_calc_beta(lk, 1.9, 1.0)      # the last admissible interval still halves
    assert b == sref.calc_beta_ref(lk, 1.9, 1.0)[0]


# ----------------------------------------------------------------------------- resampling
def test_resample_indices_equal_reference(ctx):
    for name, w, aux in cases.resample_cases():
        idx = ctx.smc_resample(w, aux)
        ref = sref.resample_ref(w, aux)
        assert idx.dtype == np.int32 and idx.shape == ref.shape
        assert np.array_equal(idx, ref), "%s: first difference at child %d" % (name, int(np.argmax(idx != ref)))
        if name.startswith("short"):
            assert idx[-1] == w.size - 1


@pytest.mark.parametrize("n", [1025, 4097])
def test_resample_device_weights_with_underflow_plateau(ctx, n):
    """the kernel's own weights of a wide likelihood spread: most are exactly 0, the cumulative sum is flat there"""
    lk = cases.calc_lk(n, 400.0)
    w = ctx.smc_stage_weights(lk, 2.0)      # exp(-2 (l_max - l)) is 0 from 373 below the maximum on
    assert (w == 0.0).sum() > n // 2 and (w > 0.0).sum() >= 3 and abs(w.sum() - 1.0) < 1e-12
    _, w_beta = ctx.smc_calc_beta(lk, 0.01, cases.CALC_CV)      # the tempering step's own weights of the same spread
    for weights in (w, w_beta):
        for aux in cases.AUX:
            idx = ctx.smc_resample(weights, aux)
            assert idx.dtype == np.int32 and np.array_equal(idx, sref.resample_ref(weights, aux))


# ----------------------------------------------------------------------------- proposal factor
@pytest.mark.parametrize("n,npar", cases.FACTOR_SHAPES)
def test_population_factor_vs_longdouble(ctx, n, npar):
    """F within 4 (n + 8) 2^-53 sqrt(w_i fact) (sum_k w_k |x_kj| / v1 + |x_ij|) per entry; F^T F against the long double
    np.cov within what that bound e implies, sum_i (|F_ij| e_ik + e_ij |F_ik| + e_ij e_ik), the product formed in long
    double so that it adds no error of its own"""
    worst = 0.0
    for wkind in cases.FACTOR_WEIGHTS:
        for pkind in cases.FACTOR_POPS:
            X, w, F_ref, cov_ref, bound = cases.factor_case(n, npar, wkind, pkind)
            F = ctx.smc_population_factor(X, w)
            assert F.dtype == np.float64 and F.shape == (n, npar)
            err = np.abs(F.astype(LD) - F_ref)
            assert (err <= bound).all(), (wkind, pkind, float((err[bound > 0] / bound[bound > 0]).max()))
            assert (F[w == 0.0] == 0.0).all()
            if (bound > 0).any():
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
            Fl = F.astype(LD)
            assert (np.abs(Fl.T @ Fl - cov_ref) <= cases.factor_cov_tolerance(F_ref, bound)).all(), (wkind, pkind)
    print("population factor (%d, %d): largest error / bound %.3f" % (n, npar, worst))


def test_population_factor_raises_and_recovers(ctx):
    X, w, F_ref, _, bound = cases.factor_case(7, 129, "normalised", "normal")
    with pytest.raises(ValueError, match="Sample covariances contains Inf or NaN"):
        ctx.smc_population_factor(np.array([[0.5, -1.0, 2.0]]), np.array([1.0]))      # a single chain
    F = ctx.smc_population_factor(X, w)        # the call right after a raise is clean
    assert (np.abs(F.astype(LD) - F_ref) <= bound).all()
    Xbad = X.copy()
    Xbad[4, 70] = INF                          # column 70: the second workgroup's
    with pytest.raises(ValueError, match="Sample covariances contains Inf or NaN"):
        ctx.smc_population_factor(Xbad, w)
    F = ctx.smc_population_factor(X, w)
    assert (np.abs(F.astype(LD) - F_ref) <= bound).all()
    ctx.synchronize()


# ----------------------------------------------------------------------------- propose
@pytest.mark.parametrize("npar", cases.PROPOSE_NPARAMS)
def test_propose_bitwise_at_the_box_edges(ctx, npar):
    import torch
    for b in cases.propose_batches(npar):
        C = b["Q0"].shape[0]
        Q0, delta, scaling, lo, up = (dev(b[k]) for k in ("Q0", "delta", "scaling", "lo", "up"))
        Qprop = torch.full((C, npar), -7.0, dtype=torch.float64, device="cuda:0")
        inb = torch.full((C,), -1, dtype=torch.int32, device="cuda:0")
        ctx.metropolis_propose(Q0, delta, scaling, lo, up, Qprop, inb)
        ctx.synchronize()
        Q_ref, inb_ref = sref.propose_ref(b["Q0"], b["delta"], b["scaling"], b["lo"], b["up"])
        got_inb = host(inb)
        assert got_inb.dtype == np.int32
        assert np.array_equal(got_inb, inb_ref), [(n, int(g), int(r)) for n, g, r in zip(b["names"], got_inb, inb_ref) if g != r]
        assert np.array_equal(inb_ref.astype(bool), b["inside"])
        got = host(Qprop)
        for c, name in enumerate(b["names"]):
            assert np.array_equal(bits(got[c]), bits(Q_ref[c])), (npar, name, np.flatnonzero(bits(got[c]) != bits(Q_ref[c]))[:4])
            if not b["inside"][c]:
                assert np.array_equal(bits(got[c]), bits(b["Q0"][c])), (npar, name)
        assert np.array_equal(bits(host(Q0)), bits(b["Q0"])) and np.array_equal(bits(host(delta)), bits(b["delta"]))


# ----------------------------------------------------------------------------- accept
def _run_accept(ctx, a, sel, beta):
    """the chains `sel` of case a through beatamd_metropolis_accept -> (Q0', L0', accepted) and the check that the inputs
    it must not touch are untouched"""
    import torch
    arrs = {k: np.ascontiguousarray(a[k][sel]) for k in ("Q0", "L0", "Qprop", "Lprop", "inbounds", "log_u")}
    d = {k: dev(v) for k, v in arrs.items()}
    acc = torch.full((len(sel),), -1, dtype=torch.int32, device="cuda:0")
    ctx.metropolis_accept(d["Q0"], d["L0"], d["Qprop"], d["Lprop"], d["inbounds"], d["log_u"],
                          dev(beta) if np.ndim(beta) else beta, acc)
    ctx.synchronize()
    for k in ("Qprop", "Lprop", "log_u"):
        assert np.array_equal(bits(host(d[k])), bits(arrs[k])), k
    assert np.array_equal(host(d["inbounds"]), arrs["inbounds"])
    return host(d["Q0"]), host(d["L0"]), host(acc)


def _check_accept(a, sel, got, beta):
    Q1, L1, acc = got
    arrs = [np.ascontiguousarray(a[k][sel]) for k in ("Q0", "L0", "Qprop", "Lprop", "inbounds", "log_u")]
    Q_ref, L_ref, acc_ref = sref.accept_ref(*arrs, beta)
    names = [a["names"][i] for i in sel]
    assert acc.dtype == np.int32
    assert np.array_equal(acc, acc_ref), [(n, int(g), int(r)) for n, g, r in zip(names, acc, acc_ref) if g != r]
    assert np.array_equal(acc_ref.astype(bool), a["accept"][sel])
    for c, name in enumerate(names):
        assert np.array_equal(bits(Q1[c]), bits(Q_ref[c])) and np.array_equal(bits(L1[c]), bits(L_ref[c])), name
        if acc_ref[c]:   # the whole rows of the proposal
            assert np.array_equal(bits(Q1[c]), bits(arrs[2][c])) and np.array_equal(bits(L1[c]), bits(arrs[3][c])), name
        else:            # untouched
            assert np.array_equal(bits(Q1[c]), bits(arrs[0][c])) and np.array_equal(bits(L1[c]), bits(arrs[1][c])), name


@pytest.mark.parametrize("npar,nllk", cases.ACCEPT_SHAPES)
def test_accept_rules_bitwise(ctx, npar, nllk):
    a = cases.accept_case(npar, nllk)
    C = len(a["names"])
    for value in sorted(set(a["beta"].tolist())):          # a scalar beta: the chains that share it
        sel = [c for c in range(C) if a["beta"][c] == value]
        _check_accept(a, sel, _run_accept(ctx, a, sel, value), value)
    sel = list(range(C))                                   # the same values as one beta per chain
    _check_accept(a, sel, _run_accept(ctx, a, sel, a["beta"]), a["beta"])


# ----------------------------------------------------------------------------- like_assemble
@pytest.mark.parametrize("C", cases.ASSEMBLE_C)
def test_like_assemble_bitwise_on_one_gpu(ctx, C):
    import torch
    A = cases.ASSEMBLE
    gathered, local, flagged, nan_datum = cases.assemble_case(C)
    LL = torch.full((C, A["nllk"]), -7.0, dtype=torch.float64, device="cuda:0")
    buf = dev(local)
    assert buf.stride(0) == A["local_width"] > A["col0"] + A["n_rest"]
    ctx.like_assemble(dev(gathered), A["dst_col"], buf, A["col0"], A["n_rest"], A["rest_dst0"], A["group_end"], LL)
    ctx.synchronize()
    ref = sref.like_assemble_ref(gathered, A["dst_col"], local, A["col0"], A["n_rest"], A["rest_dst0"], A["group_end"], A["nllk"])
    got = host(LL)
    diff = np.argwhere(bits(got) != bits(ref))
    assert diff.size == 0, "C=%d: %d entries differ, first (chain, column) %s" % (C, len(diff), diff[:4].tolist())
    assert np.isnan(got[flagged, -1]).all() and np.isnan(got[nan_datum, -1])
    for c in flagged:
        if c != nan_datum:
            assert not np.isnan(got[c, :-1]).any()      # a flagged chain's columns are still scattered


# ----------------------------------------------------------------------------- tuning, gather
def test_metropolis_tune_at_the_table_thresholds(ctx):
    from beat_amd.sampler import step_tune
    C, interval = 257, 1000
    counts = np.array([0, 1, 2, 49, 50, 51, 199, 200, 201, 500, 501, 750, 751, 950, 951, 1000], dtype=np.int32)
    acc = np.resize(counts, C)
    sc = np.linspace(0.25, 3.0, C)
    s_d, a_d = dev(sc), dev(acc)
    ctx.metropolis_tune(s_d, a_d, interval)
    ctx.synchronize()
    ref = step_tune(sc, acc / float(interval))
    assert np.array_equal(bits(host(s_d)), bits(ref))
    assert len(set((ref / sc).round(6).tolist())) == 7          # all seven factors of the table occur
    assert not host(a_d).any()


@pytest.mark.parametrize("ncol", [1, 255, 256, 257])
def test_gather_rows_exact_and_negative_index_raises(ctx, ncol):
    rng = np.random.default_rng(ncol)
    X = rng.standard_normal((9, ncol))
    idx = np.array([8, 7, 6, 5, 4, 3, 2, 1, 0, 0, 0, 8, 8, 3], dtype=np.int32)
    assert np.array_equal(bits(ctx.gather_rows(X, idx)), bits(X[idx]))
    assert np.array_equal(bits(host(ctx.gather_rows(dev(X), dev(idx)))), bits(X[idx]))
    with pytest.raises(IndexError):
        ctx.gather_rows(X, np.array([1, -1, 2], dtype=np.int32))
    assert np.array_equal(ctx.gather_rows(X, idx[:3]), X[idx[:3]])      # the status word was cleared
