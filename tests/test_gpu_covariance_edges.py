"""The per-stage noise-covariance update at the shapes it runs at, against float64 restatements of the reference
route computed here: the blocked Cholesky whitening (csrc/chol.hip) across its 64-wide diagonal blocks and
CH_NBO-wide outer panels up to the bench trace length, its per-matrix failure flags, the autocovariance
(bitwise, up to its LDS limit), the scaled Toeplitz assembly (bitwise, past its grid-stride limit), the whitening
ratio / unwhitening at the same sizes, and one NoiseCovarianceUpdate at N = 4096.

Bounds are formulas of n, u = 2^-53 and the condition number kappa of the matrix, with c = 4 throughout:
a backward-stable factorisation or solve perturbs its input by at most c n u relative, the output then moves by at
most kappa times that."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
C_RND = 4.0


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


# ----------------------------------------------------------------------------- float64 restatements
def ref_whitening(C):
    """heart.py:216-245: W = cholesky(inv(C)).T, log_pdet = 2 sum log diag cholesky(C)"""
    W = np.linalg.cholesky(np.linalg.inv(C)).T
    return W, 2.0 * np.log(np.diag(np.linalg.cholesky(C))).sum()


def ref_running_window_rms(d, w):
    """utility.py:1141-1161, mode="same" """
    return np.sqrt(np.convolve(np.power(d, 2), np.ones(w) / float(w), "same"))


def ref_autocov_lags(x, mean, lags):
    """covariance.py:716-736 for every row of x at the given lags: autocov[j] starts at 0.0 and adds
    (x[j+k] - mean) * (x[k] - mean) for k = 0, 1, ... in order (a cumulative sum is that loop), then / n"""
    nd, n = x.shape
    s = x - mean[:, None]
    out = np.empty((nd, len(lags)))
    z = np.zeros((nd, 1))
    for i, j in enumerate(lags):
        out[:, i] = np.cumsum(np.concatenate([z, s[:, j:] * s[:, :n - j]], 1), axis=1)[:, -1] / n
    return out


def ref_autocov(x):
    n = x.size
    return ref_autocov_lags(x.reshape(1, -1), np.array([x.mean()]), range(n))[0]


def ref_non_toeplitz(d, w):
    """covariance.py:739-771"""
    from scipy.linalg import toeplitz
    stds = ref_running_window_rms(d, w)
    return toeplitz(ref_autocov(d / stds)) * stds[:, np.newaxis] * stds[np.newaxis, :]


# ----------------------------------------------------------------------------- test matrices, kappa known
def exp_toeplitz(n, rho):
    """the reference's exponential structure rho^|i-j| (Kac-Murdock-Szego): its eigenvalues lie in
    ((1-rho)/(1+rho), (1+rho)/(1-rho)), so kappa < ((1+rho)/(1-rho))^2"""
    i = np.arange(n)
    return rho ** np.abs(i[:, None] - i[None, :]).astype(np.float64), ((1 + rho) / (1 - rho)) ** 2


def random_spd(n, kappa, rng):
    """Q diag(lambda) Q^T, lambda log-spaced over [1, kappa]"""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    C = (Q * np.logspace(0.0, np.log10(kappa), n)) @ Q.T
    return 0.5 * (C + C.T), float(kappa)


def non_toeplitz(n, rng):
    """the update's matrix: running-window rms and autocovariance of a noise trace (window n // 5)"""
    d = rng.standard_normal(n) * (1.0 + 0.5 * np.sin(np.arange(n) * (6.0 / n)))
    C = ref_non_toeplitz(d, max(n // 5, 1))
    ev = np.linalg.eigvalsh(C)
    assert ev[0] > 0
    return C, ev[-1] / ev[0]


def spd_kappa(n):
    return 1e6 if n <= 600 else (1e5 if n <= 1600 else 1e3)


def three_kinds(n, seed):
    rng = np.random.default_rng(seed)
    mats = [exp_toeplitz(n, np.exp(-1.0 / 5.0)), random_spd(n, spd_kappa(n), rng), non_toeplitz(n, rng)]
    return np.stack([m for m, _ in mats]), np.array([k for _, k in mats])


def check_whitening(W, lp, C, kappa, W_ref=None, lp_ref=None, what=""):
    n = C.shape[0]
    if W_ref is None:
        W_ref, lp_ref = ref_whitening(C)
    assert np.array_equal(np.tril(W, -1), np.zeros((n, n))), what + ": not upper triangular"
    # W: forward error of a Cholesky factor (of inv(C)) after a relative backward error c n u is kappa times that
    err = np.abs(W - W_ref).max()
    tol = C_RND * n * U * kappa * np.abs(W_ref).max()
    assert err <= tol, "%s: |W - W_ref| = %.3e > c n u kappa |W_ref| = %.3e" % (what, err, tol)
    # W^T W C - I = inv(C) dC for the backward error dC (c n u |C|): at most c n u kappa
    res = np.abs(W.T @ (W @ C) - np.eye(n)).max()
    tol = C_RND * n * U * kappa
    assert res <= tol, "%s: |W^T W C - I| = %.3e > c n u kappa = %.3e" % (what, res, tol)
    # log det: each of the n eigenvalue logs moves by at most |inv(C) dC| <= c n u kappa
    tol = C_RND * n * n * U * kappa
    assert abs(lp - lp_ref) <= tol, "%s: log_pdet %r vs %r (bound %.3e)" % (what, lp, lp_ref, tol)
    sl = np.linalg.slogdet(C)
    assert sl[0] == 1.0 and abs(lp - sl[1]) <= tol, "%s: log_pdet %r vs slogdet %r" % (what, lp, sl[1])


# ----------------------------------------------------------------------------- 1. blocked Cholesky whitening
@pytest.mark.parametrize("n", [63, 64, 65, 127, 255, 256, 257, 511, 512, 513, 769, 1025, 1500])
def test_chol_inverse_block_edges(ctx, n):
    """around the 64-wide diagonal blocks and 256-wide outer panels: exponential Toeplitz, random SPD
    (kappa 1e6 .. 1e5) and the update's scaled non-Toeplitz matrix in one batch of 3, each one also alone"""
    Cs, kap = three_kinds(n, 1000 + n)
    W, lp = ctx.chol_inverse_batch(Cs)
    for i in range(3):
        check_whitening(W[i], lp[i], Cs[i], kap[i], what="n=%d kind %d" % (n, i))
        W1, lp1 = ctx.chol_inverse_batch(Cs[i:i + 1])
        assert np.array_equal(W1[0], W[i]) and lp1[0] == lp[i], "n=%d kind %d: batch of 1 != batch of 3" % (n, i)


@pytest.fixture(scope="module")
def bench_length(ctx):
    """n = 4096 (the bench trace length), a batch of 3 kinds, on the device and the reference's"""
    n = 4096
    Cs, kap = three_kinds(n, 4096)
    W, lp = ctx.chol_inverse_batch(Cs)
    refs = [ref_whitening(C) for C in Cs]
    return Cs, kap, W, lp, refs


def test_chol_inverse_bench_trace_length(bench_length):
    Cs, kap, W, lp, refs = bench_length
    for i in range(len(Cs)):
        check_whitening(W[i], lp[i], Cs[i], kap[i], refs[i][0], refs[i][1], what="n=4096 kind %d" % i)


@pytest.mark.parametrize("n", [120, 513])
def test_chol_inverse_batch_of_64(ctx, n):
    """one matrix per bench target: 64 different matrices (the three kinds, varied) in one call"""
    import torch
    rng = np.random.default_rng(64 + n)
    mats = []
    for t in range(64):
        k = t % 3
        if k == 0:
            mats.append(exp_toeplitz(n, np.exp(-1.0 / (2.0 + t / 4.0))))
        elif k == 1:
            mats.append(random_spd(n, 10.0 ** (2 + 4 * t / 63.0), rng))
        else:
            mats.append(non_toeplitz(n, rng))
    Cs, kap = np.stack([m for m, _ in mats]), [k for _, k in mats]
    W, lp = ctx.chol_inverse_batch(torch.from_numpy(Cs).to("cuda:0"))
    W, lp = W.cpu().numpy(), lp.cpu().numpy()
    for t in range(64):
        check_whitening(W[t], lp[t], Cs[t], kap[t], what="n=%d target %d" % (n, t))
    for t in (0, 37, 63):
        W1, lp1 = ctx.chol_inverse_batch(Cs[t:t + 1])
        assert np.array_equal(W1[0], W[t]) and lp1[0] == lp[t]


_NBO_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import beat_amd
ctx = beat_amd.get_context(0)
inp = np.load(sys.argv[2])
out = {}
for key in inp.files:
    W, lp = ctx.chol_inverse_batch(inp[key])
    out[key + "_W"], out[key + "_lp"] = W, lp
np.savez(sys.argv[3], **out)
"""


def test_chol_inverse_outer_panel_width(tmp_path):
    """BEATAMD_CHOL_NBO (read once per process) in {64, 128, 256, 512, 1024}, each in a fresh child process: every
    width meets the bound against the reference, and the widths agree with each other within the same bound"""
    sizes = (257, 513, 1025)
    inp = {}
    kap = {}
    for n in sizes:
        inp["n%d" % n], kap[n] = three_kinds(n, 7 * n)
    np.savez(tmp_path / "in.npz", **inp)
    refs = {n: [ref_whitening(C) for C in inp["n%d" % n]] for n in sizes}
    got = {}
    for nbo in (64, 128, 256, 512, 1024):
        env = dict(os.environ, BEATAMD_CHOL_NBO=str(nbo))
        outp = tmp_path / ("nbo%d.npz" % nbo)
        r = subprocess.run([sys.executable, "-c", _NBO_CHILD, ROOT, str(tmp_path / "in.npz"), str(outp)], env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, "BEATAMD_CHOL_NBO=%d: rc %d\n%s" % (nbo, r.returncode, r.stderr[-3000:])
        got[nbo] = dict(np.load(outp))
    for n in sizes:
        Cs = inp["n%d" % n]
        for i in range(3):
            W_ref, lp_ref = refs[n][i]
            tol = C_RND * n * U * kap[n][i] * np.abs(W_ref).max()
            for nbo in got:
                W, lp = got[nbo]["n%d_W" % n][i], got[nbo]["n%d_lp" % n][i]
                check_whitening(W, lp, Cs[i], kap[n][i], W_ref, lp_ref, what="NBO=%d n=%d kind %d" % (nbo, n, i))
                d = np.abs(W - got[256]["n%d_W" % n][i]).max()
                assert d <= tol, "NBO=%d vs 256, n=%d kind %d: %.3e > %.3e" % (nbo, n, i, d, tol)
    # the knob took effect: one 1024-wide panel sums the trailing update in another order than 16 64-wide ones
    assert not np.array_equal(got[64]["n1025_W"], got[1024]["n1025_W"])


# ----------------------------------------------------------------------------- 2. failure flags
@pytest.mark.parametrize("n", [513, 1025])
def test_chol_flags_name_the_failing_matrices(ctx, n):
    """matrices that fail in the first diagonal block, in the last (padded) one, in the middle of the second outer
    panel, and a NaN matrix: the flags name exactly those; every other matrix comes out bitwise as in a batch where
    the failing ones are replaced by good ones; the raising variant raises and leaves the context usable"""
    rng = np.random.default_rng(n)
    good = [exp_toeplitz(n, np.exp(-1.0 / 3.0))[0], non_toeplitz(n, rng)[0], random_spd(n, 1e4, rng)[0],
            exp_toeplitz(n, np.exp(-1.0 / 9.0))[0]]

    # the factorisation runs on A = J C J: pivot k of A fails when C[n-1-k, n-1-k] = -1 (the leading k x k block of A
    # is untouched and positive definite, the Schur complement at k is -1 - (something >= 0))
    def failing_at(k, base):
        C = base.copy()
        C[n - 1 - k, n - 1 - k] = -1.0
        return C
    nan = np.full((n, n), np.nan)
    pivots = {"first block": 10, "second outer panel": 256 + 128 + 5, "last block": n - 1}
    batch = np.stack([good[0], failing_at(pivots["first block"], good[1]), good[1],
                      failing_at(pivots["second outer panel"], good[0]), good[2], nan, good[3],
                      failing_at(pivots["last block"], good[2])])
    expect = [0, 1, 0, 1, 0, 1, 0, 1]
    W, lp, bad = ctx.chol_inverse_batch_flags(batch)
    assert bad.tolist() == expect, "flags %s, expected %s" % (bad.tolist(), expect)
    fixed = batch.copy()
    for t in np.flatnonzero(expect):
        fixed[t] = good[t % 4]
    W2, lp2, bad2 = ctx.chol_inverse_batch_flags(fixed)
    assert bad2.tolist() == [0] * len(expect)
    for t in np.flatnonzero(np.array(expect) == 0):
        assert np.array_equal(W[t], W2[t]) and lp[t] == lp2[t], "matrix %d depends on its neighbours" % t
    W3, lp3 = ctx.chol_inverse_batch(fixed)
    assert np.array_equal(W3, W2) and np.array_equal(lp3, lp2)
    for t in range(len(expect)):
        check_whitening(W2[t], lp2[t], fixed[t], float(np.linalg.cond(fixed[t])), what="n=%d matrix %d" % (n, t))
    for name, k in pivots.items():
        with pytest.raises(np.linalg.LinAlgError):
            ctx.chol_inverse_batch(np.stack([good[0], failing_at(k, good[0])]))
    with pytest.raises(np.linalg.LinAlgError):
        ctx.chol_inverse_batch(nan[None])
    W4, lp4 = ctx.chol_inverse_batch(fixed)
    assert np.array_equal(W4, W2) and np.array_equal(lp4, lp2)


# ----------------------------------------------------------------------------- 3. autocovariance
def _sample_lags(n, rng):
    if n <= 600:
        return np.arange(n)
    fixed = [0, 1, 2, 3, 254, 255, 256, 257, 511, 512, 513, n // 2, n - 257, n - 256, n - 255, n - 3, n - 2, n - 1]
    return np.unique(np.concatenate([fixed, rng.integers(0, n, 24)]))


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4096, 8192, 8193, 19200])
def test_autocovariance_bitwise(ctx, n):
    """bitwise the reference's double loop given the same mean, several rows per call; past 8192 samples the trace
    needs more than 64 KB of LDS"""
    rng = np.random.default_rng(n)
    nd = 64 if n <= 8192 else 16
    x = rng.standard_normal((nd, n)) * rng.uniform(0.1, 10.0, (nd, 1)) + rng.uniform(-3.0, 3.0, (nd, 1))
    out = ctx.autocovariance_batch(x)
    mean = np.array([row.mean() for row in x])              # covariance.py:730 data.mean(), row by row
    lags = _sample_lags(n, rng)
    ref = ref_autocov_lags(x, mean, lags)
    assert np.array_equal(out[:, lags], ref), "n=%d: %d of %d values differ" % (n, (out[:, lags] != ref).sum(),
                                                                                 ref.size)


def test_autocovariance_refuses_longer_traces(ctx):
    x = np.random.default_rng(1).standard_normal((2, 19201))
    with pytest.raises(ValueError):
        ctx.autocovariance_batch(x)
    y = x[:, :300].copy()
    ref = ref_autocov_lags(y, y.mean(axis=1), range(300))
    assert np.array_equal(ctx.autocovariance_batch(y), ref)


@pytest.mark.parametrize("n", [120, 4096])
def test_autocovariance_host_and_device_input_agree(ctx, n):
    """the update passes device tensors: their mean must be the host path's (numpy's) to the bit"""
    import torch
    rng = np.random.default_rng(3 * n)
    x = rng.standard_normal((64, n)) * rng.uniform(0.1, 10.0, (64, 1)) + rng.uniform(-3.0, 3.0, (64, 1))
    host = ctx.autocovariance_batch(x)
    dev = ctx.autocovariance_batch(torch.from_numpy(x).to("cuda:0")).cpu().numpy()
    assert np.array_equal(dev, host), "n=%d: %d of %d values differ, max rel %.3e" % (
        n, (dev != host).sum(), host.size, (np.abs(dev - host) / np.abs(host).max()).max())


# ----------------------------------------------------------------------------- 4. scaled Toeplitz
@pytest.mark.parametrize("nd,n", [(5, 1), (64, 120), (2, 1025), (3, 4096)])
def test_scaled_toeplitz_bitwise(ctx, nd, n):
    """toeplitz(coeffs[d]) * stds[d][:, None] * stds[d][None, :], multiplied in that order; 3 x 4096^2 is past the
    kernel's grid-stride limit of 65536 x 256 elements"""
    import torch
    from scipy.linalg import toeplitz
    rng = np.random.default_rng(nd * n)
    coeffs = rng.standard_normal((nd, n))
    stds = rng.uniform(0.1, 3.0, (nd, n))
    out = ctx.scaled_toeplitz_batch(coeffs, stds)
    for d in range(nd):
        ref = toeplitz(coeffs[d]) * stds[d][:, np.newaxis] * stds[d][np.newaxis, :]
        assert np.array_equal(out[d], ref), "nd=%d n=%d dataset %d" % (nd, n, d)
    if nd * n * n <= 1 << 24:
        dev = ctx.scaled_toeplitz_batch(torch.from_numpy(coeffs).to("cuda:0"), torch.from_numpy(stds).to("cuda:0"))
        assert np.array_equal(dev.cpu().numpy(), out)


# ----------------------------------------------------------------------------- 5. whitening ratio, unwhitening
@pytest.mark.parametrize("n", [513, 1025, 4096])
def test_whitening_ratio_at_update_sizes(ctx, n):
    """M = W_new . inv(W_old) of two whitening operators; kappa(W) = sqrt(kappa(C)) since W^T W = inv(C)"""
    rng = np.random.default_rng(n + 5)
    Co = [exp_toeplitz(n, np.exp(-1.0 / 5.0)), non_toeplitz(n, rng)]
    Cn = [exp_toeplitz(n, np.exp(-1.0 / 3.0)), non_toeplitz(n, rng)]
    Wo = np.stack([ref_whitening(C)[0] for C, _ in Co])
    Wn = np.stack([ref_whitening(C)[0] for C, _ in Cn])
    M = ctx.whitening_ratio_batch(Wn, Wo)
    for i in range(2):
        kw = np.sqrt(Co[i][1])
        assert np.array_equal(np.tril(M[i], -1), np.zeros((n, n)))
        ref = Wn[i] @ np.linalg.inv(Wo[i])
        # forward error of a triangular solve: c n u kappa(W_old)
        tol = C_RND * n * U * kw * np.abs(ref).max()
        err = np.abs(M[i] - ref).max()
        assert err <= tol, "n=%d op %d: |M - M_ref| = %.3e > %.3e" % (n, i, err, tol)
        # a substitution has a componentwise residual of c n u (|M| |W_old|) (host product included); the diagonal
        # blocks are applied as explicit inverses, which costs at most another kappa(W_old).  The exponential
        # operators are bidiagonal, so M decays geometrically into subnormals at n = 4096: each of the n products
        # there may lose up to the smallest normal number, c n tiny.
        r = np.abs(M[i] @ Wo[i] - Wn[i])
        bnd = C_RND * n * (U * kw * (np.abs(M[i]) @ np.abs(Wo[i])) + np.finfo(np.float64).tiny)
        assert (r <= bnd).all(), "n=%d op %d: residual above c n u kappa |M||W_old| at %d entries" % (
            n, i, (r > bnd).sum())


def test_unwhiten_traces_with_bench_length_operators(ctx, bench_length):
    """x <- inv(W) x with the n = 4096 operators of the Cholesky test"""
    Cs, kap, W, lp, refs = bench_length
    n = W.shape[1]
    rng = np.random.default_rng(11)
    x0 = rng.standard_normal((len(W), n))
    x = x0.copy()
    ctx.unwhiten_traces(W, x)
    for i in range(len(W)):
        ref = np.linalg.solve(W[i], x0[i])
        tol = C_RND * n * U * np.sqrt(kap[i]) * np.abs(ref).max()   # triangular solve: c n u kappa(W)
        err = np.abs(x[i] - ref).max()
        assert err <= tol, "op %d: |x - x_ref| = %.3e > %.3e" % (i, err, tol)
        # back substitution: componentwise residual c n u |W| |x| (host product included)
        r = np.abs(W[i] @ x[i] - x0[i])
        assert (r <= C_RND * n * U * (np.abs(W[i]) @ np.abs(x[i]))).all()


# ----------------------------------------------------------------------------- 6. one update at N = 4096
def test_noise_covariance_update_at_bench_trace_length(ctx):
    """NoiseCovarianceUpdate.update_weights on a 4-target, 4096-sample model against the reference's numpy route
    (covariance.py:739-771, then heart.py:216-253) from the same residuals"""
    from beat_amd.covariance import NoiseCovarianceUpdate
    from beat_amd.synthetic import SyntheticSpec, build_problem, draw_population
    spec = SyntheticSpec((6,), (5,), (1.0,), T=4, N=4096, D=3, S=25, covariance="toeplitz")
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], 16)
    q_map = Q[int(np.argmax(np.asarray(f.batch(Q))[:, -1]))]
    upd = NoiseCovarianceUpdate(f)
    _, res = upd.data_covariances(q_map, 0)
    r = res.cpu().numpy()
    T, N = r.shape
    upd.update_weights(q_map)
    wm = f.problem.wavemaps[0]
    W = wm.weights.cpu().numpy() if hasattr(wm.weights, "cpu") else np.asarray(wm.weights)
    sl = np.asarray(wm.slog_pdet)
    print("n_repaired = %d of %d targets, update %.1f ms" % (upd.n_repaired, T, upd.last_ms))
    repaired = 0
    for t in range(T):
        C = ref_non_toeplitz(r[t], N // 5)
        try:
            np.linalg.cholesky(C)
        except np.linalg.LinAlgError:                  # utility.repair_covariance
            ev, evec = np.linalg.eigh(C)
            C = evec.dot(np.diag(np.maximum(ev, np.finfo(np.float64).eps))).dot(evec.T)
            repaired += 1
        ev = np.linalg.eigvalsh(C)
        # (the device's stds come from running sums, a relative difference of a few u: inside c n u kappa)
        check_whitening(W[t], sl[t], C, ev[-1] / ev[0], what="target %d" % t)
    assert upd.n_repaired == repaired
