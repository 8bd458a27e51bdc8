"""numpy restatement of the posterior diagnostics (beat_amd/csrc/summary.hip and the C entries around it), pinned to the
reference's numbers by tests/test_summary_host.py (tests/golden/summary.npz) and used as the expectation of
tests/test_gpu_summary.py.  TEST INFRASTRUCTURE ONLY."""
import numpy as np


def quad(W, x):
    """|W x|^2 for a whitening operator (scalar: W = w I)"""
    wx = W * x if np.ndim(W) == 0 else np.asarray(W) @ x
    return float(wx @ wx)


def variance_reduction(W, r, d):
    """-> (nom, denom, 1 - nom / denom) as the engine forms them: quadratic forms through W with W^T W = inv(C)"""
    nom, denom = quad(W, r), quad(W, d)
    return nom, denom, 1.0 - nom / denom


def standardize(S, r, hp=None):
    """exp(-hp) * (S . r): S scalar or (N, N); the operation order of k_standardize"""
    z = S * r if np.ndim(S) == 0 else np.asarray(S) @ r
    return z if hp is None else np.exp(-hp) * z


def standardize_batch(S, R, hp=None):
    """S (T,) or (T, N, N), R (C, T, N), hp (C, T) or None -> (C, T, N)"""
    S, R = np.asarray(S), np.asarray(R)
    z = S[None, :, None] * R if S.ndim == 1 else np.einsum("tnk,ctk->ctn", S, R)
    return z if hp is None else np.exp(-np.asarray(hp))[:, :, None] * z


def welford_update(X, state=None, n_seen=0):
    """the rows of X (C, M) folded into state (5, M) = (mean, M2, min, max, rows seen) in row order with exactly
    d = x - m; m = m + d / n; M2 = M2 + d * (x - m)   -> (state, n_seen + C)"""
    X = np.asarray(X, dtype=np.float64)
    C, M = X.shape
    if n_seen == 0:
        state = np.zeros((5, M))
        state[2], state[3] = np.inf, -np.inf
    else:
        state = np.array(state, dtype=np.float64)
    m, s, lo, hi = state[0].copy(), state[1].copy(), state[2].copy(), state[3].copy()
    for i in range(C):
        x = X[i]
        n = float(n_seen + i + 1)
        d = x - m
        m = m + d / n
        s = s + d * (x - m)
        lo = np.where(x < lo, x, lo)
        hi = np.where(x > hi, x, hi)
    state[0], state[1], state[2], state[3], state[4] = m, s, lo, hi, float(n_seen + C)
    return state, n_seen + C


def welford_finish(state, n):
    """-> mean, std (ddof = 0), min, max"""
    return state[0].copy(), np.sqrt(state[1] / float(n)), state[2].copy(), state[3].copy()


def two_pass(X):
    """mean and std (ddof = 0) of the columns in extended precision, rounded to float64 at the end"""
    X = np.asarray(X, dtype=np.longdouble)
    mean = X.sum(0) / X.shape[0]
    var = ((X - mean) ** 2).sum(0) / X.shape[0]
    return mean.astype(np.float64), np.sqrt(var).astype(np.float64)


def moments_bound(X):
    """C * 2^-52 * max|x| per column: the bound on the recurrence's distance from the two-pass result"""
    X = np.asarray(X)
    return X.shape[0] * 2.0 ** -52 * np.abs(X).max(0)


def fixture_cases(g):
    """(key prefix, n) of every covariance case of tests/golden/summary.npz"""
    return [("%s_%d" % (k, n), int(n)) for k in g["kinds"] for n in g["sizes"]]


def fixture_covariance(g, key):
    """the product's Covariance object over the fixture's terms"""
    from beat_amd.heart import Covariance
    pred_v = g[key + "_pred_v"] if key + "_pred_v" in g.files else None
    return Covariance(data=g[key + "_data"], pred_v=pred_v)
