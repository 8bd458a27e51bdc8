"""
The Python binding of the convergence entries of ``libbeat_amd.so`` (``beatamd_autocov_lags_batch``,
``beatamd_rank_normalize``, ``beatamd_convergence_summary``; csrc/convergence.hip) as functions of a ``Context`` (``ctx``,
beat_amd.engine).  The argument rules that need no device are checked here ahead of the call (the library checks them
again); results live on the side of the first array argument.  ``beat_amd.diagnostics`` is the public interface on top.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr
from ._marshal import as_input, checked
from .marginals_binding import SORT_MAX_N, check_columns

NCOL = 11                                              # csrc/kernels.hpp CV_NCOL
COLUMNS = ("mean", "sd", "hdi_lo", "hdi_hi", "mcse_mean", "mcse_sd", "ess_bulk", "ess_tail", "r_hat", "ess_mean", "ess_sd")
ACOV_TILE, ACOV_CHUNK = 512, 4096                      # csrc/kernels.hpp CV_ACOV_TILE, CV_ACOV_CHUNK


def check_rows(Y, what="Y"):
    """Y as the library reads it: a contiguous float64 (R, n) array, n >= 1 -> (Y, R, n)"""
    Y = as_input(Y)
    if len(Y.shape) != 2 or Y.shape[1] < 1:
        raise ValueError("%s must be a (rows, n) array with n >= 1, got %s" % (what, tuple(Y.shape)))
    return Y, int(Y.shape[0]), int(Y.shape[1])


def check_trace(X):
    """X as the library reads it: a contiguous float64 (C, D, V) array, all >= 1, C D <= 2^24 -> (X, C, D, V)"""
    X = as_input(X)
    if len(X.shape) != 3 or min(X.shape) < 1:
        raise ValueError("X must be a (chains, draws, variables) array, each >= 1, got %s" % (tuple(X.shape),))
    Cn, D, V = (int(s) for s in X.shape)
    if Cn * D > SORT_MAX_N:
        raise ValueError("convergence_summary: %d x %d samples a variable, at most 2^24" % (Cn, D))
    return X, Cn, D, V


def check_hdi_prob(hdi_prob):
    p = float(hdi_prob)
    if not 0.0 < p < 1.0:
        raise ValueError("hdi_prob must lie in (0, 1), got %r" % (hdi_prob,))
    return p


def check_lags(lag0, nlags):
    lag0, nlags = int(lag0), int(nlags)
    if lag0 < 0 or nlags < 0:
        raise ValueError("autocov: lag0 = %d and nlags = %d must not be negative" % (lag0, nlags))
    return lag0, nlags


def check_schedule(var_batch, first_lags):
    var_batch = 0 if var_batch is None else int(var_batch)
    first_lags = int(first_lags)
    if var_batch < 0 or first_lags < 2:
        raise ValueError("convergence_summary: var_batch = %d must not be negative and first_lags = %d must be at least 2"
                         % (var_batch, first_lags))
    return var_batch, first_lags


def tau_floor(Cn, D):
    """1 / log10(M n) of the split row sets (M = 2 C rows of n = D // 2 values), numpy's; 0 where there are no diagnostics"""
    return float(1.0 / np.log10(np.float64(2 * Cn * (D // 2)))) if D >= 4 else 0.0


def autocov_lags_batch(ctx, Y, nlags, lag0=0, out=None):
    """Y (R, n) -> (R, nlags): the biased autocovariance of every row at the lags lag0 .. lag0 + nlags (0 at lags >= n)"""
    ctx._adopt_stream(Y)
    Y, R, n = check_rows(Y)
    lag0, nlags = check_lags(lag0, nlags)
    out = checked(out, Y, (R, nlags), np.float64, "out", of="Y")
    check(ctx._lib.beatamd_autocov_lags_batch(ctx._h, R, n, ptr(Y), lag0, nlags, ptr(out)))
    return out


def rank_normalize(ctx, A, want_ranks=False):
    """A (any shape, at least one value) -> z of that shape, or (z, average ranks); ValueError for a non-finite value"""
    ctx._adopt_stream(A)
    A = as_input(A)
    n = int(np.prod(tuple(A.shape)))
    if n < 1:
        raise ValueError("rank_normalize: no values")
    if n > SORT_MAX_N:
        raise ValueError("rank_normalize: %d values, at most 2^24" % n)
    z = checked(None, A, tuple(A.shape), np.float64, "z", of="A")
    r = checked(None, A, tuple(A.shape), np.float64, "ranks", of="A") if want_ranks else None
    rc = ctx._lib.beatamd_rank_normalize(ctx._h, n, ptr(A), ptr(z), ptr(r))
    if rc == _lib.ENAN:
        raise ValueError("rank_normalize: the array holds a non-finite value")
    check(rc)
    return (z, r) if want_ranks else z


def convergence_summary(ctx, X, cols=None, hdi_prob=0.94, var_batch=None, first_lags=64):
    """X (C, D, V), cols (K,) -> (table (K, 11) in the order of ``COLUMNS`` with the two mcse columns NaN, flags int32 (K,),
    rounds): on X's side but for ``rounds``, the largest number of on-demand lag rounds of a pass.  ``var_batch`` (None:
    sized to the workspace budget) and ``first_lags`` are the schedule; no bit of the table depends on them."""
    ctx._adopt_stream(X)
    X, Cn, D, V = check_trace(X)
    c = check_columns(cols, V)
    p = check_hdi_prob(hdi_prob)
    var_batch, first_lags = check_schedule(var_batch, first_lags)
    out = checked(None, X, (c.size, NCOL), np.float64, "out", of="X")
    flags = checked(None, X, (c.size,), np.int32, "flags", of="X", zero=True)
    rounds = C.c_int64(0)
    check(ctx._lib.beatamd_convergence_summary(ctx._h, Cn, D, V, ptr(X), int(c.size), ptr(c), p, tau_floor(Cn, D), var_batch, first_lags, ptr(out),
                                               ptr(flags), C.byref(rounds)))
    return out, flags, int(rounds.value)
