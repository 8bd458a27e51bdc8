"""
The Python binding of the library-producer entries of ``libbeat_amd.so`` (``beatamd_stf_table``,
``beatamd_trace_filter_batch``, ``beatamd_seis_library_fill``; csrc/seislib.hip) as functions of a ``Context`` (``ctx``,
beat_amd.engine).  The argument rules that need no device are checked here ahead of the call (the library checks them
again); results live on the side of the first array argument.  ``beat_amd.seislib`` is the public interface on top.
"""
import numpy as np

from ._lib import check, ptr
from ._marshal import as_input, checked, is_dev, on_side

MAX_STAGES, MIN_TAPS, MAX_TAPS = 4, 3, 17      # csrc/kernels.hpp SL_MAX_STAGES, SL_MIN_TAPS, SL_MAX_TAPS
NT_MAX = 65536                                 # csrc/kernels.hpp SL_NT_MAX
GRID_MAX = 32767                               # the library's grid indices are int16 (ffi._time2idx)


def _host(a):
    return a.cpu().numpy() if is_dev(a) else np.asarray(a)


def _finite(a, what):
    """ValueError for a non-finite entry of a host array or a tensor of either side"""
    ok = bool(a.isfinite().all()) if hasattr(a, "data_ptr") and not isinstance(a, np.ndarray) else bool(np.isfinite(a).all())
    if not ok:
        raise ValueError("%s must be finite" % what)


def check_deltat(deltat):
    deltat = float(deltat)
    if not (np.isfinite(deltat) and deltat > 0.0):
        raise ValueError("deltat must be a positive number, got %r" % (deltat,))
    return deltat


def check_grid(values, what):
    """a duration or starttime grid: a finite float64 vector of 1 ... 32767 entries (the library's int16 indices)"""
    v = np.ascontiguousarray(np.atleast_1d(_host(values)), dtype=np.float64)
    if v.ndim != 1 or v.size < 1:
        raise ValueError("%s must be a vector with at least one entry, got %s" % (what, v.shape))
    if v.size > GRID_MAX:
        raise ValueError("%d %s: the library indexes them with int16, at most %d" % (v.size, what, GRID_MAX))
    _finite(v, what)
    return v


def check_durations(durations, deltat):
    """the duration grid and the length of its longest source-time function, rint(duration / deltat) + 1"""
    d = check_grid(durations, "durations")
    if np.any(d < 0.0):
        raise ValueError("durations must not be negative")
    ntmax = int(np.rint(d / deltat).max()) + 1
    if ntmax > NT_MAX:
        raise ValueError("a duration of %g s has %d samples at deltat %g; at most %d" % (d.max(), ntmax, deltat, NT_MAX))
    return d, ntmax


def check_stages(stages):
    """stages: a sequence of (b, a, demean) -> (nstage, ntaps int32 [nstage], demean int32 [nstage], coef [nstage, 2, 17]);
    at most 4 stages of 3 ... 17 taps, len(b) == len(a), finite, a[0] == 1"""
    stages = list(stages or [])
    if len(stages) > MAX_STAGES:
        raise ValueError("%d filter stages; the device cascade takes at most %d" % (len(stages), MAX_STAGES))
    n = len(stages)
    ntaps, demean = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    coef = np.zeros((max(n, 1), 2, MAX_TAPS))
    for s, (b, a, dm) in enumerate(stages):
        b, a = np.asarray(b, dtype=np.float64).ravel(), np.asarray(a, dtype=np.float64).ravel()
        if b.size != a.size:
            raise ValueError("stage %d: b has %d taps, a has %d" % (s, b.size, a.size))
        if not MIN_TAPS <= b.size <= MAX_TAPS:
            raise ValueError("stage %d has %d taps (filter order %d); the device cascade takes %d ... %d taps"
                             % (s, b.size, b.size - 1, MIN_TAPS, MAX_TAPS))
        _finite(b, "stage %d: b" % s)
        _finite(a, "stage %d: a" % s)
        if a[0] != 1.0:
            raise ValueError("stage %d is not normalised: a[0] = %r, must be 1" % (s, a[0]))
        ntaps[s], demean[s] = b.size, int(bool(dm))
        coef[s, 0, :b.size], coef[s, 1, :a.size] = b, a
    return n, ntaps, demean, coef


def stf_table(ctx, durations, deltat, ntmax=None, like=None):
    """durations (D,) -> (nt int32 (D,), A (D, ntmax)) on the side of ``like`` (None: the host): the normalised half-sinusoid
    amplitudes of every duration, zero beyond nt = rint(duration / deltat) + 1"""
    deltat = check_deltat(deltat)
    d, need = check_durations(durations, deltat)
    ntmax = need if ntmax is None else int(ntmax)
    if ntmax < need:
        raise ValueError("the table holds %d samples, the longest duration has %d" % (ntmax, need))
    ref = like if like is not None else d
    ctx._adopt_stream(ref)
    d = on_side(d, ref, np.float64, (d.size,), "durations")
    nt = checked(None, ref, (int(d.shape[0]),), np.int32, "nt")
    A = checked(None, ref, (int(d.shape[0]), ntmax), np.float64, "A")
    check(ctx._lib.beatamd_stf_table(ctx._h, int(d.shape[0]), ptr(d), deltat, ntmax, ptr(nt), ptr(A)))
    return nt, A


def unit_stf(like):
    """the table of "no source-time function": D = 1, nt = [1], A = [[1]] on the side of ``like``"""
    nt = on_side(np.ones(1, dtype=np.int32), like, np.int32, (1,), "nt")
    A = on_side(np.ones((1, 1)), like, np.float64, (1, 1), "A")
    return nt, A


def check_traces(X, ndim, what):
    X = as_input(X)
    if len(X.shape) != ndim or min(X.shape) < 1:
        raise ValueError("%s must be a %d-d array without an empty axis, got %s" % (what, ndim, tuple(X.shape)))
    _finite(X, what)
    return X


def _table(nt, A, like):
    """the table of stf_table on the side of ``like`` -> (nt, A, D, ntmax, longest nt)"""
    h = np.asarray(_host(nt))
    if h.ndim != 1 or h.size < 1 or h.size > GRID_MAX:
        raise ValueError("nt must be a vector of 1 ... %d lengths, got %s" % (GRID_MAX, h.shape))
    D = int(h.size)
    if len(A.shape) != 2 or int(A.shape[0]) != D or not 1 <= int(A.shape[1]) <= NT_MAX:
        raise ValueError("A must be (%d, ntmax <= %d), got %s" % (D, NT_MAX, tuple(A.shape)))
    ntmax = int(A.shape[1])
    if h.min() < 1 or h.max() > ntmax:
        raise ValueError("nt must lie in [1, %d]" % ntmax)
    return on_side(nt, like, np.int32, (D,), "nt"), on_side(A, like, np.float64, (D, ntmax), "A"), D, ntmax, int(h.max())


def trace_filter_batch(ctx, traces, nt, A, stages):
    """traces (R, L), the table (nt (D,), A (D, ntmax)), stages [(b, a, demean)] -> Y (R, D, L + max(nt) - 1) on the side
    of ``traces``: every trace convolved with every row of A and run through the cascade (zeros behind a row's
    L + nt[d] - 1 samples)"""
    X = check_traces(traces, 2, "traces")
    R, L = int(X.shape[0]), int(X.shape[1])
    n, ntaps, demean, coef = check_stages(stages)
    nt, A, D, ntmax, ntm = _table(nt, A, X)
    ctx._adopt_stream(X)
    Y = checked(None, X, (R, D, L + ntm - 1), np.float64, "Y", of="traces")
    check(ctx._lib.beatamd_trace_filter_batch(ctx._h, R, L, ptr(X), D, ntmax, ptr(nt), ptr(A), n, ptr(ntaps), ptr(demean),
                                              ptr(coef), ptr(Y)))
    return Y


def seis_library_fill(ctx, responses, nt, A, stages, i0, w0, N, patch_block=None, out=None):
    """responses (T, P, L), the table (nt, A), stages, the window tables i0 int64 / w0 float64 (T, P, S), N samples a window
    -> lib (T, P, D, S, N) on the side of ``responses`` (``out``: written in place)"""
    X = check_traces(responses, 3, "responses")
    T, P, L = (int(v) for v in X.shape)
    n, ntaps, demean, coef = check_stages(stages)
    nt, A, D, ntmax, _ = _table(nt, A, X)
    i0h = np.asarray(_host(i0))
    if i0h.ndim != 3 or i0h.shape[:2] != (T, P) or i0h.shape[2] < 1:
        raise ValueError("i0 must be (%d, %d, S >= 1), got %s" % (T, P, i0h.shape))
    S, N = int(i0h.shape[2]), int(N)
    if S > GRID_MAX:
        raise ValueError("%d starttimes: the library indexes them with int16, at most %d" % (S, GRID_MAX))
    if N < 1:
        raise ValueError("a window of %d samples" % N)
    i0 = on_side(i0, X, np.int64, (T, P, S), "i0")
    w0 = on_side(w0, X, np.float64, (T, P, S), "w0")
    _finite(w0, "w0")
    pb = P if patch_block is None else int(patch_block)
    if pb < 1:
        raise ValueError("patch_block must be at least 1, got %d" % pb)
    ctx._adopt_stream(X)
    lib = checked(out, X, (T, P, D, S, N), np.float64, "out", of="responses")
    check(ctx._lib.beatamd_seis_library_fill(ctx._h, T, P, L, ptr(X), D, ntmax, ptr(nt), ptr(A), n, ptr(ntaps), ptr(demean),
                                             ptr(coef), S, N, ptr(i0), ptr(w0), pb, ptr(lib)))
    return lib
