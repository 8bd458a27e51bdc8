"""
numpy restatement of csrc/seislib.hip, operation by operation (test infrastructure; float64 throughout, numpy does not
contract a * b + c).  The reference lines it follows:

  beat/ffi/base.py:1005-1064   _process_patch_seismic: per patch, per target, per starttime -> gfs.put
  beat/heart.py:3466-3525      post_process_trace: filters, extend(zeros), taper, chop(snap=(floor, floor))
  beat/heart.py:366-412        Filter / BandstopFilter
  beat/heart.py:295-304        ArrivalTaper.nsamples
  pyrocko HalfSinusoidSTF.discretize_t, Trace.extend / taper / chop: as recalled, UNVERIFIED against pyrocko

Everything elementwise is vectorised over the traces (the same bits as a loop over them); everything with an order -- the
convolution's sum over the source-time function, the demean's sum, the filter recurrence -- runs sample by sample in the
order the kernels state.  ``cos`` is numpy's: the device's differs by a few ulp in the source-time function's amplitudes,
so the functions below take the amplitude table as an argument (``stf_table`` makes numpy's).
"""
import numpy as np

import momentrate_ref as mr

EPS = float(np.finfo(np.float64).eps)


def stf_table(durations, deltat):
    """-> (nt int32 [D], A [D, ntmax]): the half-sinusoid of momentrate_ref (t0 = 0, t1 = duration) per duration"""
    rows = [mr.half_sinusoid(0.0, float(d), deltat)[1] for d in durations]
    nt = np.array([r.size for r in rows], dtype=np.int32)
    A = np.zeros((len(rows), int(nt.max())))
    for d, r in enumerate(rows):
        A[d, :r.size] = r
    return nt, A


def stf_bound(A, nt):
    """element-wise bound on |A_device - A_numpy|: each cosine within 1 ulp of a value <= 1 in either implementation
    (2 EPS between them), a difference of two (4 EPS), the normalising sum S = 2 off by at most nt * 4 EPS plus its own
    rounding, and the division: (4 + 4 nt a) EPS, doubled for the roundings of the operations themselves"""
    return 2.0 * (4.0 + 4.0 * nt[:, None] * np.abs(A)) * EPS


def convolve(g, a):
    """g [R, L], a [nt] -> [R, L + nt - 1]: yc[n] = sum_i a_i g[n - i], i ascending from 0.0"""
    R, L = g.shape
    yc = np.zeros((R, L + a.size - 1))
    for i in range(a.size):
        yc[:, i:i + L] = yc[:, i:i + L] + a[i] * g
    return yc


def sum_in_order(x):
    """x [R, n] -> [R]: one sample after the other from 0.0 (numpy's own sum is pairwise)"""
    s = np.zeros(x.shape[0])
    for n in range(x.shape[1]):
        s = s + x[:, n]
    return s


def lfilter(b, a, x):
    """direct form II transposed with zero initial state over the rows of x [R, n]:
         y = z[0] + b[0] x;  z[k] = (z[k+1] + x b[k+1]) - y a[k+1], k = 0 .. m - 2;  z[m-1] = x b[m] - y a[m]"""
    m = len(b) - 1
    z = [np.zeros(x.shape[0]) for _ in range(m)]
    out = np.empty_like(x)
    for n in range(x.shape[1]):
        xn = x[:, n]
        y = z[0] + b[0] * xn
        for k in range(m - 1):
            z[k] = (z[k + 1] + xn * b[k + 1]) - y * a[k + 1]
        z[m - 1] = xn * b[m] - y * a[m]
        out[:, n] = y
    return out


def tap_count_filters(lower=0.05, upper=0.4):
    """(ntaps, order, wn, btype) of single Butterworth sections covering every tap count 3 ... 17 of the device cascade: the
    band-pass of order 1 ... 8 (3, 5, ..., 17 taps), the low-pass at ``upper`` and the high-pass at ``lower`` of odd order
    3 ... 15 (4, 6, ..., 16 taps); wn in units of the Nyquist frequency (0.1 and 0.8 Hz at deltat = 0.25 s)"""
    cases = [(2 * order + 1, order, [lower, upper], "band") for order in range(1, 9)]
    for order in range(3, 16, 2):
        cases += [(order + 1, order, upper, "low"), (order + 1, order, lower, "high")]
    return cases


def cascade(x, stages):
    """the stages (b, a, demean) one after the other over the rows of x [R, n]"""
    for b, a, demean in stages:
        if demean:
            x = x - (sum_in_order(x) / float(x.shape[1]))[:, None]
        x = lfilter(np.asarray(b, dtype=np.float64), np.asarray(a, dtype=np.float64), x)
    return x


def filtered_traces(traces, nt, A, stages):
    """traces [R, L] -> a list over the durations of [R, L + nt[d] - 1]"""
    return [cascade(convolve(traces, A[d, :nt[d]]), stages) for d in range(len(nt))]


def window_tables(tmins, arrival_times, starttimes, deltat, taper):
    """tmins [T, P], arrival_times [T], starttimes [S], taper = (a, b, c, d) -> i0 int64 [T, P, S], w0 [T, P, S]"""
    T, P = tmins.shape
    S = len(starttimes)
    i0, w0 = np.zeros((T, P, S), dtype=np.int64), np.ones((T, P, S))
    for t in range(T):
        for s in range(S):
            shifted = arrival_times[t] - starttimes[s]              # base.py:1047
            lower, fade_start = shifted + taper[1], shifted + taper[0]
            for p in range(P):
                k = np.floor((lower - tmins[t, p]) / deltat)        # chop, snap=(floor, floor)
                t0 = tmins[t, p] + k * deltat
                i0[t, p, s] = int(k)
                if t0 < lower:                                      # CosTaper's fade-in
                    w0[t, p, s] = 0.0 if t0 <= fade_start else \
                        0.5 * (1.0 - np.cos(np.pi * (t0 - fade_start) / (lower - fade_start)))
    return i0, w0


def nsamples(taper, deltat):
    """ArrivalTaper.nsamples (heart.py:295-304) of the [b, c] cut"""
    return int(np.ceil((1.0 / deltat) * (taper[2] - taper[1])))


def cut(y, i0, w0, N):
    """one window of the row y: N samples from i0, zeros outside the row (extend(fillmethod="zeros")), sample 0 times w0"""
    row = np.zeros(N)
    lo, hi = max(i0, 0), min(i0 + N, y.size)
    if hi > lo:
        row[lo - i0:hi - i0] = y[lo:hi]
    row[0] = row[0] * w0
    return row


def taper_filter_traces(traces, tmins, deltat, taper, stages, arrival_times):
    """heart.taper_filter_traces(outmode="array") for traces [R, L] -> [R, N]"""
    N = nsamples(taper, deltat)
    y = cascade(np.array(traces, dtype=np.float64), stages)
    i0, w0 = window_tables(np.asarray(tmins, dtype=np.float64)[:, None], arrival_times, np.zeros(1), deltat, taper)
    return np.stack([cut(y[r], int(i0[r, 0, 0]), w0[r, 0, 0], N) for r in range(y.shape[0])])


def build_library(gfs, responses, tmins, deltat, arrival_times, durations, starttimes, taper, stages, nt, A):
    """_process_patch_seismic's control flow (base.py:1005-1064) for every patch, filling the host library ``gfs`` (set up
    and allocated) through ``put`` and ``set_patch_time``; (nt, A): the source-time functions of the durations"""
    T, P, L = responses.shape
    N = nsamples(taper, deltat)
    i0, w0 = window_tables(tmins, arrival_times, starttimes, deltat, taper)
    filtered = filtered_traces(responses.reshape(T * P, L), nt, A, stages)      # (the same bits as trace by trace)
    for patchidx in range(P):
        for j in range(T):
            gfs.set_patch_time(targetidx=j, tmin=arrival_times[j])
            for s, starttime in enumerate(starttimes):
                entries = np.stack([cut(filtered[d][j * P + patchidx], int(i0[j, patchidx, s]), w0[j, patchidx, s], N)
                                    for d in range(len(durations))])
                gfs.put(entries=entries, targetidx=j, patchidx=patchidx, durations=durations, starttimes=starttime)
    return gfs
