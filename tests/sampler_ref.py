"""Plain references of the sampler-step kernels (csrc/smc.hip, csrc/metropolis.hpp, k_like_assemble of csrc/logp.hip),
written from the algorithms in loop form -- not built on beat_amd.sampler.ops.HostOps, which is a second implementation
under test.  Sources: beat/sampler/smc.py:133-186, 290-324 (tempering step, weighted covariance, Kitagawa resampling),
beat/sampler/metropolis.py:313-385 with pymc's metrop_select (propose, prior box, accept), beat/models/problems.py:227-247
(`like` = the composites' sums).

Where the operation decides something (a bisection branch, a chain accepted, a parent chosen) the reference decides in
float64 exactly as numpy / Python floats do; where it returns real numbers they are np.longdouble, the more precise side
of every comparison."""
import math

import numpy as np

LD = np.longdouble


# ----------------------------------------------------------------------------- SMC stage transition
def _weights_ld(lk, step):
    """exp(step (l - max l)) / their sum, the argument rounded as float64 forms it, exp / sum / quotient in long double.
    A NaN likelihood makes every weight NaN (np.max propagates it)."""
    lk = np.asarray(lk, dtype=np.float64)
    with np.errstate(all="ignore"):
        arg = np.float64(step) * (lk - np.max(lk))
        t = np.exp(arg.astype(LD))
        total = LD(0.0)
        for v in t:
            total = total + v
        return t / total


def calc_beta_ref(lk, beta, cv, path=None):
    """smc.py:133-165 -> (beta_new, weights longdouble, margin longdouble): the interval [beta, 2] is halved until it is
    no wider than 1e-6; the midpoint moves down when std / mean of exp((mid - beta)(l - max l)) exceeds cv, as numpy's
    float64 np.std / np.mean see it.  weights: those of the last midpoint, in long double.  margin: the smallest
    |cov_temp - cv| of all midpoints, cov_temp evaluated in long double (NaN if one was NaN); path, a list, receives
    (midpoint, |cov_temp - cv|) of every halving."""
    lk = np.asarray(lk, dtype=np.float64)
    beta = float(beta)
    if not 2.0 - beta > 1e-6:
        raise ValueError("calc_beta_ref: the reference's loop does not run for beta = %r" % beta)
    lo, hi = beta, 2.0
    margin = LD(np.inf)
    with np.errstate(all="ignore"):
        shifted = lk - np.max(lk)
        while hi - lo > 1e-6:
            mid = (lo + hi) / 2.0
            arg = (mid - beta) * shifted
            temp = np.exp(arg)
            cov_temp = np.std(temp) / np.mean(temp)
            if cov_temp > cv:
                hi = mid
            else:
                lo = mid
            t = np.exp(arg.astype(LD))
            n = LD(t.size)
            mean = t.sum() / n
            d = t - mean
            cov_ld = np.sqrt((d * d).sum() / n) / mean
            gap = abs(cov_ld - LD(cv))
            if path is not None:
                path.append((mid, gap))
            if not (gap >= margin):    # smaller, or NaN: a NaN stays
                margin = gap
    return mid, _weights_ld(lk, mid - beta), margin


def stage_weights_ref(lk, dbeta):
    """smc.py:526-529: the final stage's weights for the exponent step dbeta, long double"""
    return _weights_ld(lk, float(dbeta))


def resample_ref(w, aux):
    """smc.py:290-324: child i sits at u_i = (i + aux) / n and belongs to the first parent j whose cumulative weight
    reaches it; j only moves forward.  The cumulative sum is sequential float64.  j stops at n - 1: the reference would
    index past its array when rounding leaves cum[n-1] below the last u."""
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    cum, c = [], 0.0
    for v in w.tolist():
        c = c + v
        cum.append(c)
    out, j = [], 0
    for i in range(n):
        u = (float(i) + float(aux)) / float(n)
        while j < n - 1 and u > cum[j]:
            j += 1
        out.append(j)
    return np.array(out, dtype=np.int64)


def resample_u_cum(w, aux):
    """the float64 u and cum of resample_ref, for the checks on the inputs"""
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    u = np.array([(float(i) + float(aux)) / float(n) for i in range(n)])
    cum, c = np.empty(n), 0.0
    for i, v in enumerate(w.tolist()):
        c = c + v
        cum[i] = c
    return u, cum


def population_factor_ref(X, w):
    """-> (F, cov, parts): F[i, j] = sqrt(w_i / (v1 - v2 / v1)) (x_ij - mean_j) in long double, v1 = sum w, v2 = sum w^2,
    mean_j = sum_i w_i x_ij / v1; cov = np.cov(X, aweights=w, bias=False, rowvar=0) on long double input (smc.py:167-186);
    parts = (fact, absmean, v1) with fact = 1 / (v1 - v2 / v1) and absmean_j = sum_k w_k |x_kj| / v1, the terms of the
    kernels' error bound."""
    X = np.asarray(X, dtype=np.float64).astype(LD)
    w = np.asarray(w, dtype=np.float64).astype(LD)
    n, npar = X.shape
    v1 = LD(0.0)
    v2 = LD(0.0)
    for i in range(n):
        v1 = v1 + w[i]
        v2 = v2 + w[i] * w[i]
    mean = np.zeros(npar, dtype=LD)
    absmean = np.zeros(npar, dtype=LD)
    for i in range(n):
        mean = mean + w[i] * X[i]
        absmean = absmean + w[i] * np.abs(X[i])
    mean = mean / v1
    absmean = absmean / v1
    fact = LD(1.0) / (v1 - v2 / v1)
    F = np.empty((n, npar), dtype=LD)
    for i in range(n):
        F[i] = np.sqrt(w[i] * fact) * (X[i] - mean)
    cov = np.atleast_2d(np.cov(X, aweights=w, bias=False, rowvar=0))
    return F, cov, (fact, absmean, v1)


def population_factor_bound(X, w, n_terms=None):
    """per entry: 4 (n + 8) 2^-53 sqrt(w_i fact) (sum_k w_k |x_kj| / v1 + |x_ij|), the error of an n-term float64 sum in
    any order with a factor 4 for the other operations; long double"""
    F, cov, (fact, absmean, v1) = population_factor_ref(X, w)
    Xl = np.asarray(X, dtype=np.float64).astype(LD)
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    n = Xl.shape[0] if n_terms is None else n_terms
    return LD(4.0 * (n + 8)) * LD(2.0) ** -53 * np.sqrt(wl * fact)[:, None] * (absmean[None, :] + np.abs(Xl))


# ----------------------------------------------------------------------------- Metropolis step
def propose_ref(Q0, delta, scaling, lo, up):
    """metropolis.py:313-343 -> (Qprop, inbounds): q = q0 + delta * scaling, the product rounded to float64, then the sum;
    a chain is inside iff lo <= q <= up holds for every component (false of a NaN); an outside chain keeps q0."""
    Q0 = np.asarray(Q0, dtype=np.float64)
    delta = np.asarray(delta, dtype=np.float64)
    C, npar = Q0.shape
    Qp = np.empty_like(Q0)
    inb = np.zeros(C, dtype=np.int32)
    with np.errstate(all="ignore"):
        for c in range(C):
            inside = True
            row = np.empty(npar)
            for k in range(npar):
                d = np.float64(delta[c, k]) * np.float64(scaling[c])
                q = np.float64(Q0[c, k]) + d
                row[k] = q
                if not (lo[k] <= q and q <= up[k]):
                    inside = False
            inb[c] = 1 if inside else 0
            Qp[c] = row if inside else Q0[c]
    return Qp, inb


def accept_ref(Q0, L0, Qprop, Lprop, inbounds, log_u, beta):
    """metropolis.py:344-385 + pymc's metrop_select -> (Q0', L0', accepted): a chain outside the box is rejected without
    a look at its likelihoods; else mr = beta (lp - l0), `like` being the last column, and the proposal is taken iff mr
    is finite and log u < mr: the whole rows of Qprop and Lprop replace the chain's.  beta: a float or one per chain."""
    Q1 = np.array(Q0, dtype=np.float64, copy=True)
    L1 = np.array(L0, dtype=np.float64, copy=True)
    C = Q1.shape[0]
    acc = np.zeros(C, dtype=np.int32)
    for c in range(C):
        if not int(inbounds[c]):
            continue
        b = float(beta[c]) if np.ndim(beta) else float(beta)
        lp, l0 = float(Lprop[c, -1]), float(L0[c, -1])
        mr = b * (lp - l0)
        if math.isfinite(mr) and float(log_u[c]) < mr:
            Q1[c] = Qprop[c]
            L1[c] = Lprop[c]
            acc[c] = 1
    return Q1, L1, acc


def like_assemble_ref(gathered, dst_col, local, col0, n_rest, rest_dst0, group_end, nllk):
    """problems.py:227-247 over the gathered rows of a target-sharded model -> LL [C, nllk]: row r of gathered [nsrc, C]
    goes to column dst_col[r]; a row with dst_col -1 is a rank's flag row, a NaN there marks the chain bad; columns
    rest_dst0 .. take local[:, col0 : col0 + n_rest]; like (the last column) adds each composite's entries in ascending
    order from 0.0 and then the composites' sums in order, in Python floats; a bad chain's like is NaN."""
    gathered = np.asarray(gathered, dtype=np.float64)
    C = gathered.shape[1]
    LL = np.zeros((C, nllk))
    for c in range(C):
        bad = False
        for r, d in enumerate(dst_col):
            v = gathered[r, c]
            if d >= 0:
                LL[c, d] = v
            elif v != v:
                bad = True
        for k in range(n_rest):
            LL[c, rest_dst0 + k] = local[c, col0 + k]
        total, k = 0.0, 0
        for end in group_end:
            s = 0.0
            while k < end:
                s = s + float(LL[c, k])
                k += 1
            total = total + s
        LL[c, nllk - 1] = float("nan") if bad else total
    return LL
