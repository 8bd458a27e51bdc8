"""numpy restatement of the convergence summary (csrc/convergence.hip): the statistics of arviz.summary as
restated from memory of arviz's stats/diagnostics.py and of Vehtari et al. (2021) -- unverified against an installed arviz
--, with the sums in the kernels' fixed orders.  Two autocovariance routes: ``acov_fft`` (arviz's) and ``acov_fixed`` (the
kernel's: one accumulator a lag, chunks of ``CHUNK`` consecutive i added in ascending order)."""
import numpy as np

TB, CHUNK, TILE = 256, 4096, 512      # csrc/convergence.hip CV_TB, csrc/kernels.hpp CV_ACOV_CHUNK, CV_ACOV_TILE
COLUMNS = ("mean", "sd", "hdi_lo", "hdi_hi", "mcse_mean", "mcse_sd", "ess_bulk", "ess_tail", "r_hat", "ess_mean", "ess_sd")


# ------------------------------------------------------------------------------------------------ the SUMS order
def block_sum(Y):
    """the sum of every row of Y (R, n): thread t of 256 adds the elements t, t + 256, ... ascending, then the halving tree"""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    R, n = Y.shape
    nb = (n + TB - 1) // TB
    P = np.zeros((R, nb * TB))
    P[:, :n] = Y
    P = P.reshape(R, nb, TB)
    s = np.zeros((R, TB))
    for b in range(nb):
        s = s + P[:, b]
    h = TB // 2
    while h > 0:
        s = s[:, :h] + s[:, h:2 * h]
        h //= 2
    return s[:, 0]


def moments(Y):
    """(mean, centred sum of squares, min, max) of every row of Y (R, n), the kernel's two passes"""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    n = Y.shape[1]
    mean = block_sum(Y) / np.float64(n)
    d = Y - mean[:, None]
    return mean, block_sum(d * d), Y.min(axis=1), Y.max(axis=1)


def seq_sum(v):
    s = np.float64(0.0)
    for x in v:
        s = s + np.float64(x)
    return s


def seq_var1(v):
    """var(v, ddof=1) with sequential sums"""
    M = len(v)
    mm = seq_sum(v) / np.float64(M)
    q = np.float64(0.0)
    for x in v:
        d = np.float64(x) - mm
        q = q + d * d
    with np.errstate(all="ignore"):
        return q / np.float64(M - 1)


# ------------------------------------------------------------------------------------------------ pieces of section 1
def split(A):
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    D = A.shape[1]
    h = D // 2
    return np.concatenate([A[:, :h], A[:, D - h:]], axis=0)


def ranks(A):
    """average ranks from two binary searches in the sorted values (what k_conv_rank_z does)"""
    a = np.asarray(A, dtype=np.float64).ravel()
    s = np.sort(a)
    lo, hi = np.searchsorted(s, a, "left"), np.searchsorted(s, a, "right")
    return ((lo + hi + 1).astype(np.float64) / 2.0).reshape(np.shape(A))


def z_scipy(A):
    from scipy import stats
    A = np.asarray(A, dtype=np.float64)
    r = stats.rankdata(A.ravel(), "average")
    return stats.norm.ppf((r - 3.0 / 8.0) / (A.size + 1.0 / 4.0)).reshape(A.shape)


def acov_fft(Y):
    """(R, n): the biased autocovariance of every row by arviz's route (zero-padded FFT of the centred row)"""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    n = Y.shape[1]
    m = 1
    while m < 2 * n:
        m *= 2
    y = Y - Y.mean(axis=1, keepdims=True)
    f = np.fft.rfft(y, n=m, axis=1)
    return np.fft.irfft(f * np.conjugate(f), n=m, axis=1)[:, :n] / n


def acov_fixed(Y, lag0, nlags, mean=None):
    """(R, nlags): the kernel's order -- per lag ONE accumulator from 0.0 over the ascending i of a chunk, the chunks added in
    ascending order, the sum divided by n; lags >= n give 0"""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    R, n = Y.shape
    if mean is None:
        mean = moments(Y)[0]
    y = Y - np.asarray(mean)[:, None]
    out = np.zeros((R, nlags))
    ypad = np.concatenate([y, np.zeros((R, n + nlags + lag0))], axis=1)       # (an added 0.0 changes no accumulator)
    for j0 in range(0, nlags, 128):
        ks = lag0 + np.arange(j0, min(nlags, j0 + 128))
        tot = np.zeros((R, ks.size))
        for c0 in range(0, n, CHUNK):
            i = np.arange(c0, min(n, c0 + CHUNK))
            prod = y[:, None, i] * ypad[:, ks[:, None] + i[None, :]]
            tot = tot + (0.0 + np.cumsum(prod, axis=2)[:, :, -1])
        out[:, j0:j0 + ks.size] = tot / np.float64(n)
    return out


def ess(A, route="fixed", info=None):
    """section 1's ess of A (M, n); ``info`` (a dict) receives max_t and the smallest |even + odd| of the evaluated pairs"""
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    M, n = A.shape
    mean, _, lo, hi = moments(A)
    if A.max() - A.min() < 1e-15:
        return np.float64(A.size)
    def rowmean(ac):       # sequential over ascending m
        tot = np.zeros(ac.shape[1])
        for m in range(M):
            tot = tot + ac[m]
        return tot / np.float64(M)

    macs = rowmean(acov_fft(A)) if route == "fft" else np.zeros(0)

    def mac(t):
        nonlocal macs
        while t >= macs.size:
            more = min(n, max(64, 4 * macs.size)) - macs.size
            macs = np.concatenate([macs, rowmean(acov_fixed(A, macs.size, more, mean))])
        return macs[t]

    with np.errstate(all="ignore"):
        dn = np.float64(n)
        mean_var = mac(0) * dn / (dn - 1.0)
        var_plus = mean_var * (dn - 1.0) / dn
        if M > 1:
            var_plus = var_plus + seq_var1(mean)

        def rho_of(t):
            return 1.0 - (mean_var - mac(t)) / var_plus

        rho = np.zeros(n + 2)
        rho[0] = 1.0
        rho[1] = rho_of(1)
        even, odd, t = np.float64(1.0), rho[1], 1
        gap, nan = np.inf, bool(np.isnan(rho[1]))
        while t < n - 3 and even + odd > 0:
            even, odd = rho_of(t + 1), rho_of(t + 2)
            gap = min(gap, abs(even + odd))
            if even + odd >= 0:
                rho[t + 1], rho[t + 2] = even, odd
                nan = nan or bool(np.isnan(even) or np.isnan(odd))
            t += 2
        max_t = t - 2
        if even > 0:
            rho[max_t + 1] = even
        t = 1
        while t <= max_t - 2:
            if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
                rho[t + 1] = (rho[t - 1] + rho[t]) / 2.0
                rho[t + 2] = rho[t + 1]
            t += 2
        tau = (-1.0 + 2.0 * seq_sum(rho[:max_t + 1])) + rho[max_t + 1]
        floor = np.float64(1.0) / np.log10(np.float64(M * n))
        if not tau >= floor and not np.isnan(tau):
            tau = floor
        if info is not None:
            info["max_t"], info["gap"] = max_t, gap
        return np.float64(np.nan) if nan else np.float64(M * n) / tau


def rhat(A):
    """sqrt((B / W + n - 1) / n) of A (M, n) from the row moments, sequential over the rows"""
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    M, n = A.shape
    mean, css, _, _ = moments(A)
    dn = np.float64(n)
    with np.errstate(all="ignore"):
        W = seq_sum(css / (dn - 1.0)) / np.float64(M)
        B = dn * seq_var1(mean)
        return np.sqrt(((B / W + dn) - 1.0) / dn)


def rhat_textbook(A):
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    M, n = A.shape
    means = [sum(row) / n for row in A.tolist()]
    grand = sum(means) / M
    B = n * sum((m - grand) ** 2 for m in means) / (M - 1)
    W = sum(sum((x - m) ** 2 for x in row) / (n - 1) for row, m in zip(A.tolist(), means)) / M
    return np.sqrt((B / W + n - 1) / n)


def hdi(x, hdi_prob=0.94):
    s = np.sort(np.asarray(x, dtype=np.float64).ravel())
    S = s.size
    inc = min(int(np.floor(hdi_prob * S)), S - 1)
    w = s[inc:] - s[:S - inc]
    j = int(np.argmin(w))
    return s[j], s[j + inc]


def mcse_columns(sd, ess_mean, ess_sd):
    with np.errstate(all="ignore"):
        return sd / np.sqrt(ess_mean), sd * np.sqrt(np.exp(1) * (1 - 1 / ess_sd) ** (ess_sd - 1) - 1)


def summary_column(X, hdi_prob=0.94, route="fixed", z=None, info=None):
    """the 11 entries of one variable X (C, D); ``z``: a function A -> z(A) (default: scipy's).  ``info``: a dict that
    receives the smallest gap and the largest max_t over the five scans"""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    C, D = X.shape
    S = C * D
    z = z or z_scipy
    out = np.full(len(COLUMNS), np.nan)
    if not np.all(np.isfinite(X)):
        return out
    flat = X.reshape(1, S)
    mean, css, _, _ = moments(flat)
    with np.errstate(all="ignore"):
        out[0], out[1] = mean[0], np.sqrt(css[0] / np.float64(S - 1))
    out[2], out[3] = hdi(flat, hdi_prob)
    if D < 4:
        return out
    sp = split(X)
    q05, q95 = np.quantile(flat, 0.05), np.quantile(flat, 0.95)
    sets = dict(mean=sp, sd=(sp - mean[0]) * (sp - mean[0]), t05=(sp <= q05).astype(np.float64),
                t95=(sp <= q95).astype(np.float64), bulk=z(sp))
    e = {}
    for k, A in sets.items():
        i = {}
        e[k] = ess(A, route, i)
        if info is not None and i:
            info["gap"] = min(info.get("gap", np.inf), i["gap"])
            info["max_t"] = max(info.get("max_t", -1), i["max_t"])
    folded = z(np.abs(sp - np.percentile(sp, 50)))     # (the 50 % quantile of k_col_percentiles)
    r0, r1 = rhat(sets["bulk"]), rhat(folded)
    out[6] = e["bulk"]
    out[7] = np.nan if np.isnan(e["t05"]) or np.isnan(e["t95"]) else min(e["t05"], e["t95"])
    out[8] = np.nan if np.isnan(r0) or np.isnan(r1) else max(r0, r1)
    out[9], out[10] = e["mean"], e["sd"]
    return out      # (the two MCSE are formed by ``summary`` on whole columns, as the package forms them)


def summary(X, hdi_prob=0.94, route="fixed", z=None, info=None):
    """(V, 11) of X (C, D, V); mcse_mean and mcse_sd from the whole sd and ess columns (numpy's power may round an array
    and a scalar differently, and the -1 of mcse_sd magnifies that)"""
    X = np.asarray(X, dtype=np.float64)
    t = np.array([summary_column(X[:, :, v], hdi_prob, route, z, info) for v in range(X.shape[2])]).reshape(X.shape[2], -1)
    t[:, 4], t[:, 5] = mcse_columns(t[:, 1], t[:, 9], t[:, 10])
    return t


def ar1(rng, C, D, phi, V=None):
    """C chains of D draws of a stationary unit-variance AR(1) process (V of them: (C, D, V))"""
    shape = (C, D) if V is None else (C, D, V)
    e = rng.standard_normal(shape)
    x = np.empty(shape)
    x[:, 0] = e[:, 0]
    s = np.sqrt(1.0 - phi * phi)
    for d in range(1, D):
        x[:, d] = phi * x[:, d - 1] + s * e[:, d]
    return x


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
GRID_C, GRID_D, GRID_V = (1, 2, 3, 8), (4, 5, 37, 128, 129, 130), (1, 3, 65)
_INPUTS = {}


def grid_input(C, D, V):
    """the trace of a grid case: AR(1) chains (phi = 0.3) with a scale and an offset per variable"""
    key = (C, D, V)
    if key not in _INPUTS:
        rng = np.random.default_rng(7000 + 1000 * C + 10 * D + V)
        _INPUTS[key] = ar1(rng, C, D, 0.3, V) * 10.0 ** rng.integers(-3, 4, V) + rng.normal(0.0, 5.0, V)
    return _INPUTS[key]


def special_inputs():
    """name -> trace: a constant column, a column with one NaN, slowly mixing chains (max_t beyond 64 and 128)"""
    if "special" not in _INPUTS:
        rng = np.random.default_rng(7)
        const = ar1(rng, 2, 36, 0.3, 3)
        const[:, :, 1] = 2.5
        nan = ar1(rng, 3, 129, 0.3, 3)
        nan[1, 77, 2] = np.nan
        _INPUTS["special"] = dict(constant=const, nan=nan, ar99=ar1(rng, 2, 2400, 0.99, 2))
    return _INPUTS["special"]
