"""TEST INFRASTRUCTURE ONLY.  The numpy restatement of csrc/predcov.hip's k_pred_center / k_pred_cov, operation by
operation in the kernels' order (every numpy operation below is one IEEE operation per element: no fused multiply-add, no
pairwise summation), so the device result can be compared with ``array_equal``:

    mean_j  = (((0 + X[0,j]) + X[1,j]) + ...) / K
    D[k,j]  = X[k,j] - mean_j
    out_i   = base_i + (((0 + D[0,a] D[0,b]) + D[1,a] D[1,b]) + ...) / (K - 1)

and the first-order bound the sample covariance is held to against ``numpy.cov``."""
import numpy as np

PC_TILE, PC_KC = 64, 32      # k_pred_cov's output tile edge and k-chunk length (csrc/predcov.hip)


def center(X):
    X = np.asarray(X, dtype=np.float64)
    s = np.zeros(X.shape[1])
    for k in range(X.shape[0]):
        s = s + X[k]
    return X - (s / float(X.shape[0]))[None, :]


def pred_covariance(X, sizes, base=None):
    """X (K, Nobs), sizes of the datasets (their sum is Nobs), base: None or a list of None / (n_i, n_i) -> list of (n_i, n_i)"""
    X = np.asarray(X, dtype=np.float64)
    K = X.shape[0]
    if K < 2:
        raise ValueError("a sample covariance needs at least 2 rows")
    D = center(X)
    out, o = [], 0
    for i, n in enumerate(sizes):
        d = D[:, o:o + n]
        acc = np.zeros((n, n))
        for k in range(K):
            acc = acc + d[k][:, None] * d[k][None, :]
        b = np.zeros((n, n)) if base is None or base[i] is None else np.asarray(base[i], dtype=np.float64)
        out.append(b + acc / float(K - 1))
        o += n
    return out


def cov_bound(X):
    """8 (K + 3) 2^-53 a_i a_j, a_j = max_k |X[k,j]|: a first-order bound on the rounding error of the sample covariance of
    the columns of X that holds for ANY order of the sums of mean, centring and products, u = 2^-53, K >= 2.  Sketch: the
    mean carries K u a (K - 1 additions, one division), a centred value d therefore (K + 2) u a; with sum_k d_k^2 <=
    K a^2 (Cauchy-Schwarz for the mixed sums) the K products carry (2 (K + 2) + 1) K u a_i a_j, their summation
    (K - 1) K u a_i a_j, and after the division by K - 1 the total stays under K / (K - 1) (3 K + 5) u a_i a_j, which is
    below 8 (K + 3) u a_i a_j.  The tests allow TWICE this bound between two implementations, each inside it."""
    X = np.asarray(X, dtype=np.float64)
    a = np.abs(X).max(axis=0)
    return 8.0 * (X.shape[0] + 3) * 2.0 ** -53 * a[:, None] * a[None, :]
