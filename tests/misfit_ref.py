"""Host-only references and input generators of the misfit kernels quad[c, d] = |W_d x_{c,d}|^2 (csrc/quadform.hip: the
dense FP64-MFMA kernel, the general banded kernel, the bidiagonal canonical-order kernel; csrc/logp.hip: the scalar kernel)
and of the geodetic stacking mu = G.T s that feeds them (k_geo_stack).  Pinned by tests/test_misfit_ref_host.py, used as the
expectation of tests/test_gpu_misfit_edges.py.  TEST INFRASTRUCTURE ONLY.

Two kinds of input:

EXACT.  Weights, residuals, Green's functions and slips are integers in [-7, 7] stored as float64.  For M, P <= 1100 a whitened
sample is |y_i| <= 49 * 1100 < 2^16 and sum_i y_i^2 < 2^43: every product, partial sum and square is an integer below 2^53,
so it is exact in float64 in any order, fused or not.  The reference is int64 arithmetic and the comparison is equality.

REAL VALUED.  The reference is evaluated in np.longdouble (64-bit significand; Python fractions where the platform's long double
is no wider than a double) and comes with S = sum_i (sum_k |W_ik| |x_k|)^2.  The tolerance is derived, not tuned:

    |quad - quad_ref| <= (2 K + M + 8) u S,   u = 2^-53,  K = stored terms per row (M dense, band + 1 banded)

a K-term dot product in any order, fused or not, has error <= K u a_i with a_i = sum_k |W_ik| |x_k|; squaring doubles the
relative error (2 K u a_i^2); summing M non-negative squares in any order adds M u; the constant 8 absorbs the O(u^2) terms and
the reference's own rounding (2^-64 relative per operation).  For the stacking: |mu - ref| <= (P + 2) u sum_p |G_pk s_p|.

A real-valued case is admitted only where the bound can see a precision loss: test_misfit_ref_host.py requires a float32
evaluation of the same case to miss the bound by a factor of 100 at least.  The dense cases stop at M = 257 (the bound grows
with M while the error of a float32 evaluation does not: the margin is 1e5 at M = 257 and 5e3 at M = 1030), the banded ones
go up to M = 1030; the dense kernel at large M is judged by the exact cases."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LIMIT = 2 ** 53
HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63


# ------------------------------------------------------------------------------------------------- high precision plumbing
def _hp(a):
    """float64 array -> np.longdouble, or an object array of Fractions where long double is a double"""
    a = np.asarray(a, dtype=np.float64)
    if HAVE_LONGDOUBLE:
        return a.astype(np.longdouble)
    out = np.empty(a.shape, dtype=object)
    flat = out.reshape(-1)
    for i, v in enumerate(a.reshape(-1)):
        flat[i] = Fraction(float(v))
    return out


def hp_error(got, ref):
    """|got - ref| as float64 for a float64 result and a high-precision reference (the difference is formed in high precision)"""
    d = _hp(got) - ref
    if HAVE_LONGDOUBLE:
        return np.abs(d).astype(np.float64)
    return np.array([abs(float(v)) for v in d.reshape(-1)]).reshape(d.shape)


# ------------------------------------------------------------------------------------------------- operators
def pack_band(W, band):
    """dense (nd, M, M) -> (nd, M, band + 1): wb[d, i, k] = W[d, i, i + k], 0 past the last column (k_band_pack)"""
    W = np.asarray(W)
    nd, M, _ = W.shape
    wb = np.zeros((nd, M, band + 1), dtype=W.dtype)
    for k in range(min(band, M - 1) + 1):
        wb[:, :M - k, k] = np.diagonal(W, k, 1, 2)
    return wb


def unpack_band(wb):
    """(nd, M, K) -> dense upper-triangular (nd, M, M) with exact zeros outside the band"""
    wb = np.asarray(wb)
    nd, M, K = wb.shape
    W = np.zeros((nd, M, M), dtype=wb.dtype)
    i = np.arange(M)
    for k in range(min(K, M)):
        W[:, i[:M - k], i[:M - k] + k] = wb[:, :M - k, k]
    return W


def half_bandwidth(W):
    """largest column - row of a non-zero entry over all matrices of the stack (what beatamd_weights_band reports for exact
    zeros outside the band)"""
    W = np.asarray(W)
    r, c = np.nonzero(np.abs(W).max(axis=0))
    return int((c - r).max()) if r.size else 0


def int_values(rng, shape, nonzero=False):
    """integers in [-7, 7] as float64"""
    v = rng.integers(-7, 8, size=shape)
    if nonzero:
        v = np.where(v == 0, 3, v)
    return v.astype(np.float64)


def int_dense(rng, nd, M, upper=False):
    """full (or full upper-triangular) integer operators (nd, M, M)"""
    W = int_values(rng, (nd, M, M))
    return np.triu(W) if upper else W


def int_banded(rng, nd, M, bands):
    """integer upper-triangular band operators, dataset d of half bandwidth bands[d] (its outermost diagonal and the main
    diagonal without zeros, exact zeros outside): (nd, M, M)"""
    W = np.zeros((nd, M, M))
    for d in range(nd):
        b = min(int(bands[d]), M - 1)
        wb = int_values(rng, (1, M, b + 1))
        wb[0, :, 0] = int_values(rng, M, nonzero=True)
        wb[0, :, b] = int_values(rng, M, nonzero=True)
        W[d] = unpack_band(wb)[0]
    return W


def exponential_bidiagonal(M, dt=0.5, tzero=2.0, scale=1.0):
    """the band of W = chol(inv(C)).T for the reference's "exponential" noise structure C_ij = scale * exp(-|i - j| dt / tzero)
    (covariance.py:24-51, heart.py:216-237): W is bidiagonal up to rounding residue (~1e-15 of its largest entry), which is
    cut here so that reference and kernel see the same operator: (M, M) with exact zeros outside the two diagonals.  Its rows
    are (a, -rho a) with rho = exp(-dt / tzero): a differencing operator"""
    i = np.arange(M)
    C = scale * np.exp(-np.abs(i[:, None] - i[None, :]) * (dt / tzero))
    W = np.linalg.cholesky(np.linalg.inv(C)).T
    assert np.abs(np.triu(W, 2)).max() < 1e-12 * np.abs(W).max() and np.abs(np.tril(W, -1)).max() == 0.0
    return np.triu(np.tril(W, 1))


def smooth_residuals(C, nd, M):
    """3 + sin(0.01 j (c + 1)): smooth traces, which the differencing operator above cancels to a tenth of their size"""
    j = np.arange(M, dtype=np.float64)
    c = np.arange(C, dtype=np.float64) + 1.0
    return np.repeat((3.0 + np.sin(0.01 * j[None, :] * c[:, None]))[:, None, :], nd, axis=1)


# ------------------------------------------------------------------------------------------------- cases
class QuadCase(object):
    """one weight set and one batch of residuals.  W (nd, M, M) float64 as uploaded (shared=True: one (M, M) operator for all nd,
    the Laplacian's a_stride = 0); X (C, nd, M); band: None = every column of a row is a stored term (K = M), otherwise the
    rows hold band + 1 terms; scalar: W is (nd,) and the operator is W_d * I"""

    def __init__(self, name, W, X, band=None, shared=False, scalar=False):
        self.name, self.band, self.shared, self.scalar = name, band, shared, scalar
        self.W = np.ascontiguousarray(W, dtype=np.float64)
        self.X = np.ascontiguousarray(X, dtype=np.float64)
        self.C, self.nd, self.M = self.X.shape
        self.K = 1 if scalar else (self.M if band is None else band + 1)

    def rows(self):
        """(w (nd, M, K), col (M, K)): term k of row i multiplies x[col[i, k]]; columns past the trace point at a zero weight"""
        M = self.M
        if self.scalar:
            return np.broadcast_to(self.W[:, None, None], (self.nd, M, 1)), np.arange(M)[:, None]
        W = np.broadcast_to(self.W, (self.nd, M, M)) if self.shared else self.W
        if self.band is None:
            return W, np.broadcast_to(np.arange(M)[None, :], (M, M))
        col = np.arange(M)[:, None] + np.arange(self.K)[None, :]
        return pack_band(W, self.band), np.minimum(col, M - 1)

    def sub(self, lo, hi):
        """the same weight set with chains lo:hi"""
        return QuadCase("%s[%d:%d]" % (self.name, lo, hi), self.W, self.X[lo:hi], self.band, self.shared, self.scalar)


def quad_exact(case):
    """int64 |W x|^2 (C, nd) of an integer case; asserts that nothing leaves the exactly representable range"""
    w, col = case.rows()
    wi, xi = np.rint(w).astype(np.int64), np.rint(case.X).astype(np.int64)
    if not case.scalar:
        assert np.array_equal(wi, w) and np.abs(wi).max() <= 7, case.name + ": weights are not integers in [-7, 7]"
    assert np.array_equal(xi, case.X), case.name + ": residuals are not integers"
    if case.scalar:
        # power-of-two weights: (w x)^2 = w^2 x^2 exactly, the sum of the integer squares scaled by w^2
        m, e = np.frexp(case.W)
        assert np.all(m == 0.5), case.name + ": scalar weights are not powers of two"
        q = (xi * xi).sum(axis=2)
        assert q.max() < LIMIT and np.abs(e).max() <= 16
        return q.astype(np.float64) * (case.W ** 2)[None, :]
    if case.band is None:
        y = np.einsum("dik,cdk->cdi", wi, xi)
        ya = np.einsum("dik,cdk->cdi", np.abs(wi), np.abs(xi))
    else:
        y = np.zeros((case.C, case.nd, case.M), dtype=np.int64)
        ya = np.zeros_like(y)
        for k in range(case.K):
            y += wi[None, :, :, k] * xi[:, :, col[:, k]]
            ya += np.abs(wi[None, :, :, k] * xi[:, :, col[:, k]])
    q = (y * y).sum(axis=2)
    assert (ya * ya).sum(axis=2).max() < LIMIT, case.name + ": a partial sum may leave 2^53"
    return q


def quad_ref(case):
    """-> (quad_ref (C, nd) in high precision, S (C, nd) float64) of a real-valued case"""
    w, col = case.rows()
    wh, xh = _hp(np.ascontiguousarray(w)), _hp(case.X)
    wa, xa = np.abs(np.ascontiguousarray(w)), np.abs(case.X)
    if case.band is None and not case.scalar:
        y = np.stack([xh[:, d] @ wh[d].T for d in range(case.nd)], axis=1)
        a = np.einsum("dik,cdk->cdi", wa, xa)
    else:
        y = wh[None, :, :, 0] * xh[:, :, col[:, 0]]
        a = wa[None, :, :, 0] * xa[:, :, col[:, 0]]
        for k in range(1, case.K):
            y = y + wh[None, :, :, k] * xh[:, :, col[:, k]]
            a = a + wa[None, :, :, k] * xa[:, :, col[:, k]]
    return (y * y).sum(axis=2), (a * a).sum(axis=2) * (1.0 + 4.0 * case.M * U)   # (S itself rounded upwards)


def quad_bound(case, S):
    """(2 K + M + 8) u S"""
    return (2 * case.K + case.M + 8) * U * np.asarray(S, dtype=np.float64)


def quad_eval(case, dtype=np.float64, order="natural", seed=0):
    """plain evaluation in `dtype`: the terms of a row and the squares of a trace added one by one in natural, reversed or a
    random (seeded) order, multiply and add rounded separately.  What a correct kernel may do, in a precision of choice"""
    w, col = case.rows()
    w, x = np.ascontiguousarray(w).astype(dtype), case.X.astype(dtype)
    rng = np.random.default_rng(seed)
    ks, rows = np.arange(case.K), np.arange(case.M)
    if order == "reversed":
        ks, rows = ks[::-1], rows[::-1]
    elif order == "permuted":
        ks, rows = rng.permutation(ks), rng.permutation(rows)
    else:
        assert order == "natural"
    y = np.zeros((case.C, case.nd, case.M), dtype=dtype)
    for k in ks:
        y += w[None, :, :, k] * x[:, :, col[:, k]]
    q = np.zeros((case.C, case.nd), dtype=dtype)
    for i in rows:
        q += y[:, :, i] * y[:, :, i]
    return q


# ------------------------------------------------------------------------------------------------- the admitted real-valued cases
def _normal_case(name, seed, C, nd, M, band=None):
    rng = np.random.default_rng(seed)
    if band is None:
        W = rng.standard_normal((nd, M, M))
    else:
        W = unpack_band(rng.standard_normal((nd, M, band + 1)))
    return QuadCase(name, W, rng.standard_normal((C, nd, M)), band)


def _exponential_case(name, seed, C, nd, M, smooth):
    W = np.stack([exponential_bidiagonal(M, scale=0.3 + d) for d in range(nd)])
    X = smooth_residuals(C, nd, M) if smooth else np.random.default_rng(seed).standard_normal((C, nd, M))
    return QuadCase(name, W, X, band=1)


REAL_CASES = {}
for _M in (17, 65, 257):
    REAL_CASES["dense M=%d" % _M] = lambda M=_M: _normal_case("dense M=%d" % M, 100 + M, 65, 2, M)
REAL_CASES["band 5 M=257"] = lambda: _normal_case("band 5 M=257", 205, 9, 3, 257, band=5)
for _M in (65, 513, 1030):
    REAL_CASES["band 1 random M=%d" % _M] = lambda M=_M: _exponential_case("band 1 random M=%d" % M, 300 + M, 17, 2, M, False)
    REAL_CASES["band 1 smooth M=%d" % _M] = lambda M=_M: _exponential_case("band 1 smooth M=%d" % M, 0, 17, 2, M, True)


def real_case(name):
    return REAL_CASES[name]()


# ------------------------------------------------------------------------------------------------- geodetic stacking
def geo_exact(G, slips, mu0=None):
    """int64 mu[c, k] = mu0[c, k] + sum_p G[p, k] s[c, p] of integer G (P, Nobs), slips (C, P) and start values"""
    Gi, si = np.rint(G).astype(np.int64), np.rint(slips).astype(np.int64)
    assert np.array_equal(Gi, G) and np.array_equal(si, slips) and np.abs(Gi).max() <= 7 and np.abs(si).max() <= 7
    m0 = np.zeros((si.shape[0], Gi.shape[1]), dtype=np.int64) if mu0 is None else np.rint(mu0).astype(np.int64)
    assert mu0 is None or np.array_equal(m0, mu0)
    mu = m0 + si @ Gi
    assert (np.abs(m0) + np.abs(si) @ np.abs(Gi)).max() < LIMIT
    return mu


def geo_ref(G, slips):
    """-> (mu_ref (C, Nobs) in high precision, bound (C, Nobs) = (P + 2) u sum_p |G_pk s_p|)"""
    G, slips = np.asarray(G, dtype=np.float64), np.asarray(slips, dtype=np.float64)
    mu = _hp(slips) @ _hp(G)
    return mu, (G.shape[0] + 2) * U * (np.abs(slips) @ np.abs(G)) * (1.0 + 4.0 * G.shape[0] * U)


def geo_eval(G, slips, dtype=np.float64, order="natural", seed=0):
    G, s = np.asarray(G).astype(dtype), np.asarray(slips).astype(dtype)
    ps = np.arange(G.shape[0])
    if order == "reversed":
        ps = ps[::-1]
    elif order == "permuted":
        ps = np.random.default_rng(seed).permutation(ps)
    mu = np.zeros((s.shape[0], G.shape[1]), dtype=dtype)
    for p in ps:
        mu += s[:, p, None] * G[None, p, :]
    return mu


def geo_real_case():
    """P = 400 patches, 129 observation points, 67 chains"""
    rng = np.random.default_rng(400129)
    return rng.standard_normal((400, 129)), rng.standard_normal((67, 400))
