"""CPU tests of tests/misfit_ref.py, the expectation of tests/test_gpu_misfit_edges.py: the exact generators stay inside the
exactly representable range and their int64 result is what float64 gives; every admitted real-valued case lets three honest
float64 evaluations (natural, permuted, reversed order) through its derived bound and catches a float32 evaluation by a factor
of 100 at least; the long double reference agrees with 40-digit arithmetic."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import misfit_ref as mref  # noqa: E402


def _exact_cases():
    rng = np.random.default_rng(1)
    yield mref.QuadCase("dense 1030", mref.int_dense(rng, 1, 1030), mref.int_values(rng, (5, 1, 1030)))
    yield mref.QuadCase("upper 131", mref.int_dense(rng, 3, 131, upper=True), mref.int_values(rng, (9, 3, 131)))
    yield mref.QuadCase("shared 400", mref.int_dense(rng, 1, 400)[0], mref.int_values(rng, (7, 3, 400)), shared=True)
    yield mref.QuadCase("band 16", mref.int_banded(rng, 3, 513, (16, 5, 16)), mref.int_values(rng, (9, 3, 513)), band=16)
    yield mref.QuadCase("band 1", mref.int_banded(rng, 2, 1025, (1, 1)), mref.int_values(rng, (17, 2, 1025)), band=1)
    yield mref.QuadCase("band 0", mref.int_banded(rng, 3, 33, (0, 0, 0)), mref.int_values(rng, (7, 3, 33)), band=0)
    yield mref.QuadCase("scalar", 2.0 ** np.array([-3.0, 0.0, 2.0]), mref.int_values(rng, (5, 3, 200)), scalar=True)


def test_exact_generators_stay_below_2_53_and_int64_equals_float64():
    """quad_exact asserts the range itself (sum of absolute terms); the largest value is far below 2^53; numpy's float64
    product of the same integers -- BLAS, any order, fused or not -- gives the same numbers"""
    worst = 0
    for case in _exact_cases():
        q = mref.quad_exact(case)
        worst = max(worst, float(np.abs(q).max()))
        assert q.shape == (case.C, case.nd)
        for order in ("natural", "reversed", "permuted"):
            assert np.array_equal(mref.quad_eval(case, np.float64, order, seed=3), q), (case.name, order)
        if not case.scalar:
            W = np.broadcast_to(case.W, (case.nd, case.M, case.M))
            y = np.einsum("dik,cdk->cdi", W, case.X)
            assert np.array_equal((y * y).sum(axis=2), q), case.name
            # the banded form of the reference is the dense one
            dense = mref.QuadCase(case.name, W, case.X)
            assert np.array_equal(mref.quad_exact(dense), q), case.name
    print("largest exact quad %.3g (2^53 = %.3g)" % (worst, 2.0 ** 53))
    assert worst < 2.0 ** 43


def test_exact_range_at_the_extreme():
    """all entries +-7 at M = 1100: |y| = 49 * 1100 < 2^16, the sum 1100 * 53900^2 < 2^43 -- the docstring's arithmetic"""
    M = 1100
    case = mref.QuadCase("extreme", np.full((1, M, M), 7.0), np.full((1, 1, M), -7.0))
    q = mref.quad_exact(case)
    assert q[0, 0] == M * (49 * M) ** 2 and 49 * M < 2 ** 16 and q[0, 0] < 2 ** 43


def test_band_packing_round_trip():
    rng = np.random.default_rng(2)
    W = mref.int_banded(rng, 3, 40, (5, 2, 0))
    assert mref.half_bandwidth(W) == 5 and mref.half_bandwidth(W[1:]) == 2 and mref.half_bandwidth(W[2:]) == 0
    wb = mref.pack_band(W, 5)
    assert np.array_equal(mref.unpack_band(wb), W)
    assert np.array_equal(np.tril(W, -1), np.zeros_like(W)) and np.array_equal(np.triu(W, 6), np.zeros_like(W))


def test_exponential_operator_is_a_differencing_operator():
    """rows (a, -rho a), the last row (1 / sqrt(scale)): the smooth residuals cancel to a fraction of their size, which is what
    makes a relative tolerance on quad the wrong yardstick and S the right one"""
    M = 513
    W = mref.exponential_bidiagonal(M)
    rho = np.exp(-0.25)
    a = 1.0 / np.sqrt(1.0 - rho * rho)
    assert np.allclose(np.diag(W)[:-1], a, rtol=1e-12) and np.allclose(np.diag(W, 1), -rho * a, rtol=1e-12)
    assert np.isclose(W[-1, -1], 1.0, rtol=1e-12) and mref.half_bandwidth(W[None]) == 1
    case = mref.QuadCase("smooth", W[None], mref.smooth_residuals(3, 1, M), band=1)
    ref, S = mref.quad_ref(case)
    assert (np.asarray(ref, dtype=np.float64) < 0.02 * S).all()


@pytest.mark.parametrize("name", sorted(mref.REAL_CASES))
def test_real_case_admits_float64_and_rejects_float32(name):
    case = mref.real_case(name)
    ref, S = mref.quad_ref(case)
    bound = mref.quad_bound(case, S)
    assert (bound > 0).all()
    for order in ("natural", "permuted", "reversed"):
        ratio = (mref.hp_error(mref.quad_eval(case, np.float64, order, seed=7), ref) / bound).max()
        print("%s float64 %s: error / bound = %.4f" % (name, order, ratio))
        assert ratio <= 1.0, (name, order, ratio)
    r32 = mref.hp_error(mref.quad_eval(case, np.float32).astype(np.float64), ref) / bound
    print("%s float32: error / bound = %.3g (median %.3g)" % (name, r32.max(), np.median(r32)))
    assert r32.max() >= 100.0 and np.median(r32) >= 100.0, (name, r32.max(), np.median(r32))


def test_geo_reference_and_bound():
    rng = np.random.default_rng(5)
    G, s, mu0 = mref.int_values(rng, (400, 129)), mref.int_values(rng, (7, 400)), mref.int_values(rng, (7, 129))
    mu = mref.geo_exact(G, s, mu0)
    assert np.array_equal(mu, mu0 + s @ G) and np.abs(mu).max() < 2 ** 53
    for order in ("natural", "reversed", "permuted"):
        assert np.array_equal(mref.geo_eval(G, s, np.float64, order, seed=1) + mu0, mu)
    G, s = mref.geo_real_case()
    ref, bound = mref.geo_ref(G, s)
    for order in ("natural", "permuted", "reversed"):
        ratio = (mref.hp_error(mref.geo_eval(G, s, np.float64, order, seed=7), ref) / bound).max()
        print("geo float64 %s: error / bound = %.4f" % (order, ratio))
        assert ratio <= 1.0
    r32 = mref.hp_error(mref.geo_eval(G, s, np.float32).astype(np.float64), ref) / bound
    print("geo float32: error / bound = %.3g (median %.3g)" % (r32.max(), np.median(r32)))
    assert r32.max() >= 100.0 and np.median(r32) >= 100.0


def test_longdouble_reference_against_40_digits():
    """two small cases, dense and bidiagonal: the reference within 2 (K + M) 2^-64 S of mpmath at 40 digits -- 2^-11 of the bound
    the kernels are held to"""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp.clone()
    mp.dps = 40
    rng = np.random.default_rng(40)
    cases = [mref.QuadCase("dense 17", rng.standard_normal((2, 17, 17)), rng.standard_normal((3, 2, 17))),
             mref.QuadCase("smooth 65", mref.exponential_bidiagonal(65)[None], mref.smooth_residuals(3, 1, 65), band=1)]
    for case in cases:
        ref, S = mref.quad_ref(case)
        w, col = case.rows()
        for c in range(case.C):
            for d in range(case.nd):
                q = mp.mpf(0)
                for i in range(case.M):
                    y = mp.mpf(0)
                    for k in range(case.K):
                        y += mp.mpf(float(w[d, i, k])) * mp.mpf(float(case.X[c, d, col[i, k]]))
                    q += y * y
                # the reference's value as an exact sum of two doubles
                hi = float(ref[c, d])
                lo = float(ref[c, d] - type(ref[c, d])(hi)) if mref.HAVE_LONGDOUBLE else float(ref[c, d] - mref.Fraction(hi))
                err = abs(mp.mpf(hi) + mp.mpf(lo) - q)
                tol = 2 * (case.K + case.M) * 2.0 ** -64 * S[c, d]
                assert err <= tol, (case.name, c, d, float(err), tol)
