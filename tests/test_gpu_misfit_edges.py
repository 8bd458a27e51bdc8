"""The misfit kernels |W r|^2 at their tile, band and batch edges, against the references of tests/misfit_ref.py: the dense
FP64-MFMA kernel k_quadform (64 -> 128 chains per block, several chain blocks, the XCD-aware workgroup decode, M around the
16-wide k tile and the 64-row block, the scalar-load fallback), the general banded kernel k_quadform_banded<0> (bands 0 .. 16,
the 8-chain block, the 256-thread sample stride), the bidiagonal canonical-order kernel k_quadform_band1 (chunks of 512
samples, one-sample chunks, odd traces, a misaligned dataset), the scalar kernel k_scalar_quad, the band detector and packer
that choose between them, and k_geo_stack (its 16-deep double-buffered prefetch over patches, the 1-chain and 4-chain tile,
accumulate mode, the limit of 8192 patch slips).

Integer inputs: int64 reference, np.array_equal -- no tolerance.  Real-valued inputs: long double reference and the derived
bound (2 K + M + 8) 2^-53 S of misfit_ref.py (the stacking: (P + 2) 2^-53 sum |G s|); every test prints its largest
error / bound.  A chain's value does not depend on the batch it is evaluated in, to the bit, for all four families."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import misfit_ref as mref  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LOG_2PI = 1.8378770664093453


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


# ----------------------------------------------------------------------------- helpers
def _create(ctx, case):
    if case.scalar:
        return ctx.weights_create_scalar(case.W, np.zeros(case.nd), case.M)
    return ctx.weights_create_dense(case.W, np.zeros(case.nd))


def _misaligned(X):
    """the same values as a contiguous device tensor that starts 8 bytes into a 16-byte aligned buffer"""
    import torch
    buf = torch.empty(X.size + 2, dtype=torch.float64, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    v = buf[1:X.size + 1]
    v.copy_(torch.from_numpy(np.ascontiguousarray(X).reshape(-1)))
    v = v.view(X.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 8
    return v


def _assert_exact(got, case):
    ref = mref.quad_exact(case)
    assert got.dtype == np.float64 and got.shape == ref.shape
    assert np.array_equal(got, ref), "%s: %d of %d values differ, first at %s" % (
        case.name, (got != ref).sum(), ref.size, np.argwhere(got != ref)[:4].tolist())


def _check_exact(ctx, wid, case, misaligned=True):
    got = ctx.wset_quad_batch(wid, case.X)
    _assert_exact(got, case)
    if misaligned:
        off = ctx.wset_quad_batch(wid, _misaligned(case.X)).cpu().numpy()
        assert np.array_equal(off, got), case.name + ": misaligned residuals give other bits"
    return got


def _check_bound(ctx, wid, case, what):
    ref, S = mref.quad_ref(case)
    got = ctx.wset_quad_batch(wid, case.X)
    ratio = (mref.hp_error(got, ref) / mref.quad_bound(case, S)).max()
    print("%s: %s: largest error / bound = %.4f" % (what, case.name, ratio))
    assert ratio <= 1.0, (case.name, ratio)
    return got


# ----------------------------------------------------------------------------- dense k_quadform
# diagonal pairing of M in (1, 15, 16, 17, 63, 64, 65, 130, 131), C in (1, 63, 64, 65, 128, 129, 257), nd in (1, 3, 5), then the
# named extras; with 64 rows per block nrb * nd = 1, 3, 5, 6, 9, 10, 15, 17 work items around the 8-item XCD round
DENSE = [(1, 1, 1), (15, 3, 63), (16, 5, 64), (17, 1, 65), (63, 3, 128), (64, 5, 129), (65, 1, 257), (130, 3, 1), (131, 5, 63),
         (65, 5, 257), (131, 3, 129), (65, 3, 64), (257, 3, 65), (1030, 1, 65)]


@pytest.mark.parametrize("M,nd,C", DENSE)
def test_dense_exact(ctx, M, nd, C):
    """full integer W (no triangle: K starts at 0) and, after weights_update, full upper-triangular integer W (band M - 1 > 16:
    dense with the K loop started at the block's first row); the misaligned view takes the scalar-load fallback, as odd M does"""
    rng = np.random.default_rng([M, nd, C])
    X = mref.int_values(rng, (C, nd, M))
    full = mref.QuadCase("full M=%d nd=%d C=%d" % (M, nd, C), mref.int_dense(rng, nd, M), X)
    wid = _create(ctx, full)
    assert ctx.weights_band(wid) == -1
    _check_exact(ctx, wid, full)
    upper = mref.QuadCase("upper M=%d nd=%d C=%d" % (M, nd, C), mref.int_dense(rng, nd, M, upper=True), X)
    ctx.weights_update(wid, upper.W, np.zeros(nd))
    assert ctx.weights_band(wid) == -1
    _check_exact(ctx, wid, upper)
    ctx.weights_destroy(wid)


def test_dense_exact_on_a_banded_set(ctx, monkeypatch):
    """BEATAMD_QF_BAND=0: a band-5 weight set on the dense kernel (upper_tri set, zeros beyond the band)"""
    rng = np.random.default_rng(50)
    case = mref.QuadCase("band 5 dense", mref.int_banded(rng, 3, 130, (5, 2, 5)), mref.int_values(rng, (65, 3, 130)), band=5)
    wid = _create(ctx, case)
    assert ctx.weights_band(wid) == 5
    banded = _check_exact(ctx, wid, case)
    monkeypatch.setenv("BEATAMD_QF_BAND", "0")
    assert ctx.weights_band(wid) == -1
    dense = _check_exact(ctx, wid, case)
    monkeypatch.delenv("BEATAMD_QF_BAND")
    assert np.array_equal(dense, banded)
    ctx.weights_destroy(wid)


@pytest.mark.parametrize("M", [17, 65, 257])
def test_dense_real_valued(ctx, M):
    case = mref.real_case("dense M=%d" % M)
    wid = _create(ctx, case)
    assert ctx.weights_band(wid) == -1
    got = _check_bound(ctx, wid, case, "k_quadform")
    assert np.array_equal(ctx.wset_quad_batch(wid, _misaligned(case.X)).cpu().numpy(), got)
    ctx.weights_destroy(wid)


# ----------------------------------------------------------------------------- Laplacian path (one shared operator)
@pytest.mark.parametrize("P,nvar,C", [(63, 2, 65), (400, 3, 129), (63, 3, 7), (400, 2, 64)])
def test_laplacian_path_exact_quads(ctx, P, nvar, C):
    """laplacian_logp_batch with h = 0 and logdet = 0 is -0.5 (P log 2 pi + quad_v) summed over v in order: rebuilt from the
    exact integer quads, (nvar + 3) 2^-53 sum |term| for the roundings of P log 2 pi, the terms and their sum"""
    rng = np.random.default_rng([P, nvar, C])
    L = mref.int_dense(rng, 1, P)[0]
    case = mref.QuadCase("laplacian P=%d" % P, L, mref.int_values(rng, (C, nvar, P)), shared=True)
    quad = mref.quad_exact(case).astype(np.float64)
    lid = ctx.laplacian_create(L, 0.0)
    out = ctx.laplacian_logp_batch(lid, case.X, np.zeros(C))
    ctx.laplacian_destroy(lid)
    terms = -0.5 * (P * LOG_2PI + quad)
    ref = np.zeros(C)
    for v in range(nvar):
        ref = ref + terms[:, v]
    tol = (nvar + 3) * U * np.abs(terms).sum(axis=1)
    err = np.abs(out - ref)
    print("laplacian P=%d nvar=%d: largest error / bound = %.4f" % (P, nvar, (err / tol).max()))
    assert (err <= tol).all(), (err / tol).max()


# ----------------------------------------------------------------------------- banded k_quadform_banded<0>
BANDED = [(0, 33, 1), (2, 64, 7), (5, 255, 8), (16, 256, 9), (0, 257, 7), (2, 513, 8), (16, 33, 8), (5, 513, 9), (16, 513, 1),
          (2, 257, 9), (5, 64, 1), (16, 255, 7)]


@pytest.mark.parametrize("band,M,C", BANDED)
def test_banded_exact(ctx, band, M, C):
    """integer band operators with exact zeros outside the band, three datasets, the middle one narrower: the set is evaluated
    on the widest band"""
    rng = np.random.default_rng([band, M, C])
    bands = (band, band // 2 if band != 2 else 0, band)
    case = mref.QuadCase("band %d M=%d C=%d" % (band, M, C), mref.int_banded(rng, 3, M, bands),
                         mref.int_values(rng, (C, 3, M)), band=band)
    assert mref.half_bandwidth(case.W) == band and mref.half_bandwidth(case.W[1:2]) == bands[1]
    wid = _create(ctx, case)
    assert ctx.weights_band(wid) == band
    assert ctx.weights_band_info(wid) == (band, 0.0)
    _check_exact(ctx, wid, case)
    ctx.weights_destroy(wid)


def test_banded_real_valued(ctx):
    case = mref.real_case("band 5 M=257")
    wid = _create(ctx, case)
    assert ctx.weights_band(wid) == 5 and case.K == 6
    _check_bound(ctx, wid, case, "k_quadform_banded")
    ctx.weights_destroy(wid)


# ----------------------------------------------------------------------------- bidiagonal k_quadform_band1
BAND1_M = (33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 575, 576, 577, 1024, 1025)
BAND1 = [(M, 17, 2) for M in BAND1_M] + [(M, C, 1 + (i + j) % 3) for j, M in enumerate((513, 576))
                                         for i, C in enumerate((1, 15, 16, 17, 33))]


@pytest.mark.parametrize("M,C,nd", BAND1)
def test_band1_exact(ctx, M, C, nd):
    """integer (w0, w1) rows; traces that end at a chunk end (512, 1024), one sample later (513, 1025), a tile later (576, 577);
    odd M with nd = 2 leaves dataset 1 misaligned while dataset 0 takes the double2 path; and every case again from the
    misaligned view"""
    rng = np.random.default_rng([M, C, nd])
    case = mref.QuadCase("band 1 M=%d C=%d nd=%d" % (M, C, nd), mref.int_banded(rng, nd, M, (1,) * nd),
                         mref.int_values(rng, (C, nd, M)), band=1)
    wid = _create(ctx, case)
    assert ctx.weights_band(wid) == 1
    _check_exact(ctx, wid, case)
    ctx.weights_destroy(wid)


@pytest.mark.parametrize("M", [65, 513, 1030])
@pytest.mark.parametrize("kind", ["random", "smooth"])
def test_band1_real_valued(ctx, kind, M):
    """the exponential-covariance operator on random residuals and on smooth ones (the cancellation case), K = 2"""
    case = mref.real_case("band 1 %s M=%d" % (kind, M))
    wid = _create(ctx, case)
    assert ctx.weights_band(wid) == 1 and case.K == 2
    got = _check_bound(ctx, wid, case, "k_quadform_band1")
    assert np.array_equal(ctx.wset_quad_batch(wid, _misaligned(case.X)).cpu().numpy(), got)
    ctx.weights_destroy(wid)


# ----------------------------------------------------------------------------- scalar k_scalar_quad
@pytest.mark.parametrize("M", [1, 63, 64, 65, 200])
def test_scalar_exact(ctx, M):
    """integer residuals and power-of-two weights: (w x)^2 summed in any order is exact"""
    rng = np.random.default_rng(M)
    case = mref.QuadCase("scalar M=%d" % M, 2.0 ** np.array([-3.0, 0.0, 2.0]), mref.int_values(rng, (5, 3, M)), scalar=True)
    wid = _create(ctx, case)
    _check_exact(ctx, wid, case)
    ctx.weights_update(wid, 2.0 ** np.array([1.0, -2.0, 3.0]), np.zeros(3))
    _check_exact(ctx, wid, mref.QuadCase(case.name + " updated", 2.0 ** np.array([1.0, -2.0, 3.0]), case.X, scalar=True))
    ctx.weights_destroy(wid)


# ----------------------------------------------------------------------------- batch independence
def _independence_cases():
    rng = np.random.default_rng(130)
    yield ("dense", mref.QuadCase("dense", rng.standard_normal((2, 65, 65)), rng.standard_normal((130, 2, 65))), -1,
           [(60, 70), (120, 130), (64, 128)])
    yield ("band1", mref.QuadCase("band1", np.stack([mref.exponential_bidiagonal(513, scale=0.3 + d) for d in range(2)]),
                                  rng.standard_normal((35, 2, 513)), band=1), 1, [(10, 20), (16, 33)])
    yield ("banded", mref.QuadCase("banded", mref.unpack_band(rng.standard_normal((2, 257, 6))),
                                   rng.standard_normal((35, 2, 257)), band=5), 5, [(5, 12), (8, 17)])
    yield ("scalar", mref.QuadCase("scalar", np.array([0.7, 1.9]), rng.standard_normal((35, 2, 200)), scalar=True), None,
           [(2, 7), (3, 5)])


@pytest.mark.parametrize("family", ["dense", "band1", "banded", "scalar"])
def test_chain_value_is_independent_of_the_batch(ctx, family):
    """real-valued inputs; the first chain alone, the last chain alone and slices across a block edge (64 / 128 chains dense,
    16 bidiagonal, 8 banded, 4 scalar) give the bits they have in the whole batch: ranks that split a population compute
    identical values"""
    name, case, band, slices = [c for c in _independence_cases() if c[0] == family][0]
    wid = _create(ctx, case)
    if band is not None:
        assert ctx.weights_band(wid) == band
    whole = ctx.wset_quad_batch(wid, case.X)
    assert np.array_equal(whole, ctx.wset_quad_batch(wid, case.X))
    for lo, hi in [(0, 1), (case.C - 1, case.C)] + slices:
        part = ctx.wset_quad_batch(wid, case.X[lo:hi])
        assert np.array_equal(part, whole[lo:hi]), "%s: chains %d:%d differ from the batch of %d" % (name, lo, hi, case.C)
    ctx.weights_destroy(wid)


# ----------------------------------------------------------------------------- band detection
def _bidiagonal(rng, nd, M):
    return mref.int_banded(rng, nd, M, (1,) * nd)


def test_band_detection_sizes_and_limits(ctx):
    rng = np.random.default_rng(32)
    for M, want in ((32, -1), (33, 1)):
        case = mref.QuadCase("bidiagonal M=%d" % M, _bidiagonal(rng, 2, M), mref.int_values(rng, (9, 2, M)), band=1)
        wid = _create(ctx, case)
        assert ctx.weights_band(wid) == want, (M, ctx.weights_band(wid))
        _check_exact(ctx, wid, case)
        ctx.weights_destroy(wid)
    for band, want in ((16, 16), (17, -1)):
        case = mref.QuadCase("band %d" % band, mref.int_banded(rng, 2, 64, (band, 3)), mref.int_values(rng, (9, 2, 64)), band=band)
        wid = _create(ctx, case)
        assert ctx.weights_band_info(wid) == (want, 0.0)
        _check_exact(ctx, wid, case)            # (band 17: the dense kernel, the same exact value)
        ctx.weights_destroy(wid)


@pytest.mark.parametrize("band,M", [(5, 40), (16, 33), (16, 257)])
def test_band_entry_only_in_the_last_row_that_holds_it(ctx, band, M):
    rng = np.random.default_rng([band, M])
    W = mref.int_banded(rng, 2, M, (0, 0))
    W[1, M - 1 - band, M - 1] = 5.0
    case = mref.QuadCase("corner band %d M=%d" % (band, M), W, mref.int_values(rng, (9, 2, M)), band=band)
    wid = _create(ctx, case)
    assert ctx.weights_band(wid) == band
    _check_exact(ctx, wid, case)
    ctx.weights_destroy(wid)


def test_band_detection_zero_row_and_negative_zero(ctx):
    rng = np.random.default_rng(7)
    M = 65
    W = _bidiagonal(rng, 2, M)
    W[0, 7, :] = 0.0                                   # a row of all zeros: its maximum is 0, nothing exceeds it
    W[1, M - 1, :] = 0.0
    case = mref.QuadCase("zero rows", W, mref.int_values(rng, (9, 2, M)), band=1)
    wid = _create(ctx, case)
    assert ctx.weights_band_info(wid) == (1, 0.0)
    _check_exact(ctx, wid, case)
    Wz = W.copy()
    Wz[1, 5, 2] = -0.0                                 # -0.0 below the diagonal: still triangular
    Wz[0, M - 1, 0] = -0.0
    ctx.weights_update(wid, Wz, np.zeros(2))
    assert ctx.weights_band(wid) == 1
    _check_exact(ctx, wid, case)
    ctx.weights_destroy(wid)


def test_band_threshold_is_strict_at_2_to_the_minus_40(ctx):
    """an entry of exactly 2^-40 of its row's largest (a power of two, so the product is exact) at distance 20 is dropped and
    reported; one ulp more and the set is dense"""
    rng = np.random.default_rng(40)
    M = 65
    W = _bidiagonal(rng, 2, M)
    W[1, 3, 3], W[1, 3, 4] = -4.0, 3.0                 # row maximum 4
    wid = ctx.weights_create_dense(W, np.zeros(2))
    assert ctx.weights_band_info(wid) == (1, 0.0)
    W[1, 3, 23] = 2.0 ** -40 * 4.0
    ctx.weights_update(wid, W, np.zeros(2))
    assert ctx.weights_band_info(wid) == (1, 2.0 ** -40)
    W[1, 3, 23] = 2.0 ** -40 * 4.0 * (1.0 + 2.0 ** -52)
    ctx.weights_update(wid, W, np.zeros(2))
    assert ctx.weights_band_info(wid) == (-1, 0.0)
    W[1, 3, 23] = -(2.0 ** -40) * 4.0                  # the sign does not matter
    ctx.weights_update(wid, W, np.zeros(2))
    assert ctx.weights_band_info(wid) == (1, 2.0 ** -40)
    ctx.weights_destroy(wid)


# ----------------------------------------------------------------------------- k_geo_stack
def _geo_library(ctx, G):
    from beat_amd.ffi import GeodeticGFLibrary
    lib = GeodeticGFLibrary()
    lib.setup(G.shape[0], G.shape[1], allocate=True)
    lib.put(G, np.arange(G.shape[0]))
    lib.init_optimization(ctx)
    return lib


# diagonal pairing of P in (1, 15, 16, 17, 31, 32, 33, 48, 400), Nobs in (1, 127, 128, 129, 300), C in (1, 63, 64, 65, 67) (the
# chain list shifted by two so that Nobs and C do not move together), then the named extras
GEO = [(1, 1, 64), (15, 127, 65), (16, 128, 67), (17, 129, 1), (31, 300, 63), (32, 1, 64), (33, 127, 65), (48, 128, 67),
       (400, 129, 1), (33, 129, 67), (400, 300, 65), (2048, 3, 64), (2049, 3, 64), (8192, 3, 2)]


@pytest.mark.parametrize("P,Nobs,C", GEO)
def test_geo_stack_exact(ctx, P, Nobs, C):
    """integer G and slips, with and without out= (accumulate onto an integer mu): fewer than 16 patches, one / two / three
    full groups of the prefetch with and without a tail, the 4-chain tile from 64 chains on; P = 2048 is the last size whose
    four chains fit 64 KiB (4-chain tile), P = 2049 the first on the 1-chain tile, P = 8192 the largest accepted"""
    rng = np.random.default_rng([P, Nobs, C])
    G, s = mref.int_values(rng, (P, Nobs)), mref.int_values(rng, (C, P))
    lib = _geo_library(ctx, G)
    mu = lib.stack_all_batch(s)
    assert mu.shape == (C, Nobs) and np.array_equal(mu, mref.geo_exact(G, s))
    mu0 = mref.int_values(rng, (C, Nobs))
    out = mu0.copy()
    res = lib.stack_all_batch(s, out=out)
    assert res is out and np.array_equal(out, mref.geo_exact(G, s, mu0))
    ctx.geo_gflib_destroy(lib.lib_id)


def test_geo_stack_refuses_more_than_8192_patches(ctx):
    rng = np.random.default_rng(8193)
    G, s = mref.int_values(rng, (8193, 3)), mref.int_values(rng, (2, 8193))
    lib = _geo_library(ctx, G)
    with pytest.raises(ValueError):
        lib.stack_all_batch(s)
    ctx.geo_gflib_destroy(lib.lib_id)
    lib = _geo_library(ctx, G[:8192])                  # the context goes on working
    assert np.array_equal(lib.stack_all_batch(s[:, :8192]), mref.geo_exact(G[:8192], s[:, :8192]))
    ctx.geo_gflib_destroy(lib.lib_id)


def test_geo_stack_real_valued_and_tiles_agree_bitwise(ctx):
    """P = 400, Nobs = 129: the batch of 67 (4-chain tile) within the bound, and its chains 0:63 bit-equal to the same chains as
    a batch of 63 (1-chain tile) -- the kernel's claim that both tiles run the same fma sequence"""
    G, s = mref.geo_real_case()
    ref, bound = mref.geo_ref(G, s)
    lib = _geo_library(ctx, G)
    mu = lib.stack_all_batch(s)
    ratio = (mref.hp_error(mu, ref) / bound).max()
    print("k_geo_stack: largest error / bound = %.4f" % ratio)
    assert ratio <= 1.0
    assert np.array_equal(lib.stack_all_batch(s[:63]), mu[:63])
    assert np.array_equal(lib.stack_all_batch(s[66:67]), mu[66:67])
    ctx.geo_gflib_destroy(lib.lib_id)
