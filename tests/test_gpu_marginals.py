"""The posterior marginals on the GPU (beat_amd/marginals.py, csrc/marginals.hip).  Exact results (sorted columns,
percentiles, counts, edges, densities) are compared with numpy directly -- the restatement of the kernels,
tests/marginals_ref.py, is pinned to numpy by tests/test_marginals_host.py --; the two density sums with 50-digit values
(tests/golden/marginals.npz), scipy and the restatement.  Every test prints the figures it asserts on."""
import warnings

import numpy as np
import pytest

import marginals_ref as ref
from conftest import load_golden

pytestmark = pytest.mark.gpu

T = 16384                     # csrc/kernels.hpp MG_SORT_TILE
NS = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, T - 1, T, T + 1, 3 * T + 1]
Q8 = [0, 0.01, 5, 50, 68, 95, 99.99, 100]


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.fixture(scope="module")
def gold():
    return load_golden("marginals")


def _side(X, side):
    if side == "numpy":
        return X
    import torch
    return torch.from_numpy(np.ascontiguousarray(X)).cuda()


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _population(n, variant):
    """(n, 5): A = random, sorted, reversed, all equal, many ties; B = both signed zeros, 1e-300, 1e300, ties, random"""
    rng = np.random.default_rng(1000 * n + len(variant))
    z = rng.standard_normal((n, 5))
    if variant == "A":
        z[:, 1] = np.sort(z[:, 1])
        z[:, 2] = np.sort(z[:, 2])[::-1]
        z[:, 3] = 2.5
        z[:, 4] = np.round(z[:, 4], 1)
    else:
        z[:, 0] = np.where(z[:, 0] > 0.5, z[:, 0], np.where(z[:, 0] > 0, 0.0, -0.0)) * np.sign(z[:, 1])
        z[:, 1] *= 1e-300
        z[:, 2] *= 1e300
        z[:, 3] = np.round(z[:, 3], 1)
    return z


# ------------------------------------------------------------------------------------------------ columns
@pytest.mark.parametrize("side", ["numpy", "torch"])
@pytest.mark.parametrize("variant", ["A", "B"])
@pytest.mark.parametrize("n", NS)
def test_sort_percentiles_histograms_are_numpys(ctx, n, variant, side):
    from beat_amd import marginals as m
    X = _population(n, variant)
    for cols in (None, [3, 0, 3, 1]):       # all; permuted, repeated, a strict subset
        D = X if cols is None else X[:, cols]
        Xs = _side(X, side)
        h = m.sort_columns(Xs, cols)
        assert (h.K, h.n) == (D.shape[1], n)
        assert np.array_equal(_np(h.sorted), np.sort(D, axis=0).T)
        want = np.percentile(D, Q8, axis=0).T
        got = m.percentiles(h, Q8)
        assert isinstance(got, np.ndarray) == (side == "numpy")
        assert np.array_equal(_np(got), want)
        assert np.array_equal(_np(m.percentiles(Xs, Q8, cols)), want)       # the handle equals passing X
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            edge_sets = []
            for qlist in ([0.01, 99.99], None):
                e = _np(m.make_bins(h, 40, qlist))
                lo, hi = (np.percentile(D, qlist, axis=0) if qlist else (D.min(axis=0), D.max(axis=0)))
                assert np.array_equal(e, np.array([np.linspace(lo[k], hi[k], 40) for k in range(D.shape[1])]))
                assert np.array_equal(e, _np(m.make_bins(Xs, 40, qlist, cols)))
                edge_sets.append(e)
            q25, q75 = np.percentile(D, [25, 75], axis=0)
            edge_sets.append(np.array([np.linspace(q25[k], q75[k], 12) for k in range(D.shape[1])]))   # samples outside
            for e in edge_sets:
                for cumulative in (False, True):
                    c, e2, hts = m.histograms(h, edges=e, cumulative=cumulative)
                    assert _np(c).dtype == np.int64 and np.array_equal(_np(e2), e)
                    for k in range(D.shape[1]):
                        cn = np.histogram(D[:, k], bins=e[k])[0]
                        assert np.array_equal(_np(c)[k], cn), (n, variant, k)
                        dn = np.histogram(D[:, k], bins=e[k], density=True)[0]
                        np.testing.assert_array_equal(_np(hts)[k], (dn * np.diff(e[k])).cumsum() if cumulative else dn)
            for bins in (1, 10, 40):
                try:
                    [np.histogram(D[:, k], bins=bins) for k in range(D.shape[1])]
                except ValueError:      # numpy cannot make the bins (one sample of size 1e300 +- 0.5): the same error here
                    with pytest.raises(ValueError, match="Too many bins"):
                        m.histograms(h, bins=bins)
                    continue
                c, e, hts = m.histograms(h, bins=bins)
                c2 = m.histograms(Xs, bins=bins, cols=cols)[0]
                for k in range(D.shape[1]):
                    cn, en = np.histogram(D[:, k], bins=bins)
                    assert np.array_equal(_np(e)[k], en) and np.array_equal(_np(c)[k], cn), (n, variant, bins, k)
                    np.testing.assert_array_equal(_np(hts)[k], np.histogram(D[:, k], bins=bins, density=True)[0])
                assert np.array_equal(_np(c), _np(c2))


@pytest.mark.parametrize("side", ["numpy", "torch"])
def test_nonfinite_sample_names_its_column(ctx, side):
    from beat_amd import marginals as m
    rng = np.random.default_rng(5)
    X = rng.standard_normal((1025, 5))
    bad = X.copy()
    bad[1000, 2] = np.nan
    with pytest.raises(ValueError, match="column 2 "):
        m.percentiles(_side(bad, side), [50])
    bad = X.copy()
    bad[3, 4] = np.inf
    with pytest.raises(ValueError, match="column 4 "):
        m.sort_columns(_side(bad, side), cols=[4, 1])
    with pytest.raises(ValueError, match="column 4 "):
        m.kde2d(_side(bad, side), [[1, 4]], grid=5)
    with pytest.raises(ValueError, match="column 4 "):
        m.hist2d(_side(bad, side), [[0, 1], [4, 0]], bins=(3, 3))
    assert np.array_equal(_np(m.percentiles(_side(bad, side), [50], cols=[0, 1])), np.percentile(X[:, :2], [50], axis=0).T)
    assert np.array_equal(_np(m.percentiles(_side(X, side), [50])), np.percentile(X, [50], axis=0).T)


# ------------------------------------------------------------------------------------------------ hist2d
def _rounded(n, V=10, seed=0):
    rng = np.random.default_rng(77 + n + seed)
    return np.round(rng.standard_normal((n, V)) * np.linspace(0.5, 3.0, V), 1)


@pytest.mark.parametrize("side", ["numpy", "torch"])
@pytest.mark.parametrize("n", [1, 65, 1000, 4097])
def test_hist2d_is_numpys(ctx, n, side):
    from beat_amd import marginals as m
    X = _rounded(n)
    Xs = _side(X, side)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for pairs in ([[3, 1]], [[0, 1], [2, 2], [1, 0]], m.correlation_pairs(range(10)).tolist()):
            for bins in ((1, 40), (7, 40), (40, 40), (128, 128)):
                c, ex, ey, dens = m.hist2d(Xs, pairs, bins=bins)
                assert _np(c).dtype == np.int64 and _np(c).shape == (len(pairs),) + bins
                for p, (i, j) in enumerate(pairs):
                    H, exn, eyn = np.histogram2d(X[:, i], X[:, j], bins=bins)
                    assert np.array_equal(_np(c)[p], H.astype(np.int64)), (n, bins, i, j)
                    assert np.array_equal(_np(ex)[p], exn) and np.array_equal(_np(ey)[p], eyn)
                    np.testing.assert_array_equal(_np(dens)[p], np.histogram2d(X[:, i], X[:, j], bins=bins, density=True)[0])
        for i, j in ((0, 9), (4, 4), (7, 2)):       # bins=(None, None): hist_binning of each column's range
            c, ex, ey, dens = m.hist2d(Xs, [[i, j]])
            bins = (m.hist_binning(X[:, i].min(), X[:, i].max()), m.hist_binning(X[:, j].min(), X[:, j].max()))
            H, exn, eyn = np.histogram2d(X[:, i], X[:, j], bins=bins)
            assert np.array_equal(_np(c)[0], H.astype(np.int64)) and np.array_equal(_np(ex)[0], exn)
        pairs = m.correlation_pairs(range(10))
        whole = _np(m.hist2d(Xs, pairs, bins=(40, 40))[0])
        parts = np.concatenate([_np(m.hist2d(Xs, pairs[:1], bins=(40, 40))[0]), _np(m.hist2d(Xs, pairs[1:], bins=(40, 40))[0])])
        assert np.array_equal(whole, parts)


# ------------------------------------------------------------------------------------------------ kde2d
def _scipy_kde(x, y, gx, gy):
    from scipy import stats
    G = np.meshgrid(np.linspace(x.min(), x.max(), gx), np.linspace(y.min(), y.max(), gy), indexing="ij")
    return stats.gaussian_kde(np.vstack([x, y]))(np.vstack([G[0].ravel(), G[1].ravel()])).reshape(gx, gy)


def test_kde2d_against_50_digit_values(ctx, gold):
    """within 16 x scipy's own distance on the same case, floor 8, in units of 2^-53 max Z.  Observed on an MI355X: 2.5 to
    10.3 units where scipy has 2.8 to 16.6; 47 to 53 at rho = -0.999 (scipy 11.6 to 91.5); the table is in DESIGN 3.12"""
    from beat_amd import marginals as m
    worst = []
    for k in range(int(gold["kde_n"])):
        x, y, Zmp = gold["kde%d_x" % k], gold["kde%d_y" % k], gold["kde%d_Zmp" % k]
        Z, ext, pairs = m.kde2d(np.stack([x, y], axis=1), [[0, 1]], grid=Zmp.shape)
        assert np.array_equal(ext[0], [x.min(), x.max(), y.min(), y.max()])
        units = np.abs(Z[0] - Zmp).max() / (2.0 ** -53 * Zmp.max())
        scipy_units = float(gold["kde%d_scipy_units" % k])
        print("kde2d case %d n=%d: device %.1f units, scipy %.1f units" % (k, x.size, units, scipy_units))
        worst.append((units, max(16.0 * scipy_units, 8.0), k))
        # the reference's own kde2plot_op on its square grid
        Zr = gold["kde%d_Z" % k]
        Z2 = m.kde2d(np.stack([x, y], axis=1), [[0, 1]], grid=Zr.shape[0])[0][0]
        assert np.abs(Z2 - Zr).max() <= 1e-9 * Zr.max()
    for units, bound, k in worst:
        assert units <= bound, (k, units, bound)


KDE_CASES = [(3, (9, 7), 0.3), (63, (1, 1), 0.0), (64, (2, 3), 0.999), (65, (9, 7), -0.999), (257, (64, 64), 0.999),
             (257, (65, 33), -0.999), (4097, (65, 33), 0.3), (4097, (64, 64), -0.999), (4097, (200, 200), 0.9)]


@pytest.mark.parametrize("n,grid,rho", KDE_CASES)
def test_kde2d_against_scipy(ctx, n, grid, rho):
    from beat_amd import marginals as m
    rng = np.random.default_rng(n + grid[0])
    z = rng.standard_normal((2, n))
    X = np.stack([1e5 * (3.0 + z[0]), 1e-6 * (-3.0 + rho * z[0] + np.sqrt(1 - rho * rho) * z[1]), z[1]], axis=1)
    side = "torch" if n % 2 else "numpy"
    Z = _np(m.kde2d(_side(X, side), [[0, 1]], grid=grid)[0])[0]
    Zs = _scipy_kde(X[:, 0], X[:, 1], *grid)
    err = np.abs(Z - Zs).max() / Zs.max()
    print("kde2d n=%d grid=%s rho=%g: %.2e of max Z from scipy" % (n, grid, rho, err))
    assert Z.shape == grid and err <= 1e-9


def test_kde2d_bits_do_not_depend_on_the_call(ctx):
    from beat_amd import marginals as m
    import torch
    rng = np.random.default_rng(9)
    X = rng.standard_normal((1500, 10)) * np.linspace(1e-3, 1e3, 10) + np.arange(10)
    Xd = torch.from_numpy(X).cuda()
    pairs = m.correlation_pairs(range(10))
    Z, ext, p = m.kde2d(Xd, pairs, grid=(33, 65))
    assert np.array_equal(p, pairs) and Z.shape == (45, 33, 65)
    Z1, Z44 = m.kde2d(Xd, pairs[:1], grid=(33, 65))[0], m.kde2d(Xd, pairs[1:], grid=(33, 65))[0]
    assert torch.equal(Z, torch.cat([Z1, Z44]))
    Zc, extc, pc = m.correlation_kdes(Xd, range(10), grid=(33, 65))
    assert torch.equal(Z, Zc) and torch.equal(ext, extc) and np.array_equal(pc, pairs)
    Zh = m.kde2d(X, pairs[[0, 17, 44]], grid=(33, 65))[0]        # host input: only the used columns go up
    assert np.array_equal(Zh, Z[[0, 17, 44]].cpu().numpy())
    for shape in ("wide", "narrow"):                             # every launch shape on offer, many pairs and one
        assert torch.equal(Z, m.kde2d(Xd, pairs, grid=(33, 65), shape=shape)[0])
        assert torch.equal(Z1, m.kde2d(Xd, pairs[:1], grid=(33, 65), shape=shape)[0])
        assert torch.equal(Z, m.kde2d(Xd, pairs, grid=(33, 65), shape=shape, skip_blocks=False)[0])


def test_kde2d_block_skip_changes_no_bit(ctx):
    """a sharply peaked column, in ascending order so that whole blocks of samples lie > 38.6 bandwidths (arg / 2 > 745.2)
    from whole tiles of the grid: their terms are exact zeros"""
    from beat_amd import marginals as m
    rng = np.random.default_rng(10)
    x = np.sort(np.concatenate([rng.normal(0.0, 1e-5, 4087), rng.uniform(-1.0, 1.0, 10)]))
    assert (x.max() - x.min()) / (x.std(ddof=1) * x.size ** (-1.0 / 6.0)) > 4 * 38.7 + 40      # four tiles of the grid
    X = np.stack([x, rng.standard_normal(4097)], axis=1)
    Zs = m.kde2d(X, [[0, 1], [1, 0]], grid=(64, 64), skip_blocks=True)[0]
    Zn = m.kde2d(X, [[0, 1], [1, 0]], grid=(64, 64), skip_blocks=False)[0]
    assert np.array_equal(Zs, Zn) and np.isfinite(Zs).all()
    for shape in ("wide", "narrow"):
        assert np.array_equal(Zs, m.kde2d(X, [[0, 1], [1, 0]], grid=(64, 64), shape=shape)[0])
    assert np.abs(Zs[0] - _scipy_kde(X[:, 0], X[:, 1], 64, 64)).max() <= 1e-9 * Zs[0].max()


def test_kde2d_singular_pairs_are_flagged_one_by_one(ctx):
    from beat_amd import marginals as m
    rng = np.random.default_rng(11)
    X = rng.standard_normal((300, 4))
    X[:, 2] = 7.0
    pairs = np.array([[0, 1], [0, 2], [1, 1], [3, 0], [2, 3]])
    with pytest.raises(np.linalg.LinAlgError) as ei:
        m.kde2d(X, pairs, grid=(9, 7))
    e = ei.value
    assert "[(0, 2), (1, 1), (2, 3)]" in str(e) and e.flags.tolist() == [0, 1, 1, 0, 1]
    good = m.kde2d(X, pairs[[0, 3]], grid=(9, 7))[0]
    assert np.array_equal(e.Z[[0, 3]], good) and np.isnan(e.Z[[1, 2, 4]]).all()
    with pytest.raises(np.linalg.LinAlgError, match=r"\[\(0, 1\), \(3, 0\)\]"):
        m.kde2d(X[:2], pairs[[0, 3]], grid=(9, 7))           # n = 2 is singular in scipy too
    assert np.array_equal(m.kde2d(X, pairs[[0, 3]], grid=(9, 7))[0], good)


# ------------------------------------------------------------------------------------------------ spherical
def _sph_units(got, want, sigma):
    return np.abs(got - want).max() / ((1.0 + 1.0 / sigma ** 2) * 2.0 ** -53 * want.max())


def test_spherical_kde_against_50_digit_values_and_the_reference(ctx, gold):
    """within 8 units of (1 + 1/sigma^2) 2^-53 max of the 50-digit values and of the reference's arrays.  Observed on an
    MI355X: 0.65, 0.24, 0.97, 0.30 from the 50-digit values (the reference itself 0.54, 0.49, 0.85, 0.30) and 0.12, 0.24,
    0.24, 0.00 from the reference's arrays"""
    from beat_amd import marginals as m
    lats, lons = gold["sph_lats"], gold["sph_lons"]
    figures = []
    for k in range(int(gold["sph_n"])):
        key = "sph%d" % k
        lats0, lons0, sigma = gold[key + "_lats0"], gold[key + "_lons0"], float(gold[key + "_sigma"])
        kde, la, lo = m.spherical_kde(lats0, lons0, lats=lats, lons=lons, grid_size=lats.shape, sigma=sigma)
        assert kde.shape == lats.shape and la is lats and lo is lons
        u_mp, u_ref = _sph_units(kde, gold[key + "_kdemp"], sigma), _sph_units(kde, gold[key + "_kde"], sigma)
        print("spherical case %d n=%d sigma=%g: device %.2f units from 50 digits, %.2f from the reference (the reference "
              "itself %.2f)" % (k, lats0.size, sigma, u_mp, u_ref, float(gold[key + "_ref_units"])))
        figures.append((k, u_mp, u_ref))
        if lats0.size > 1:
            got = m.vonmises_std(lons=lons0, lats=lats0)
            np.testing.assert_allclose(got, float(gold[key + "_sigmahat"]), rtol=1e-12)
            auto = m.spherical_kde(lats0, lons0, lats=lats, lons=lons, grid_size=lats.shape)[0]
            s = 1.06 * got * lats0.size ** -0.2
            assert np.array_equal(auto, m.spherical_kde(lats0, lons0, lats=lats, lons=lons, grid_size=lats.shape, sigma=s)[0])
    for k, u_mp, u_ref in figures:
        assert u_mp <= 8.0 and u_ref <= 8.0, (k, u_mp, u_ref)


@pytest.mark.parametrize("n", [1, 499, 500, 501])
def test_spherical_kde_chunk_edges(ctx, n):
    from beat_amd import marginals as m
    import torch
    rng = np.random.default_rng(n)
    lats0, lons0 = rng.normal(-30.0, 10.0, n), rng.normal(170.0, 15.0, n)     # longitudes across the date line
    lons, lats = np.meshgrid(np.linspace(-180.0, 180, 9), np.linspace(-90.0, 90, 8))
    want = ref.spherical_kde(lats0, lons0, lats, lons, 0.2)
    got = m.spherical_kde(lats0, lons0, grid_size=(8, 9), sigma=0.2)
    assert np.array_equal(got[1], lats) and np.array_equal(got[2], lons)
    units = _sph_units(got[0], want, 0.2)
    print("spherical n=%d: %.2f units from the restatement" % (n, units))
    assert units <= 8.0
    dev = m.spherical_kde(torch.from_numpy(lats0).cuda(), torch.from_numpy(lons0).cuda(), grid_size=(8, 9), sigma=0.2)[0]
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got[0])
    for shape in ("wide", "narrow"):
        assert np.array_equal(m.spherical_kde(lats0, lons0, grid_size=(8, 9), sigma=0.2, shape=shape)[0], got[0])


def test_spherical_kde_default_grid_and_lune(ctx):
    from beat_amd import marginals as m
    from beat_amd.sources import v_to_gamma, w_to_delta
    rng = np.random.default_rng(12)
    lats0, lons0 = rng.normal(40.0, 5.0, 65), rng.normal(-100.0, 9.0, 65)
    kde, lats, lons = m.spherical_kde(lats0, lons0, sigma=0.1)
    assert kde.shape == lats.shape == lons.shape == (200, 200) and lats[0, 0] == -90.0 and lons[0, -1] == 180.0
    units = _sph_units(kde, ref.spherical_kde(lats0, lons0, lats, lons, 0.1), 0.1)
    print("spherical 200 x 200: %.2f units from the restatement" % units)
    assert units <= 8.0
    # MTQT draws: v in [-1/3, 1/3], w in [-3 pi / 8, 3 pi / 8]
    v, w = rng.uniform(-0.3, 0.3, 300), rng.uniform(-1.0, 1.0, 300)
    kde, lats, lons = m.lune_kde(v, w, grid_size=(40, 30))
    gamma, delta = np.rad2deg(v_to_gamma(v)), np.rad2deg(w_to_delta(w))
    assert lats[0, 0] == -90.0 and lats[-1, 0] == 90.0 and lons[0, 0] == -30.0 and lons[0, -1] == 30.0
    sigma = 1.06 * ref.vonmises_std(lons=gamma, lats=delta) * 300 ** -0.2
    units = _sph_units(kde, ref.spherical_kde(delta, gamma, lats, lons, sigma), sigma)
    print("lune_kde: sigma %.4f, %.2f units from the restatement" % (sigma, units))
    assert units <= 8.0
    with pytest.raises(ValueError, match="jitter"):
        m.lune_kde(np.full(300, 0.1) + 1e-6 * rng.standard_normal(300), w)


# ------------------------------------------------------------------------------------------------ end to end
def test_marginals_of_a_sampled_population(ctx):
    """a 256-chain SMC run on the synthetic problem of smoke(); its final population, on the device, through percentiles,
    make_bins, histograms and correlation_kdes for four variables"""
    import torch
    from beat_amd import marginals as m
    from beat_amd.sampler import SMC, smc_sample
    from beat_amd.synthetic import SyntheticSpec, build_problem
    spec = SyntheticSpec((6,), (5,), (1.0,), T=4, N=128, D=3, S=25, covariance="toeplitz", station_shifts=True,
                         geodetic_nobs=(12,), laplacian=True)
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    lo, up = host["layout"].bounds(host["lower"], host["upper"])
    step = SMC(f, lo, up, n_chains=256, device=torch.device("cuda", 0), random_seed=3)
    # (stopped after three tempering stages: pushed on to beta = 1 in so few steps, the resampling would leave copies of one
    # chain, whose marginals are points)
    pop, lp, betas = smc_sample(5, step, max_stages=3, final_stage=False)
    assert pop.shape == (256, lo.size)
    cols = np.sort(np.argsort(pop.std(axis=0))[-4:])
    print("end to end: betas %s, columns %s, distinct values %s" % (betas, cols, [np.unique(pop[:, c]).size for c in cols]))
    Xd = torch.from_numpy(np.ascontiguousarray(pop)).cuda()
    h = m.sort_columns(Xd, cols)
    D = pop[:, cols]
    assert np.array_equal(m.percentiles(h, [0.01, 5, 68, 95, 99.99]).cpu().numpy(),
                          np.percentile(D, [0.01, 5, 68, 95, 99.99], axis=0).T)
    e = m.make_bins(h, 40, [0.01, 99.99])
    c, e2, hts = m.histograms(h, edges=e)
    for k in range(4):
        assert np.array_equal(c[k].cpu().numpy(), np.histogram(D[:, k], bins=e[k].cpu().numpy())[0])
    Z, ext, pairs = m.correlation_kdes(Xd, cols, grid=50)
    assert Z.shape == (6, 50, 50) and Z.is_cuda
    for p, (i, j) in enumerate(pairs):
        Zs = _scipy_kde(pop[:, i], pop[:, j], 50, 50)
        err = np.abs(Z[p].cpu().numpy() - Zs).max() / Zs.max()
        print("end to end pair (%d, %d): %.2e of max Z from scipy" % (i, j, err))
        assert err <= 1e-9
