"""CPU tests of the posterior marginals (beat_amd/marginals.py, csrc/marginals.hip): the numpy restatement of the kernels
(tests/marginals_ref.py) is pinned to numpy / scipy and to the reference's own functions (tests/golden/marginals.npz,
tools/gen_golden_marginals.py); the host functions, the argument rules, the prototypes and the kernels' resources."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import marginals_ref as ref
from conftest import ROOT, load_golden

Q8 = [0, 0.01, 5, 50, 68, 95, 99.99, 100]


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def gold():
    return load_golden("marginals")


# ------------------------------------------------------------------------------------------------ restatement vs numpy
def test_percentile_restatement_is_numpy():
    rng = np.random.default_rng(1)
    for trial in range(160):
        n = int(rng.choice([1, 2, 3, 63, 64, 65, 1023, 1025, 4097]))
        X = rng.standard_normal((n, 2)) * 10.0 ** rng.integers(-6, 7)
        if trial % 3 == 0:
            X = np.round(X, 1)
        S = ref.sort_columns(X)
        assert np.array_equal(ref.percentiles(S, Q8), np.percentile(X, Q8, axis=0).T)


def test_histogram_restatement_is_numpy():
    rng = np.random.default_rng(2)
    for trial in range(120):
        n = int(rng.choice([1, 2, 65, 1000, 4097]))
        d = np.round(rng.normal(0.0, 2.0, n), 1)
        S = np.sort(d)[None, :]
        for bins in (1, 10, 40):
            e = ref.outer_edges(d.min(), d.max(), bins)
            cn, en = np.histogram(d, bins=bins)
            assert np.array_equal(e, en) and np.array_equal(ref.hist_counts(S, e[None, :])[0], cn)
        e = np.linspace(-1.0, 1.5, 12)      # samples outside on both sides, rounded samples on edges
        assert np.array_equal(ref.hist_counts(S, e[None, :])[0], np.histogram(d, bins=e)[0])


def test_hist2d_restatement_is_numpy():
    rng = np.random.default_rng(3)
    for n in (1, 65, 1000, 4097):
        x, y = np.round(rng.normal(0, 1, n), 1), np.round(rng.normal(5, 3, n), 0)
        for bx, by in ((1, 40), (7, 40), (40, 40), (128, 128)):
            ex, ey = ref.outer_edges(x.min(), x.max(), bx), ref.outer_edges(y.min(), y.max(), by)
            H, ex_n, ey_n = np.histogram2d(x, y, bins=(bx, by))
            assert np.array_equal(ex, ex_n) and np.array_equal(ey, ey_n)
            assert np.array_equal(ref.hist2d_counts(x, y, ex, ey), H.astype(np.int64))


def test_densities_are_numpys():
    from beat_amd import marginals as m
    rng = np.random.default_rng(4)
    d = np.round(rng.normal(0, 1, (1000, 2)), 1)
    for bins in (1, 10, 40):
        e = np.array([ref.outer_edges(d[:, k].min(), d[:, k].max(), bins) for k in range(2)])
        c = ref.hist_counts(ref.sort_columns(d), e)
        h = m.histogram_heights(c, e)
        for k in range(2):
            assert np.array_equal(h[k], np.histogram(d[:, k], bins=bins, density=True)[0])
    ex, ey = ref.outer_edges(d[:, 0].min(), d[:, 0].max(), 7), ref.outer_edges(d[:, 1].min(), d[:, 1].max(), 40)
    c = ref.hist2d_counts(d[:, 0], d[:, 1], ex, ey)
    assert np.array_equal(m.hist2d_density(c[None], ex[None], ey[None])[0],
                          np.histogram2d(d[:, 0], d[:, 1], bins=(7, 40), density=True)[0])


def test_cumulative_heights_are_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from beat_amd import marginals as m
    rng = np.random.default_rng(5)
    d = np.round(rng.normal(0, 1, 1000), 1)
    fig, ax = plt.subplots()
    for cumulative in (False, True):
        n, edges, _ = ax.hist(d, bins=37, density=True, cumulative=cumulative)
        c = ref.hist_counts(np.sort(d)[None], edges[None])
        assert np.array_equal(m.histogram_heights(c, edges[None], cumulative)[0], n)
    plt.close(fig)


# ------------------------------------------------------------------------------------------------ vs the reference
def test_host_functions_are_the_references(gold):
    from beat_amd import marginals as m
    for mind, maxd, nbins, bins in gold["hb"]:
        assert m.hist_binning(mind, maxd, int(nbins)) == int(bins)
    for llk, idx in zip(gold["fit_llk"], gold["fit_idx"]):
        got = m.get_fit_indexes(llk)
        assert [int(got[k]) for k in ("mean", "min", "max")] == idx.tolist()


def test_histplot_op_fixture(gold):
    """what histplot_op hands to ax.hist, reproduced: bins = hist_binning of the 0.01 / 99.99 percentiles, the counts on
    numpy's edges, the heights"""
    from beat_amd import marginals as m
    for k in range(int(gold["hist_n"])):
        d, key = gold["hist%d_d" % k], "hist%d" % k
        S = np.sort(d)[None]
        qu = ref.percentiles(S, [0.01, 99.99, 5, 68, 95])[0]
        assert np.array_equal(qu, gold[key + "_quants"])
        bins = m.hist_binning(qu[0], qu[1], nbins=40)
        assert bins == int(gold[key + "_bins"])
        e = ref.outer_edges(d.min(), d.max(), bins)
        assert np.array_equal(e, gold[key + "_edges"])
        h = m.histogram_heights(ref.hist_counts(S, e[None]), e[None], bool(gold[key + "_cumulative"]))[0]
        assert np.array_equal(h, gold[key + "_n"])


def test_kde_restatement_against_fixture_and_scipy(gold):
    from scipy import stats
    for k in range(int(gold["kde_n"])):
        x, y, Zmp = gold["kde%d_x" % k], gold["kde%d_y" % k], gold["kde%d_Zmp" % k]
        Z = ref.kde2d(x, y, *Zmp.shape)
        unit = 2.0 ** -53 * Zmp.max()
        bound = max(16.0 * float(gold["kde%d_scipy_units" % k]), 8.0)
        assert np.abs(Z - Zmp).max() / unit <= bound, (k, np.abs(Z - Zmp).max() / unit, bound)
        # the reference's own kde2plot_op (square grid, mgrid points): the same rows where the grids agree
        Zr = gold["kde%d_Z" % k]
        assert np.abs(ref.kde2d(x, y, *Zr.shape) - Zr).max() <= 1e-9 * Zr.max()
        assert np.array_equal(gold["kde%d_extent" % k], [x.min(), x.max(), y.min(), y.max()])
    rng = np.random.default_rng(6)
    x = rng.normal(3, 1, 257)
    y = 0.999 * (x - 3) + np.sqrt(1 - 0.999 ** 2) * rng.normal(0, 1, 257)
    G = np.meshgrid(np.linspace(x.min(), x.max(), 9), np.linspace(y.min(), y.max(), 7), indexing="ij")
    Zs = stats.gaussian_kde(np.vstack([x, y]))(np.vstack([G[0].ravel(), G[1].ravel()])).reshape(9, 7)
    assert np.abs(ref.kde2d(x, y, 9, 7) - Zs).max() <= 1e-9 * Zs.max()


def test_spherical_restatement_against_fixture(gold):
    lats, lons = gold["sph_lats"], gold["sph_lons"]
    for k in range(int(gold["sph_n"])):
        key = "sph%d" % k
        lats0, lons0, sigma = gold[key + "_lats0"], gold[key + "_lons0"], float(gold[key + "_sigma"])
        unit = (1.0 + 1.0 / sigma ** 2) * 2.0 ** -53
        got = ref.spherical_kde(lats0, lons0, lats, lons, sigma)
        for want in (gold[key + "_kdemp"], gold[key + "_kde"]):
            assert np.abs(got - want).max() <= 8.0 * unit * want.max(), (k, np.abs(got - want).max() / (unit * want.max()))
        # vonmises_fisher itself: the log-density of the first samples
        U0, Ug = ref.unit_vectors(lats0[:3], lons0[:3]), ref.unit_vectors(lats, lons)
        vmf = ref.vmf_norm(sigma) + np.tensordot(Ug, U0, axes=[[0], [0]]).reshape(lats.shape + (-1,)) / sigma ** 2
        np.testing.assert_allclose(vmf, gold[key + "_vmf"], rtol=0, atol=8.0 * unit * np.abs(gold[key + "_vmf"]).max())
        if lats0.size > 1:
            np.testing.assert_allclose(ref.vonmises_std(lons=lons0, lats=lats0), float(gold[key + "_sigmahat"]), rtol=1e-12)


def test_vmf_norm_is_the_restatements():
    from beat_amd import marginals as m
    for sigma in (0.3, 0.05, 0.01, 1.0):
        assert m.vmf_norm(sigma) == ref.vmf_norm(sigma)


def test_correlation_pairs_follow_the_plot_loop():
    from beat_amd import marginals as m
    assert m.correlation_pairs([4, 1, 7]).tolist() == [[4, 1], [4, 7], [1, 7]]
    assert m.correlation_pairs(range(10)).shape == (45, 2)
    assert m.correlation_pairs([3]).shape == (0, 2)


# ------------------------------------------------------------------------------------------------ ABI, argument rules
NEW_ENTRIES = {"beatamd_column_sort": 8, "beatamd_column_percentiles": 7, "beatamd_column_histograms": 7,
               "beatamd_pair_hist2d": 12, "beatamd_pair_kde2d": 14, "beatamd_unit_vector_sum": 6, "beatamd_spherical_kde": 11}


def test_marginals_entries_are_declared_and_bound():
    from beat_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "beat_amd.h")).read()
    lib = _lib.load()
    for name, arity in NEW_ENTRIES.items():
        m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr)
        assert m, "%s is not declared" % name
        assert len(m.group(1).split(",")) == arity == len(_lib._PROTOS[name]), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for cite in ("beat/plotting/common.py:248-397", "common.py:445-461", "common.py:471-523",
                 "beat/models/distributions.py:245-337", "beat/plotting/seismic.py:2707-2729"):
        assert cite in hdr
    assert lib.beatamd_version() == 120


def test_argument_rules_need_no_device():
    from beat_amd import marginals as m, marginals_binding as mb
    X = np.zeros((5, 3))
    with pytest.raises(ValueError):
        m.percentiles(np.zeros(5), [50])                    # not (n, V)
    with pytest.raises(ValueError):
        m.percentiles(np.zeros((0, 3)), [50])               # no sample
    with pytest.raises(IndexError):
        m.sort_columns(X, cols=[0, 3])
    with pytest.raises(IndexError):
        m.sort_columns(X, cols=[-1])
    with pytest.raises(ValueError):
        m.sort_columns(X, cols=[0.5])
    with pytest.raises(IndexError):
        m.kde2d(X, [[0, 3]])
    with pytest.raises(ValueError):
        m.kde2d(X, [0, 1])                                  # not (P, 2)
    with pytest.raises(ValueError):
        m.histograms(X)                                     # neither edges nor bins
    with pytest.raises(ValueError):
        m.histograms(X, bins=0)
    with pytest.raises(ValueError):
        mb.check_percents([50, 101])
    with pytest.raises(ValueError):
        mb.check_percents([np.nan])
    with pytest.raises(ValueError, match="increase monotonically"):
        mb.check_edges(np.array([[0.0, 1.0, 0.5], [0.0, 1.0, 2.0]]), 2)
    with pytest.raises(ValueError):
        mb.check_edges(np.array([[0.0, np.inf]]), 1)
    with pytest.raises(ValueError):
        mb.check_edges(np.array([[0.0]]), 1)                # no bin
    assert mb.check_edges(np.array([[0.0, 0.0, 1.0]]), 1).shape == (1, 3)     # equal edges are numpy's too
    with pytest.raises(ValueError, match="128 x 128"):
        mb.check_hist2d_bins(129, 128)
    with pytest.raises(ValueError, match="128 x 128"):
        m.hist2d(X, [[0, 1]], bins=(129, 128))
    assert mb.check_hist2d_bins(128, 128) == (128, 128) and mb.check_hist2d_bins(1, 4096) == (1, 4096)
    with pytest.raises(ValueError):
        mb.check_hist2d_bins(1, 4097)
    with pytest.raises(ValueError):
        mb.check_grid((0, 5))
    assert mb.check_grid(200) == (200, 200) and mb.check_grid((9, 7)) == (9, 7)
    with pytest.raises(ValueError, match="launch shape"):
        m.kde2d(X, [[0, 1]], shape="tall")
    with pytest.raises(ValueError, match="jitter"):
        m.lune_kde(np.full(50, 0.1), np.linspace(-0.5, 0.5, 50))      # v fixed
    with pytest.raises(ValueError):
        m.spherical_kde(np.zeros(4), np.zeros(5))
    with pytest.raises(ValueError):
        m.spherical_kde(np.zeros(4), np.zeros(4), lats=np.zeros((3, 3)), lons=np.zeros((3, 3)), grid_size=(2, 2))


@pytest.mark.skipif(_gpu_present(), reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    from beat_amd import BeatAmdError, marginals as m
    rng = np.random.default_rng(7)
    X = rng.standard_normal((50, 3))
    calls = [lambda: m.sort_columns(X), lambda: m.percentiles(X, [50]), lambda: m.make_bins(X),
             lambda: m.histograms(X, bins=10), lambda: m.hist2d(X, [[0, 1]]), lambda: m.kde2d(X, [[0, 1]], grid=5),
             lambda: m.correlation_kdes(X, [0, 1, 2], grid=5), lambda: m.spherical_kde(X[:, 0], X[:, 1], grid_size=(4, 4)),
             lambda: m.spherical_kde(X[:, 0], X[:, 1], grid_size=(4, 4), sigma=0.3),
             lambda: m.lune_kde(rng.uniform(-0.3, 0.3, 50), rng.uniform(-1.0, 1.0, 50), grid_size=(4, 4))]
    for call in calls:
        with pytest.raises(BeatAmdError):
            call()


KERNELS = ("k_col_check", "k_col_sort_tile", "k_col_sort_global", "k_col_percentiles", "k_col_hist", "k_pair_hist2d",
           "k_pair_moments", "k_pair_whiten", "k_pair_kde2d", "k_sph_unit", "k_sph_sum", "k_sph_kde")


def test_marginals_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "beat_amd", "csrc", "marginals.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "marginals.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    seen, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    assert len(seen) == len(KERNELS) + 2, sorted(seen)      # every kernel of the file is listed above; the KDEs have two shapes
    for kern in KERNELS:
        hits = [v for k, v in seen.items() if kern in k]
        assert hits, "no resource report for %s:\n%s" % (kern, r.stdout[-2000:])
        assert hits == [0] * len(hits), "%s uses scratch: %s" % (kern, hits)
    # the tile of the column sort and the caps of the 2-d histogram are stated once, and the binding repeats them
    from beat_amd import marginals_binding as mb
    hpp = open(os.path.join(ROOT, "beat_amd", "csrc", "kernels.hpp")).read()
    assert "MG_SORT_TILE = 16384" in hpp and "MG_HIST2D_MAX_CELLS = 128 * 128, MG_HIST2D_MAX_SIDE = 4096" in hpp
    assert (mb.HIST2D_MAX_CELLS, mb.HIST2D_MAX_SIDE, mb.SORT_MAX_N) == (128 * 128, 4096, 1 << 24)
