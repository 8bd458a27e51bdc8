"""CPU tests of the geodetic non-Toeplitz data covariance: the numpy restatement of csrc/noise2d.hip's one summation order
(tests/noise2d_ref.py) against the reference's numbers (tests/golden/noise2d.npz, tools/gen_golden_noise2d.py), the C ABI
table, the argument rules of the Python layer and the analyser's error texts."""
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise2d_ref as nref  # noqa: E402

FULL_CASES = ("n30", "n33", "laq0", "laq1", "n1024", "grid")


@pytest.fixture(scope="module")
def gold(golden):
    return golden("noise2d")


@pytest.fixture(scope="module")
def restated(gold):
    """the restatement of every case, once: {case: (radius, counts, stds)}"""
    return dict((c, nref.ball_rms(gold[c + "_coords"], gold[c + "_res"], float(gold[c + "_perc"])))
                for c in FULL_CASES + ("lone",))


# ------------------------------------------------------------------------------------------------- restatement vs the reference
@pytest.mark.parametrize("case", FULL_CASES)
def test_restatement_vs_fixture(gold, restated, case):
    """radius bit for bit ``utility.distances(coords, coords).max() * max_dist_perc``; the neighbour counts those of
    scipy's KDTree.query_ball_point (the 4 x 5 grid: every neighbour an exact tie); stds at rtol 1e-12, which is >= 8 x the
    first-order bound (count + 3) 2^-53 at count <= 1024 (the KD-tree's summation order is not defined).  Observed: 3.3e-16."""
    radius, counts, stds = restated[case]
    assert radius == float(gold[case + "_radius"])
    assert counts.dtype == np.int32 and np.array_equal(counts, gold[case + "_counts"])
    err = float(np.abs(stds / gold[case + "_stds"] - 1.0).max())
    print("%s: restatement vs the reference's stds: worst relative difference %.3g" % (case, err))
    np.testing.assert_allclose(stds, gold[case + "_stds"], rtol=1e-12, atol=0.0)


def test_the_grid_radius_is_exactly_one_and_every_neighbour_a_tie(gold, restated):
    c = gold["grid_coords"]
    assert float(gold["grid_radius"]) == 1.0 and restated["grid"][0] == 1.0
    want = np.array([np.sum(np.abs(c - p).sum(axis=1) <= 1.0) for p in c])     # itself and the grid neighbours
    assert np.array_equal(restated["grid"][1], want) and want.min() == 3 and want.max() == 5


@pytest.mark.parametrize("case", FULL_CASES)
def test_data_covariance_vs_fixture(gold, case):
    """C_d = toeplitz(coeffs) * stds stds^T of the restated composition against the reference's, rebuilt from the stored
    vectors, to 1e-11 of max|C_d|.  Observed: 7.5e-16."""
    ref = nref.scaled_toeplitz(gold[case + "_coeffs"], gold[case + "_stds"])
    got, _ = nref.non_toeplitz_covariance_2d(gold[case + "_coords"], gold[case + "_res"], float(gold[case + "_perc"]))
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max()) / scale
    print("%s: restated C_d vs the reference's: worst |difference| / max|C_d| = %.3g" % (case, err))
    assert err <= 1e-11
    from beat_amd.heart import Covariance
    np.testing.assert_allclose(Covariance(data=ref).log_pdet, float(gold[case + "_logpdet"]), rtol=1e-9)


def test_the_lone_point(gold, restated):
    """one point without a neighbour: count 1 there, NaN there and nowhere else"""
    _, counts, stds = restated["lone"]
    assert np.array_equal(counts, gold["lone_counts"])
    assert np.array_equal(np.isnan(stds), gold["lone_nan"])
    assert np.array_equal(np.nonzero(np.isnan(stds))[0], [17]) and counts[17] == 1


def test_restatement_order_depends_on_the_point_and_the_size_alone(gold):
    """a dataset alone and inside a batch: the same bits"""
    sizes = [2, 65, 33]
    rng = np.random.default_rng(5)
    coords, data = rng.uniform(-1, 1, (sum(sizes), 2)), rng.standard_normal(sum(sizes))
    rad, cnt, std = nref.ball_rms_batch(coords, data, sizes, 0.5)
    o = 0
    for i, n in enumerate(sizes):
        r, k, s = nref.ball_rms(coords[o:o + n], data[o:o + n], 0.5)
        assert r == rad[i] and np.array_equal(k, cnt[o:o + n]) and np.array_equal(s, std[o:o + n], equal_nan=True)
        o += n


# ------------------------------------------------------------------------------------------------- ABI table
def test_entry_is_declared_bound_and_built():
    from beat_amd import _lib
    from beat_amd.engine import Context
    header = open(os.path.join(ROOT, "include", "beat_amd.h")).read()
    m = re.search(r"int beatamd_ball_rms_batch\(([^;]*)\);", header)
    assert m, "beatamd_ball_rms_batch is not declared"
    nargs = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
    assert nargs == len(_lib._PROTOS["beatamd_ball_rms_batch"]) == 9
    assert "beat/covariance.py:774-811" in header
    assert "beatamd_ball_rms_batch" in _lib.EXPORTS and callable(Context.ball_rms_batch)
    assert _lib.ABI_VERSION == 120
    assert "noise2d.hip" in open(os.path.join(ROOT, "beat_amd", "csrc", "Makefile")).read()
    if os.path.exists(os.path.join(ROOT, "beat_amd", "libbeat_amd.so")):
        assert hasattr(_lib.load(), "beatamd_ball_rms_batch")


# ------------------------------------------------------------------------------------------------- argument rules
def test_k_nearest_neighbor_rms_argument_rules():
    from beat_amd import covariance as cov
    c, d = np.zeros((4, 2)), np.zeros(4)
    with pytest.raises(ValueError, match="Either k or max_dist_perc should be defined!"):
        cov.k_nearest_neighbor_rms(c, d, k=3)                       # max_dist_perc keeps its default: both given
    with pytest.raises(ValueError, match="Either k or max_dist_perc should be defined!"):
        cov.k_nearest_neighbor_rms(c, d, k=3, max_dist_perc=0.1)
    with pytest.raises(NotImplementedError, match="k nearest neighbours"):
        cov.k_nearest_neighbor_rms(c, d, k=3, max_dist_perc=None)
    with pytest.raises(ValueError):
        cov.k_nearest_neighbor_rms(c, d, k=None, max_dist_perc=None)
    assert cov.available_noise_structures_2d() == ["import", "non-toeplitz"]
    assert set(cov.NoiseStructureCatalog2d) < set(cov.NoiseStructureCatalog)
    assert np.array_equal(cov.NoiseStructureCatalog2d["non-toeplitz"](3), np.ones((3, 3)))
    for name in ("toeplitz_covariance_2d", "non_toeplitz_covariance_2d", "non_toeplitz_covariance_2d_batch"):
        assert callable(getattr(cov, name))


def _stub_model(sizes=(3, 4), corrections=None):
    g = SimpleNamespace(sizes=list(sizes), data=np.zeros(sum(sizes)), corrections=corrections, fixed={})
    return SimpleNamespace(problem=SimpleNamespace(geodetic=g, layout=None), geodetic_residuals=lambda *a, **k: None,
                           ctx=SimpleNamespace(device=0))


def test_update_object_argument_rules():
    from beat_amd.covariance import GeodeticNoiseCovarianceUpdate as U
    from beat_amd.heart import Covariance
    f = _stub_model()
    covs = [Covariance(data=np.eye(3)), Covariance(data=np.eye(4))]
    coords = [np.zeros((3, 2)), np.zeros((4, 2))]
    u = U(f, coords, covs, 0.2)
    assert (u.last_ms, u.n_updates, u.n_host_route) == (0.0, 0, 0) and u.typs == ["SAR", "SAR"] and u.sar == [0, 1]
    assert U(f, coords, covs, 0.2, typs=["SAR", "GNSS"]).sar == [0]
    with pytest.raises(ValueError, match="1 covariances for 2 geodetic datasets"):
        U(f, coords, covs[:1], 0.2)
    with pytest.raises(ValueError, match="1 coordinate arrays for 2"):
        U(f, coords[:1], covs, 0.2)
    with pytest.raises(ValueError, match="dataset 1: coordinates of shape \\(3, 2\\), expected \\(4, 2\\)"):
        U(f, [coords[0], coords[0]], covs, 0.2)
    with pytest.raises(ValueError, match="1 dataset types for 2"):
        U(f, coords, covs, 0.2, typs=["SAR"])
    with pytest.raises(ValueError, match="max_dist_perc must be finite"):
        U(f, coords, covs, float("nan"))
    with pytest.raises(ValueError, match="no geodetic composite"):
        U(SimpleNamespace(problem=SimpleNamespace(geodetic=None)), coords, covs, 0.2)
    other = SimpleNamespace(f=_stub_model(), covariances=covs)
    with pytest.raises(ValueError, match="same model and Covariance objects"):
        U(f, coords, covs, 0.2, velocity=other)
    assert U(f, coords, covs, 0.2, velocity=SimpleNamespace(f=f, covariances=covs)).velocity is not None


# ------------------------------------------------------------------------------------------------- the analyser
def test_analyser_rules_and_error_texts():
    from beat_amd.covariance import GeodeticNoiseAnalyser
    from beat_amd.heart import Covariance
    with pytest.raises(AttributeError, match='Selected noise structure "variance" not supported! Implemented'
                                             " noise structures: import, non-toeplitz"):
        GeodeticNoiseAnalyser(SimpleNamespace(structure="variance", max_dist_perc=0.2))
    imp = GeodeticNoiseAnalyser(SimpleNamespace(structure="import", max_dist_perc=0.2))
    C = np.diag([1.0, 2.0, 3.0])
    ds = SimpleNamespace(typ="SAR", id="scene_A", ncoords=3, covariance=Covariance(data=C))
    assert np.array_equal(imp.get_structure(ds), np.ones((3, 3)))
    assert np.array_equal(imp.get_data_covariance(ds), C)
    with pytest.raises(ValueError, match="Data covariance for dataset scene_A needs to be defined!"):
        imp.do_import(SimpleNamespace(id="scene_A", covariance=Covariance()))
    ntz = GeodeticNoiseAnalyser(SimpleNamespace(structure="non-toeplitz", max_dist_perc=0.2), events=[None])
    gnss = SimpleNamespace(typ="GNSS", id="net_B", ncoords=3, covariance=Covariance(data=C))
    assert np.array_equal(ntz.do_non_toeplitz(gnss, None), C)             # no SAR scene: keeps covariance.data
    assert np.array_equal(ntz.get_data_covariance(gnss), C)
    bad = C.copy()
    bad[1, 1] = np.nan
    gnss.covariance.data = bad
    with pytest.raises(ValueError, match="Estimated Non-Toeplitz covariance matrix for dataset net_B contains Nan! "
                                         "Please increase 'max_dist_perc'!"):
        ntz.do_non_toeplitz(gnss, None)
