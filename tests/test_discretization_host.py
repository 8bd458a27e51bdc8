"""Host side of the geodetic library builder and the resolution-based discretization: the patch arithmetic, the index
mapping, the elbow, the spread and both host smoothing operators against the recorded outputs of the reference's own
functions (tests/golden/discretization_reference.npz, tools/gen_golden_discretization.py) -- bit for bit -- and against
the fixture problem (tests/golden/discretization_fixture.npz, restated)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import discretization_ref as dref  # noqa: E402
from beat_amd import _lib, discretization as dz, utility  # noqa: E402
from beat_amd.models import laplacian  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(HERE, "golden", "discretization_reference.npz"))


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(HERE, "golden", "discretization_fixture.npz"))


def test_division_mapping_equals_the_reference(ref):
    for k in range(int(ref["nmap"])):
        counts, div = ref["map%d_counts" % k], ref["map%d_div" % k]
        o2n, d2n, new = dz.get_division_mapping(range(int(counts.sum())), div.tolist(), counts)
        assert list(o2n.items()) == [tuple(r) for r in ref["map%d_old2new" % k].tolist()]
        assert list(d2n.items()) == [tuple(r) for r in ref["map%d_div2new" % k].tolist()]
        np.testing.assert_array_equal(new, ref["map%d_new" % k])
        assert new.dtype == counts.dtype


def test_distances_bitwise(ref):
    np.testing.assert_array_equal(utility.distances(ref["coords_a"], ref["coords_a"]), ref["dist_a"])
    np.testing.assert_array_equal(utility.distances(ref["dist2_points"], ref["dist2_ref"]), ref["dist2"])
    with pytest.raises(TypeError):
        utility.distances(np.zeros((3, 2)), np.zeros((3, 3)))


def test_find_elbow_and_spread_bitwise(ref):
    data = ref["elbow_data"]
    for tag, kw in (("left", dict(rotate_left=True)), ("plain", dict()), ("theta", dict(theta=0.3))):
        idx, rot = utility.find_elbow(data, **kw)
        assert idx == int(ref["elbow_%s_idx" % tag])
        np.testing.assert_array_equal(rot, ref["elbow_%s_rot" % tag])
    assert utility.get_data_radiant(data) == float(ref["radiant"])
    assert utility.normalized_resolution_spread(ref["spread_R"], 23) == float(ref["spread"])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_correlated_operators_bitwise(ref, tag):
    c = ref["coords_" + tag]
    g = laplacian.get_smoothing_operator_correlated(c, "gaussian")
    e = laplacian.get_smoothing_operator_correlated(c, "exponential")
    np.testing.assert_array_equal(g, ref["gauss_" + tag])
    np.testing.assert_array_equal(e, ref["expo_" + tag])
    # the documented order (rows ascending) is numpy's a.sum(0) order, also past the pairwise block of 128
    np.testing.assert_array_equal(dref.smoothing_correlated(c, "gaussian"), g)
    np.testing.assert_array_equal(dref.smoothing_correlated(c, "exponential"), e)
    with pytest.raises(ValueError):
        laplacian.get_smoothing_operator_correlated(c, "nearest_neighbor")


def test_nearest_neighbor_and_block_diagonal_operator():
    from beat_amd.synthetic import smoothing_operator_nearest_neighbor
    a = laplacian.get_smoothing_operator_nearest_neighbor(3, 2, 1.5, 2.0)
    np.testing.assert_array_equal(a, smoothing_operator_nearest_neighbor(3, 2, 1.5, 2.0))
    b = laplacian.get_smoothing_operator_nearest_neighbor(2, 2, 1.0, 0.5)
    L = laplacian.get_smoothing_operator([(3, 2, 1.5, 2.0), (2, 2, 1.0, 0.5)], correlation_function="nearest_neighbor")
    assert L.shape == (10, 10)
    np.testing.assert_array_equal(L[:6, :6], a)
    np.testing.assert_array_equal(L[6:, 6:], b)
    assert not L[:6, 6:].any() and not L[6:, :6].any()
    np.testing.assert_array_equal(L.sum(1), np.zeros(10))
    with pytest.raises(laplacian.InvalidDiscretizationError):
        laplacian.get_smoothing_operator(None, np.zeros((4, 3)), "nearest_neighbor")
    fault = dz.DiscretizedFault(dref.fixture_problem()["subfaults"])
    with pytest.raises(laplacian.InvalidDiscretizationError):
        fault.get_smoothing_operator(None, "nearest_neighbor")


def test_patch_cutting_and_division():
    fp = dref.fixture_problem()
    for sf, (nl, nw) in zip(fp["subfaults"], ((3, 2), (2, 2))):
        cut = dz.cut_patches(sf, nl, nw)
        np.testing.assert_array_equal(cut, dref.patches(sf, nl, nw))
        assert cut.shape == (nl * nw, 10)
        # row-wise from shallow to deep; the patches tile the source
        assert np.all(np.diff(cut[::nl, 2]) >= 0)
        np.testing.assert_allclose(cut[:, 6], sf[6] / nl, rtol=0, atol=0)
        cen = np.array([dz.center(p) for p in cut])
        np.testing.assert_allclose(cen.mean(0), dz.center(sf), rtol=1e-14, atol=1e-14)
        np.testing.assert_array_equal(cen, dref.centers(cut))
    # the vertical subfault: the dip vector has no horizontal part beyond cos(90 deg)'s rounding
    v = fp["subfaults"][1]
    assert abs(dz.bottom_depth(v) - (v[2] + v[7])) < 1e-15
    np.testing.assert_allclose(dz.bottom_left(v)[:2], np.array(v[:2]) - 0.5 * v[6] * dz.strikevector(v)[:2], atol=1e-15)
    # division along the longer side, along strike on a tie
    wide = np.array([0, 0, 1, 10, 50, 0, 2.0, 3.0, 1, 0], dtype=float)
    assert dz.divide_patch(wide)[:, 7].tolist() == [1.5, 1.5] and dz.divide_patch(wide)[:, 6].tolist() == [2.0, 2.0]
    sq = np.array([0, 0, 1, 10, 50, 0, 3.0, 3.0, 1, 0], dtype=float)
    assert dz.divide_patch(sq)[:, 6].tolist() == [1.5, 1.5] and dz.divide_patch(sq)[:, 7].tolist() == [3.0, 3.0]
    # get_n_patches: round(.., 4) then ceil
    assert dz.get_n_patches(12.0, 4.0) == 3 and dz.get_n_patches(6.5, 3.4) == 2
    assert dz.get_n_patches(3.00004, 1.0) == 3 and dz.get_n_patches(3.0002, 1.0) == 4


def test_slip_directions():
    p = dref.fixture_problem()["subfaults"]
    for comp, (drake, opening) in dref.COMPONENTS.items():
        rows = dz.component_parameters(p, comp)
        np.testing.assert_array_equal(rows[:, 5], p[:, 5] + drake)
        np.testing.assert_array_equal(rows[:, 8], 1.0)
        np.testing.assert_array_equal(rows[:, 9], p[:, 9] if opening is None else opening)
        np.testing.assert_array_equal(rows, dref.component_rows(p, comp))
    with pytest.raises(ValueError):
        dz.component_parameters(p, "slip")


def test_restatement_reproduces_the_recorded_fixture(fix):
    """the recorded decisions are what the restatement gives on this machine too (the margins make that robust)"""
    fp = dref.fixture_problem()
    res = dref.optimize(fp["cfg"], fp["subfaults"], fp["east"], fp["north"], fp["los"], fp["odw"], fp["nu"],
                        fp["varnames"])
    assert len(res["generations"]) == int(fix["ngen"]) >= 3
    for g, gen in enumerate(res["generations"]):
        np.testing.assert_array_equal(gen["sf_div_idxs"], fix["g%d_sf_div_idxs" % g])
        np.testing.assert_array_equal(gen["fixed_idxs"], fix["g%d_fixed_idxs" % g])
        np.testing.assert_array_equal(gen["subfault_npatches"], fix["g%d_subfault_npatches" % g])
    np.testing.assert_allclose(res["params"], fix["params"], rtol=1e-13, atol=1e-13)
    assert len(res["params"]) % 16 != 0
    # the two index mappings agree
    for g, gen in enumerate(res["generations"][:-1]):
        counts = gen["subfault_npatches"]
        a = dz.get_division_mapping(range(sum(counts)), gen["sf_div_idxs"].tolist(), np.array(counts))
        b = dref.division_mapping(sum(counts), gen["sf_div_idxs"], counts)
        assert dict(a[0]) == b[0] and dict(a[1]) == b[1]
        np.testing.assert_array_equal(a[2], b[2])


def test_config_defaults_and_result():
    c = dz.ResolutionDiscretizationConfig()
    assert (c.epsilon, c.epsilon_search_runs, c.resolution_thresh, c.depth_penalty, c.alpha) == (4.0e-3, 1, 0.999, 3.5,
                                                                                               0.3)
    assert c.patch_widths_min == [1.0] and c.patch_widths_max == [5.0]
    assert c.patch_lengths_min == [1.0] and c.patch_lengths_max == [5.0]
    assert c.get_patch_dimensions() == ([5.0], [5.0])
    r = dz.ResolutionDiscretizationResult([0.01, 0.1, 1.0], [0.07, 0.03, 0.029], [50, 40, 30])
    r.derive_optimum_fault_geometry()
    data = np.array([[0.01, 0.07], [0.1, 0.03], [1.0, 0.029]])
    assert r.optimum["idx"] == int(utility.find_elbow(data, rotate_left=True)[0])
    assert r.optimum["npatches"] == r.faults_npatches[r.optimum["idx"]]
    assert "normalized_rspreads" in r.dump()


def test_svd_and_foreign_engines_raise():
    fp = dref.fixture_problem()
    fault = dz.DiscretizedFault(fp["subfaults"])
    cfg = dz.ResolutionDiscretizationConfig(**fp["cfg"])
    with pytest.raises(NotImplementedError, match="svd"):
        dz.optimize_discretization(cfg, fault, [], fp["varnames"], engine=None, method="svd")
    from beat_amd import ffi
    with pytest.raises(TypeError, match="static displacements"):
        ffi.geo_construct_gf_linear_patches(object(), datasets=[], patches=np.zeros((1, 10)))
    with pytest.raises(TypeError, match="static displacements"):
        dz.optimize_discretization(cfg, fault, [], fp["varnames"], engine=object())


def test_new_symbols_are_exported_and_declared():
    names = ["beatamd_geo_gf_library", "beatamd_smoothing_correlated", "beatamd_model_resolution",
             "beatamd_division_rating"]
    with open(os.path.join(HERE, "..", "include", "beat_amd.h")) as f:
        header = f.read()
    for n in names:
        assert n in _lib.EXPORTS and n in _lib._PROTOS
        assert ("int %s(" % n) in header
    assert "beat/ffi/base.py:804-1002" in header
