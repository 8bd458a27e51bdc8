"""Dataset corrections of the geodetic likelihood, host side: the numpy restatement, the basis columns and the names
against the reference's own numbers (tests/golden/geo_corrections.npz, written by tools/gen_golden_corrections.py
from the reference's RampCorrection / StrainRateCorrection)."""
import re
from collections import OrderedDict

import numpy as np
import pytest

import corrections_ref as cref
from conftest import ROOT, load_golden

RAMP_SUFFIXES = ["azimuth_ramp", "range_ramp", "offset"]
STRAIN_SUFFIXES = ["exx", "eyy", "exy", "rotation"]


def _ramp(g, d):
    from beat_amd.models.corrections import RampConfig
    names = [str(s) for s in g["ramp_names"]]
    corr = RampConfig(dataset_names=names, enabled=True).init_correction()
    corr.setup_correction(g["ramp%d_north_shifts" % d], g["ramp%d_east_shifts" % d], None, None, names[d])
    return corr


def _strain(g, b, local=True):
    from beat_amd.models.corrections import StrainRateConfig
    corr = StrainRateConfig(dataset_names=["gnss"], enabled=True).init_correction()
    corr.setup_correction(g["strain_lats"], g["strain_lons"], g["strain%d_los" % b], g["strain_mask"], "gnss", number=b,
                          local_coordinates=(g["strain_norths"], g["strain_easts"]) if local else None)
    return corr


def test_fixture_shape():
    g = load_golden("geo_corrections")
    assert int(g["ramp_n"]) == 2
    assert g["ramp0_disp"].shape[1] == 214 and g["ramp1_disp"].shape[1] == 205
    assert g["ramp0_coefs"].shape[0] >= 8 and g["strain_coefs"].shape[0] >= 8
    assert np.all(np.abs(g["ramp0_coefs"][:, :2]) <= 0.1) and np.all(np.abs(g["ramp0_coefs"][:, 2]) <= 0.05)
    assert np.all(np.abs(g["strain_coefs"]) <= 200.0)
    m = g["strain_mask"]
    assert m.size >= 60 and m.any() and not m.all()


def test_restatement_ramp_bitwise():
    g = load_golden("geo_corrections")
    for d in range(2):
        n, e = g["ramp%d_north_shifts" % d], g["ramp%d_east_shifts" % d]
        for i, co in enumerate(g["ramp%d_coefs" % d]):
            disp = cref.ramp(n, e, *co)
            assert np.array_equal(disp, g["ramp%d_disp" % d][i])
            res = (g["ramp%d_data" % d] - g["ramp%d_mu" % d][i]) * g["ramp%d_odw" % d]
            assert np.array_equal(cref.apply_corrections([res], [[disp]])[0], g["ramp%d_res" % d][i])


def test_restatement_strain_rate():
    g = load_golden("geo_corrections")
    for b in range(2):
        B = _strain(g, b).basis()
        for i, co in enumerate(g["strain_coefs"]):
            disp = cref.strain_rate(g["strain_norths"], g["strain_easts"], g["strain%d_los" % b], g["strain_mask"], *co)
            want = g["strain%d_disp" % b][i]
            assert np.all(np.abs(disp - want) <= cref.strain_bound(B, co))
            assert np.all(disp[g["strain_mask"]] == 0.0)


def test_basis_through_contract_formula():
    """basis() pushed through the arithmetic the C ABI documents: the ramp bit for bit the reference's, the strain
    rate within the derived bound (asserted element by element), masked rows exactly zero"""
    g = load_golden("geo_corrections")
    for d in range(2):
        B = _ramp(g, d).basis()
        assert B.shape == (g["ramp%d_disp" % d].shape[1], 3) and np.all(B[:, 2] == 1.0)
        for i, co in enumerate(g["ramp%d_coefs" % d]):
            assert np.array_equal(cref.contract(B, co), g["ramp%d_disp" % d][i])
            res = (g["ramp%d_data" % d] - g["ramp%d_mu" % d][i]) * g["ramp%d_odw" % d] - cref.contract(B, co)
            assert np.array_equal(res, g["ramp%d_res" % d][i])
    for b in range(2):
        B = _strain(g, b).basis()
        assert B.shape == (g["strain_mask"].size, 4)
        assert np.all(B[g["strain_mask"]] == 0.0)
        worst = 0.0
        for i, co in enumerate(g["strain_coefs"]):
            got, want = cref.contract(B, co), g["strain%d_disp" % b][i]
            bound = cref.strain_bound(B, co)
            assert np.all(np.abs(got - want) <= bound)
            assert np.all(got[g["strain_mask"]] == 0.0) and np.all(want[g["strain_mask"]] == 0.0)
            nz = bound > 0
            worst = max(worst, float(np.max(np.abs(got - want)[nz] / (bound[nz] / 16))))
        print("strain block %d: worst |diff| / (2^-53 sum|B coef|) = %.2f (bound 16)" % (b, worst))


def test_names_suffixes_and_displacements():
    from beat_amd.models.corrections import RampConfig, StrainRateConfig
    g = load_golden("geo_corrections")
    names = [str(s) for s in g["ramp_names"]]
    cfg = RampConfig(dataset_names=names[:1], enabled=True)
    assert cfg.get_suffixes() == RAMP_SUFFIXES
    assert cfg.get_hierarchical_names(names[0]) == ["%s_%s" % (names[0], s) for s in RAMP_SUFFIXES]
    assert cfg.get_hierarchical_names(names[1]) == []          # not configured for that scene
    scfg = StrainRateConfig(dataset_names=["gnss"], enabled=True)
    assert scfg.get_suffixes() == STRAIN_SUFFIXES
    assert scfg.get_hierarchical_names(name="gnss", number=3) == ["3_%s" % s for s in STRAIN_SUFFIXES]
    with pytest.raises(AttributeError):
        RampConfig(dataset_names=[], enabled=True).init_correction()
    for d in range(2):
        corr = _ramp(g, d)
        assert corr.get_required_coordinate_names() == ["east_shifts", "north_shifts"]
        assert corr.correction_names == ["%s_%s" % (names[d], s) for s in RAMP_SUFFIXES]
        for i, co in enumerate(g["ramp%d_coefs" % d]):
            point = dict(zip(corr.correction_names, co))
            assert np.array_equal(corr.get_displacements({}, point=point), g["ramp%d_disp" % d][i])
            # fixed variables: not in the point, taken from the hierarchicals
            assert np.array_equal(corr.get_displacements(point, point={"other": 1.0}), g["ramp%d_disp" % d][i])
    for b in range(2):
        corr = _strain(g, b)
        assert corr.get_required_coordinate_names() == ["lons", "lats"]
        assert corr.correction_names == ["%d_%s" % (b, s) for s in STRAIN_SUFFIXES]
        for i, co in enumerate(g["strain_coefs"]):
            point = dict(zip(corr.correction_names, co))
            got = corr.get_displacements({}, point=point)
            assert np.all(np.abs(got - g["strain%d_disp" % b][i]) <= cref.strain_bound(corr.basis(), co))
    unset = RampConfig(dataset_names=names, enabled=True).init_correction()
    with pytest.raises(ValueError):
        unset.get_displacements({}, point={"x": 1.0})


def test_strain_rate_needs_local_coordinates_without_pyrocko():
    g = load_golden("geo_corrections")
    try:
        import pyrocko  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="local_coordinates"):
            _strain(g, 0, local=False)
    else:
        corr = _strain(g, 0, local=False)
        assert corr.norths.shape == g["strain_norths"].shape


def test_free_fixed_resolution_and_keyerror():
    from beat_amd.models import ParameterLayout
    from beat_amd.models.corrections import correction_tables
    g = load_golden("geo_corrections")
    names = [str(s) for s in g["ramp_names"]]
    r0, r1 = _ramp(g, 0), _ramp(g, 1)
    lay = ParameterLayout(OrderedDict([("uparr", 5), (r0.correction_names[0], 1), (r0.correction_names[2], 1),
                                       (r1.correction_names[1], 1), ("h_SAR", 1)]))
    fixed = {r0.correction_names[1]: 0.03, r1.correction_names[0]: -0.02, r1.correction_names[2]: 0.0}
    ds, ncol, basis, off, fix = correction_tables([[r0], [r1]], [214, 205], lay, fixed)
    assert ds == [0, 1] and ncol == [3, 3]
    assert off == [[5, -1, 6], [-1, 7, -1]]
    assert fix == [[0.0, 0.03, 0.0], [-0.02, 0.0, 0.0]]
    assert np.array_equal(basis[1], r1.basis())
    # one scene corrected, one not; no corrections at all
    assert correction_tables([[r0], []], [214, 205], lay, fixed)[0] == [0]
    assert correction_tables([[], None], [214, 205], lay, fixed)[0] == []
    assert correction_tables(None, [214, 205], lay)[0] == []
    with pytest.raises(KeyError, match=re.escape(r1.correction_names[0])):
        correction_tables([[r0], [r1]], [214, 205], lay, {r0.correction_names[1]: 0.03})
    with pytest.raises(ValueError):
        correction_tables([[r1], [r0]], [214, 205], lay, fixed)     # basis length != dataset size
    with pytest.raises(ValueError):
        correction_tables([[r0]], [214, 205], lay, fixed)           # one list per dataset


def test_rvs_list_the_correction_variables():
    """LogpForwFunc(return_rvs=True) lists the free variables in layout order: the hierarchical ones are among
    them because they are part of the layout (no device needed: the names come from the layout)"""
    from beat_amd.models import LogpForwFunc, ParameterLayout
    g = load_golden("geo_corrections")
    r0 = _ramp(g, 0)
    lay = ParameterLayout(OrderedDict([("uparr", 5)] + [(n, 1) for n in r0.correction_names] + [("h_SAR", 1)]))

    class _Prob(object):
        layout, wavemaps, geodetic, laplacian = lay, [], object(), None

    class _Ctx(object):
        def ffi_model_nllk(self, mid):
            return 2

    f = LogpForwFunc(_Ctx(), 0, _Prob(), return_rvs=True, wsets=[], geo_wsets=[])
    assert f.out_names == ["uparr"] + r0.correction_names + ["h_SAR", "geo_like", "like"]
    assert f._llk_index == len(f.out_names) - 1


def test_symbol_declared_exported_and_bound():
    from beat_amd import _lib
    name = "beatamd_ffi_model_add_geodetic_corrections"
    hdr = open(ROOT + "/include/beat_amd.h").read()
    assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
    assert name in _lib.EXPORTS and len(_lib._PROTOS[name]) == 8
    assert hasattr(_lib.load(), name)
    assert _lib.ABI_VERSION == 120 and "BEATAMD_VERSION 120" in re.sub(r"\s+", " ", hdr)
