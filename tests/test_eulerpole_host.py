"""The Euler-pole correction, host side: the numpy evaluation in the reference's order, the linear form
``basis() @ coefficients()`` and the coupling lines against the reference's own numbers and 50-digit mpmath values
(tests/golden/euler_pole.npz, written by tools/gen_golden_eulerpole.py).

Bound per entry: 16 * 2^-53 * |w'| * |l_i|_1 (w' = omega * 1e-6 * pi/180 * r_earth).  Observed here (numpy): the
reference's values lie <= 4.4 of those units from the mpmath values; get_displacements (cross product by components,
one dot product per local axis) lies 0 from the reference's values -- the same IEEE products and sums in the same
order --, the linear form <= 3.8 from the reference and <= 5.9 from mpmath, the three coefficients
<= 2.5 units of 2^-53 |w'| from mpmath (the tests print the maxima)."""
import re
from collections import OrderedDict

import numpy as np
import pytest

import eulerpole_ref as eref
from conftest import ROOT, load_golden

SUFFIXES = ["pole_lat", "pole_lon", "omega"]


def _pole(g, b, earth=None, number=None):
    from beat_amd.models.corrections import EarthModel, EulerPoleConfig
    corr = EulerPoleConfig(dataset_names=["gnss"], enabled=True).init_correction()
    corr.setup_correction(g["lats"], g["lons"], g["los%d" % b], g["mask"], "gnss", number=b if number is None else number,
                          earth=earth if earth is not None else EarthModel(*g["earth"]))
    return corr


def test_fixture_shape():
    g = load_golden("euler_pole")
    assert g["lats"].size == 72 and g["mask"].sum() == 9 and g["coefs"].shape[0] >= 12 + 7
    co = g["coefs"]
    assert np.all(np.abs(co[:, 0]) <= 90) and np.all(np.abs(co[:, 1]) <= 180) and np.all(np.abs(co[:, 2]) <= 10)
    assert (co[:, 0] == 90).any() and (co[:, 0] == -90).any() and (co[:, 1] == 180).any() and (co[:, 1] == -180).any()
    assert (co[:, 2] == 0).any() and (co[:, 2] < 0).any()
    near = np.hypot(co[:, 0][:, None] - g["lats"][None], co[:, 1][:, None] - g["lons"][None]).min()
    assert near < 1e-3
    assert np.array_equal(g["los0"][:3], np.eye(3))


def test_names_and_config():
    from beat_amd.models.corrections import EulerPoleConfig, EulerPoleCorrection
    cfg = EulerPoleConfig(dataset_names=["gnss"], enabled=True, station_blacklist=["A"], station_whitelist=["B"])
    assert cfg.get_suffixes() == SUFFIXES and cfg.station_blacklist == ["A"] and cfg.station_whitelist == ["B"]
    assert cfg.get_hierarchical_names(name="gnss", number=3) == ["3_pole_lat", "3_pole_lon", "3_omega"]
    corr = cfg.init_correction()
    assert isinstance(corr, EulerPoleCorrection) and corr.get_required_coordinate_names() == ["lons", "lats"]
    with pytest.raises(ValueError):
        corr.get_displacements({}, point={"x": 1.0})
    with pytest.raises(AttributeError):
        EulerPoleConfig(enabled=True).init_correction()


def test_get_displacements_vs_reference_and_mpmath():
    g = load_golden("euler_pole")
    worst = [0.0, 0.0]
    for b in range(2):
        corr = _pole(g, b)
        for i, co in enumerate(g["coefs"]):
            point = dict(zip(corr.correction_names, co))
            got = corr.get_displacements({}, point=point)
            bd = eref.bound(co[2], g["earth"], g["los%d" % b])
            for k, want in enumerate((g["disp%d" % b][i], g["mp_disp%d" % b][i])):
                err = np.abs(got - want)
                assert np.all(err <= bd)
                if co[2] != 0.0:
                    ok = bd > 0
                    worst[k] = max(worst[k], float(np.max(err[ok] / bd[ok])) * 16)
            assert np.all(got[g["mask"]] == 0.0)
            # fixed variables come from `hierarchicals` when the point lacks them
            assert np.array_equal(corr.get_displacements(point, point={"other": 1.0}), got)
    print("get_displacements: <= %.2f units from the reference, <= %.2f from mpmath (bound 16)" % tuple(worst))


def test_linear_form_vs_reference_and_mpmath():
    g = load_golden("euler_pole")
    worst = [0.0, 0.0, 0.0]
    wp = eref.omega_prime(g["coefs"][:, 2], g["earth"])
    for b in range(2):
        corr = _pole(g, b)
        B = corr.basis()
        assert B.shape == (72, 3) and np.all(B[g["mask"]] == 0.0)
        for i, co in enumerate(g["coefs"]):
            coef = corr.coefficients(*co)
            assert np.array_equal(coef, eref.coefficients(*co, g["earth"]))
            assert np.all(np.abs(coef - g["mp_coef"][i]) <= 16 * eref.U * wp[i])
            if wp[i] > 0:
                worst[2] = max(worst[2], float(np.max(np.abs(coef - g["mp_coef"][i])) / (eref.U * wp[i])))
            lin = eref.linear(B, coef)
            assert np.array_equal(lin, (B[:, 0] * coef[0] + B[:, 1] * coef[1]) + B[:, 2] * coef[2])
            bd = eref.bound(co[2], g["earth"], g["los%d" % b])
            for k, want in enumerate((g["disp%d" % b][i], g["mp_disp%d" % b][i])):
                err = np.abs(lin - want)
                assert np.all(err <= bd)
                if co[2] != 0.0:
                    ok = bd > 0
                    worst[k] = max(worst[k], float(np.max(err[ok] / bd[ok])) * 16)
    print("linear form: <= %.2f units from the reference, <= %.2f from mpmath; coefficients <= %.2f (bound 16)"
          % tuple(worst))


def test_coefficients_vectorised_and_ref_bitwise():
    from beat_amd.models.corrections import EarthModel, pole_coefficients
    rng = np.random.default_rng(5)
    lat, lon, om = rng.uniform(-90, 90, 200), rng.uniform(-180, 180, 200), rng.uniform(-10, 10, 200)
    for em in (EarthModel(6371.0e3, 6378.14e3, 1 / 298.257223563), EarthModel.sphere(6371.0e3)):
        got = pole_coefficients(lat, lon, om, em)
        assert got.shape == (200, 3) and np.array_equal(got, eref.coefficients(lat, lon, om, em.as_tuple()))
        assert np.array_equal(got[7], pole_coefficients(lat[7], lon[7], om[7], em))


def test_sphere_equals_the_spherical_formula():
    from beat_amd.models.corrections import EarthModel
    g = load_golden("euler_pole")
    em = EarthModel.sphere(6371.0e3)
    assert em.as_tuple() == (6371.0e3, 6371.0e3, 0.0)
    corr = _pole(g, 1, earth=em)
    d2r = np.pi / 180

    def unit(lat, lon):
        return np.stack([np.cos(lat * d2r) * np.cos(lon * d2r), np.cos(lat * d2r) * np.sin(lon * d2r),
                         np.sin(lat * d2r) + 0 * lon], axis=-1)
    x = unit(g["lats"], g["lons"])
    for co in g["coefs"]:
        w = co[2] * 1e-6 * d2r * em.radius
        v = w * np.cross(unit(co[0], co[1])[None, :], x)
        la, lo = g["lats"] * d2r, g["lons"] * d2r
        north = np.stack([-np.sin(la) * np.cos(lo), -np.sin(la) * np.sin(lo), np.cos(la)], axis=1)
        east = np.stack([-np.sin(lo), np.cos(lo), 0 * lo], axis=1)
        down = np.stack([-np.cos(la) * np.cos(lo), -np.cos(la) * np.sin(lo), -np.sin(la)], axis=1)
        neu = np.stack([(north * v).sum(1), (east * v).sum(1), (down * v).sum(1)], axis=1)
        neu[g["mask"]] = 0.0
        want = (neu * g["los1"]).sum(1)
        got = corr.get_displacements({}, point=dict(zip(corr.correction_names, co)))
        assert np.all(np.abs(got - want) <= eref.bound(co[2], em.as_tuple(), g["los1"]))
        # a rigid rotation of a sphere has no radial velocity
        up = corr.velocities(*co)[:, 2]
        assert np.all(np.abs(up) <= 16 * eref.U * abs(w))


def test_earth_model_defaults_documented():
    from beat_amd.models.corrections import EarthModel
    em = EarthModel()
    try:
        from pyrocko import orthodrome
        assert em.as_tuple() == (orthodrome.earthradius, orthodrome.earthradius_equator, orthodrome.earth_oblateness)
    except ImportError:
        assert em.as_tuple() == (6371.0e3, 6378.14e3, 1 / 298.257223563)
    assert "nobody has checked" in EarthModel.__doc__
    assert EarthModel(1.0, 2.0, 0.5).as_tuple() == (1.0, 2.0, 0.5)


def test_correction_tables_order_kinds_and_keyerror():
    from beat_amd.models import ParameterLayout, RampConfig, StrainRateConfig
    from beat_amd.models.corrections import correction_tables
    g = load_golden("euler_pole")
    n = g["lats"].size
    pole, pole2 = _pole(g, 0), _pole(g, 1, number=1)
    ramp = RampConfig(dataset_names=["gnss"], enabled=True).init_correction()
    ramp.setup_correction(np.arange(n) * 1e3, np.arange(n) * 2e3, None, None, "gnss")
    strain = StrainRateConfig(dataset_names=["gnss"], enabled=True).init_correction()
    strain.setup_correction(g["lats"], g["lons"], g["los0"], g["mask"], "gnss", number=0,
                            local_coordinates=(np.arange(n) * 1e3, np.arange(n) * 2e3))
    names = ramp.correction_names + ["0_pole_lat", "0_omega"] + strain.correction_names
    lay = ParameterLayout(OrderedDict([("uparr", 5)] + [(k, 1) for k in names] + [("h_SAR", 1)]))
    fixed = {"0_pole_lon": 171.5, "1_pole_lat": 10.0, "1_pole_lon": 20.0, "1_omega": 0.0}
    # given out of order: the table follows iter_corrections (ramp, Euler poles in the order given, strain rates)
    ds, ncol, basis, off, fix, kind, earth = correction_tables([[strain, pole, ramp, pole2], []], [n, 4], lay, fixed,
                                                               kinds=True)
    assert ds == [0, 0, 0, 0] and ncol == [3, 3, 3, 4] and kind == [0, 1, 1, 0]
    assert off[0] == [5, 6, 7] and off[1] == [8, -1, 9] and off[2] == [-1, -1, -1] and off[3] == [10, 11, 12, 13]
    assert fix[1] == [0.0, 171.5, 0.0] and fix[2] == [10.0, 20.0, 0.0]
    assert earth[0] == (0.0, 0.0, 0.0) and earth[1] == tuple(g["earth"]) and earth[3] == (0.0, 0.0, 0.0)
    assert np.array_equal(basis[1], pole.basis()) and np.array_equal(basis[2], pole2.basis())
    with pytest.raises(KeyError, match="0_pole_lon"):
        correction_tables([[pole], []], [n, 4], lay, {}, kinds=True)
    # five lists cannot describe a pole term
    with pytest.raises(ValueError, match="kinds=True"):
        correction_tables([[pole], []], [n, 4], lay, fixed)
    assert len(correction_tables([[ramp, strain], []], [n, 4], lay, fixed)) == 5


def test_kind_argument_rules_of_the_binding():
    """the rules of the ..._kinds entry that need no model, as the binding checks them ahead of the call (the library's
    own checks, and the offsets against q, are GPU tests: they need a context)"""
    from beat_amd.engine import Context
    e = (6371.0e3, 6378.14e3, 1 / 298.257223563)
    kd, ea = Context.check_correction_kinds([3, 4, 3], [0, 0, 1], [(0, 0, 0), (0, 0, 0), e])
    assert kd.dtype == np.int32 and list(kd) == [0, 0, 1] and ea.shape == (3, 3) and tuple(ea[2]) == e
    for ncol, kind, earth, msg in [([3], [2], [e], "unknown kind"), ([3], [-1], [e], "unknown kind"),
                                   ([2], [1], [e], "not 3"), ([4], [1], [e], "not 3"),
                                   ([3], [1], [(0.0, 1.0, 0.0)], "earth"), ([3], [1], [(1.0, -1.0, 0.0)], "earth"),
                                   ([3], [1], [(1.0, 1.0, 1.0)], "earth"), ([3, 3], [1], [e], "kinds"),
                                   ([3], [1], [e, e], "earth constants")]:
        with pytest.raises(ValueError, match=msg):
            Context.check_correction_kinds(ncol, kind, earth)


def test_config_classes_are_siblings():
    from beat_amd.models.corrections import EulerPoleConfig, GNSSCorrectionConfig, StrainRateConfig
    assert issubclass(EulerPoleConfig, GNSSCorrectionConfig) and issubclass(StrainRateConfig, GNSSCorrectionConfig)
    assert not issubclass(EulerPoleConfig, StrainRateConfig)


def test_backslip2coupling_restatement_bitwise():
    g = load_golden("euler_pole")
    for i in range(g["coefs"].shape[0]):
        got = eref.backslip2coupling(g["patch_uparr"][i].copy(), g["euler_slips"][i])
        assert np.array_equal(got, g["coupling"][i], equal_nan=True)
    cp = g["coupling"]
    assert np.isnan(cp).any() and (cp == 100).any() and (cp == 0).any() and ((cp > 0) & (cp < 100)).any()


def test_patch_basis_vs_reference_slips():
    from beat_amd.models.corrections import EarthModel
    from beat_amd.summary import pole_patch_basis
    g = load_golden("euler_pole")
    sv = g["patch_strikevectors_enu"]
    Bp = pole_patch_basis(g["patch_lats"], g["patch_lons"], sv, EarthModel(*g["earth"]))
    neu = np.stack([sv[:, 1], sv[:, 0], 0 * sv[:, 2]], axis=1)
    for i, co in enumerate(g["coefs"]):
        es = eref.euler_slips(Bp, eref.coefficients(*co, g["earth"]))
        assert np.all(np.abs(es - g["euler_slips"][i]) <= eref.bound(co[2], g["earth"], neu))


def test_symbols_declared_exported_and_bound():
    from beat_amd import _lib
    hdr = open(ROOT + "/include/beat_amd.h").read()
    for name, nargs in (("beatamd_ffi_model_add_geodetic_corrections_kinds", 10), ("beatamd_pole_coefficients_batch", 9),
                        ("beatamd_pole_coupling_batch", 12)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
        assert name in _lib.EXPORTS and len(_lib._PROTOS[name]) == nargs
        assert hasattr(_lib.load(), name)
    assert _lib.ABI_VERSION == 120 and "BEATAMD_VERSION 120" in re.sub(r"\s+", " ", hdr)
