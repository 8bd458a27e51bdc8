"""The multi-precision half-space reference (oracle/okada_mp.py, mpmath at 60 digits) and its fixture
tests/golden/okada_mp.npz: pinned to Okada's (1985) published check values, continuous through the vertical dip, the
fixture reproducible from it; and the float64 oracle (oracle/okada_oracle.py) held to it.  Host only."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import okada_oracle as ok


def _mp():
    pytest.importorskip("mpmath")
    from oracle import okada_mp
    return okada_mp


def test_mp_reference_matches_okada_table2():
    """Okada (1985) Table 2, case 2 (dip 70 deg) and case 3 (vertical fault): the values and the tolerance of
    test_geometry.test_okada85_published_check_values (four published digits)"""
    om = _mp()
    want = {(1, 0, 0): (-8.689e-3, -4.298e-3, -2.747e-3),
            (0, 1, 0): (-4.682e-3, -3.527e-2, -3.564e-2),
            (0, 0, 1): (-2.660e-4, 1.056e-2, 3.214e-3)}
    for U, ref in want.items():
        got = [float(v) for v in om.okada85_local(2.0, 3.0, 4.0, 70.0, 3.0, 2.0, *U)]
        np.testing.assert_allclose(got, ref, rtol=6e-4)
    want90 = {(1, 0, 0): (0.0, 5.253e-3, 0.0), (0, 1, 0): (0.0, 0.0, 0.0),
              (0, 0, 1): (1.223e-2, 0.0, -1.606e-2)}
    for U, ref in want90.items():
        got = [float(v) for v in om.okada85_local(0.0, 0.0, 4.0, 90.0, 3.0, 2.0, *U)]
        np.testing.assert_allclose(got, ref, rtol=6e-4, atol=1e-12)


def test_mp_mogi_closed_form():
    om = _mp()
    ue, un, uz = om.mogi(2.0, 0.0, 0.0, 0.0, 2.0, 1e6)
    assert float(ue / uz) == 1.0 and float(un) == 0.0
    _, _, uz0 = om.mogi(0.0, 0.0, 0.0, 0.0, 2.0, 1e6)
    np.testing.assert_allclose(float(uz0), 0.75 / np.pi * 1e6 / 2000.0 ** 2, rtol=1e-15)


def test_mp_general_formulas_meet_the_vertical_ones():
    """what makes the general-dip formulas at 60 digits the truth near vertical: at 90 - 1e-9 deg they are within
    1e-9 * slip of the vertical-branch result at 90 deg (the field changes by < 0.04 * |cos dip| * slip, and
    |cos dip| = 1.7e-11), on both sides; and 60 digits are enough there -- 100 digits give the same numbers"""
    om = _mp()
    g = load_golden("okada_mp")
    rows = g["inputs"][(g["group"] == "dip_ladder") & (g["inputs"][:, 4] == 90.0)]
    assert len(rows) == 6
    for row in rows:
        es, ns, depth, strike, dip, rake, L, W, slip, f, nu, e, n = [float(v) for v in row]
        u90 = om.rect_source(e, n, es, ns, depth, strike, 90.0, rake, L, W, slip, f, nu)
        for near in (90.0 - 1e-9, 90.0 + 1e-9):
            u = om.rect_source(e, n, es, ns, depth, strike, near, rake, L, W, slip, f, nu)
            u100 = om.rect_source(e, n, es, ns, depth, strike, near, rake, L, W, slip, f, nu, dps=100)
            assert max(abs(a - b) for a, b in zip(u, u90)) <= 1e-9 * abs(slip)
            assert max(abs(a - b) for a, b in zip(u, u100)) <= 1e-30 * abs(slip)


def test_fixture_inputs_are_the_generator_s():
    from oracle import okada_mp as om       # numpy only up to here
    g = load_golden("okada_mp")
    groups, kinds, rows = om.build_rows()
    assert np.array_equal(groups, g["group"]) and np.array_equal(kinds, g["kind"])
    assert np.array_equal(rows, g["inputs"]) and list(g["columns"]) == list(om.COLUMNS)
    # one nu and one kind per group (a group is one launch), the ladder on both sides of the vertical switch
    for name in np.unique(groups):
        m = groups == name
        assert np.unique(rows[m, 10]).size == 1 and np.unique(kinds[m]).size == 1
    cosd = np.abs(np.cos(np.deg2rad(np.array(om.LADDER_DIPS))))
    for side in (np.array(om.LADDER_DIPS) < 90, np.array(om.LADDER_DIPS) > 90):
        inside, outside = cosd[side & (cosd <= ok.VERTICAL_COS)], cosd[side & (cosd > ok.VERTICAL_COS)]
        assert inside.max() > 0.98 * ok.VERTICAL_COS and outside.min() < 1.02 * ok.VERTICAL_COS


def test_fixture_regenerates_to_one_ulp():
    """every fifth row again from the multi-precision reference"""
    om = _mp()
    g = load_golden("okada_mp")
    idx = np.arange(0, g["kind"].size, 5)
    u = om.evaluate_rows(g["kind"][idx], g["inputs"][idx])
    assert np.all(np.abs(u - g["u"][idx]) <= np.spacing(np.abs(g["u"][idx])))
    assert np.isfinite(g["u"]).all()


def vertical_distance_bound(dip):
    """the bound on max |u - u_ref| / |slip| of float64 evaluations, by the distance of the dip from vertical:
    1e-11 up to 89 deg (the general expressions round like 1e-16 / cos^2(dip): 3e-13 at 89 deg), 1e-8 at least
    0.01 deg from vertical (3e-9 there), 2e-6 in between: rounding of the general expressions (1e-16 / cos^2) and the
    vertical expressions' error for a dip that is not vertical (< 0.04 |cos dip|) cross near |cos dip| = 1e-5 at 1e-6"""
    away = np.abs(np.asarray(dip) - 90.0)
    return np.where(away >= 1.0, 1e-11, np.where(away >= 0.01 - 1e-9, 1e-8, 2e-6))


def test_float64_oracle_against_the_fixture():
    """oracle/okada_oracle.py describes the same model as the kernel (vertical I1..I5 up to |cos dip| = 1e-7): its
    distance from the multi-precision values, per row, under the bound of the row's distance from vertical"""
    g = load_golden("okada_mp")
    worst = {}
    for name, kind, row, ref in zip(g["group"], g["kind"], g["inputs"], g["u"]):
        es, ns, depth, strike, dip, rake, L, W, slip, f, nu, e, n = row
        if kind == 1:
            u = np.array(ok.mogi(e, n, es, ns, depth, slip, nu), dtype=np.float64)
            err, bound = np.abs(u - ref).max() / np.abs(ref).max(), 1e-13
        else:
            u = np.array(ok.rect_source(e, n, es, ns, depth, strike, dip, rake, L, W, slip, f, nu), dtype=np.float64)
            err, bound = np.abs(u - ref).max() / abs(slip), float(vertical_distance_bound(dip))
        assert np.isfinite(u).all(), (name, row)
        assert err <= bound, (name, dip, err, bound)
        key = "%s %.9g" % (name, dip) if name in ("dip_ladder", "dip_over") else str(name)
        worst[key] = max(worst.get(key, 0.0), err)
    for k, v in worst.items():
        print("float64 oracle %-28s %.3g" % (k, v))
