"""The half-space kernels of geometry.hip against values that do not share their arithmetic.

k_geom_disp against tests/golden/okada_mp.npz: Okada (1985) eqs 25-30 and Mogi (1958) evaluated at 60 digits
(oracle/okada_mp.py; tests/test_okada_mp.py pins that reference) and rounded to float64.  The metric is
max |u - u_ref| / |slip| per row; Mogi rows relative to the row's largest |u_ref|.  The bounds, each with its reason:

    dips up to 89 deg and every group but the ladder   1e-11   the arithmetic rounds to <= 2.2e-13 there in a host
                                                               build; the margin is the device's log / atan
    ladder rows at least 0.01 deg from vertical        1e-8    rounding ~ 1e-16 / cos^2(dip): 2.9e-9 at 89.99 deg
    every ladder row, either side of vertical          2e-6    the general expressions round like 1e-16 / cos^2(dip),
                                                               taking a dip for vertical costs < 0.04 |cos dip| slip:
                                                               the two cross near |cos dip| = 1e-5 at about 1e-6
    Mogi                                               1e-13   a handful of roundings

The kernel met these bounds only after the change that added this file: with Okada's general expressions as printed
an MI355X gave (this file's print-outs, one launch per group) 1.3e-11 at 90.1 deg, and on the ladder 1.7e-13 at 89 deg,
9.6e-12 at 89.9, 1.8e-9 at 89.99, 2.2e-7 at 89.999, 1.4e-6 at 89.9995, 1.4e-5 at 89.9999, 1.3e-3 at 89.99999, 0.30 at
89.999999, 1.5e5 at 90 - 1e-9, 1e-16 at 90, 11 at 90 + 1e-7, 6.2e-7 at 90.0005, 2.9e-7 at 90.001; every other group
<= 4.5e-15 (far field 1000 km: 2.2e-13), Mogi 4.8e-16.  In its present form (rounding ~ 1e-16 / |cos dip|, vertical
I1..I5 up to |cos dip| = 1e-7) the device functions compiled for the host give <= 5.2e-10 on the whole ladder (at the
switch), 1.5e-13 at 89.99 deg, 1.8e-14 at 90.1 deg, 1.3e-15 at 89 deg and the same figures as above elsewhere; on the
device that form has not been measured yet.

k_geom_los at the edges of launch_geom_los's dispatch (the instance with the source constants in LDS holds 48
(chain, source) pairs per workgroup; with fewer observation points every thread computes its own): its synthetics
against the components of k_geom_disp for the same sources, projected on the line of sight in numpy.
"""
from collections import OrderedDict

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.fixture(scope="module")
def fixture_rows():
    g = load_golden("okada_mp")
    return g["group"], g["kind"], g["inputs"], g["u"]


# ------------------------------------------------------------------------------------------------- k_geom_disp
def _device_rows(ctx, kind, rows):
    """(ue, un, uz) of every row from ONE launch: row i is source i at point i of a rows x rows evaluation"""
    nu = np.unique(rows[:, 10])
    assert nu.size == 1 and np.unique(kind).size == 1
    prm = np.ascontiguousarray(rows[:, None, :10])
    out = ctx.halfspace_displacements_batch([int(kind[0])], prm, np.ascontiguousarray(rows[:, 11]),
                                            np.ascontiguousarray(rows[:, 12]), float(nu[0]))
    assert out.shape == (len(rows), 1, len(rows), 3)
    i = np.arange(len(rows))
    d = out[i, 0, i]                                      # (north, east, up)
    return np.stack([d[:, 1], d[:, 0], d[:, 2]], axis=1)


def _errors(kind, rows, u, ref):
    scale = np.abs(ref).max(axis=1) if kind[0] == 1 else np.abs(rows[:, 8])
    return np.abs(u - ref).max(axis=1) / scale


GROUPS = ["prior_box", "prior_box_nu", "far_100", "far_1000", "surface_breaking", "near_q0", "near_xi0", "dip_flat",
          "dip_over", "mogi"]


def test_fixture_groups_are_all_tested(fixture_rows):
    assert sorted(np.unique(fixture_rows[0])) == sorted(GROUPS + ["dip_ladder"])


@pytest.mark.parametrize("group", GROUPS)
def test_displacements_vs_multiprecision(ctx, fixture_rows, group):
    groups, kinds, inputs, ref = fixture_rows
    m = groups == group
    kind, rows, ref = kinds[m], inputs[m], ref[m]
    u = _device_rows(ctx, kind, rows)
    assert np.isfinite(u).all()
    err = _errors(kind, rows, u, ref)
    for dip in np.unique(rows[:, 4]) if group == "dip_over" else [None]:
        sel = rows[:, 4] == dip if dip is not None else slice(None)
        print("k_geom_disp %-17s%s worst %.3g over %d rows" % (group, "" if dip is None else " dip %.9g" % dip,
                                                                err[sel].max(), np.size(err[sel])))
    bound = 1e-13 if group == "mogi" else 1e-11
    assert err.max() <= bound, (group, rows[np.argmax(err)], err.max())


def test_dip_ladder_vs_multiprecision(ctx, fixture_rows):
    """the same six sources and points at dips from 89 deg through vertical to 90.001 deg.  Okada's general expressions
    as printed round like 1e-16 / cos^2(dip) and miss the 2e-6 bound by orders of magnitude from 89.9999 deg on (2e-5
    there, 0.3 at 89.999999 deg, 1e5 at 90 - 1e-9 deg, measured on the kernel that used them): source_disp evaluates
    them in a form that rounds like 1e-16 / |cos dip| and takes the vertical I1..I5 up to |cos dip| = 1e-7"""
    groups, kinds, inputs, ref = fixture_rows
    m = groups == "dip_ladder"
    kind, rows, ref = kinds[m], inputs[m], ref[m]
    u = _device_rows(ctx, kind, rows)
    err = _errors(kind, rows, u, ref)
    dips = np.unique(rows[:, 4])
    assert dips.size == 17
    for dip in dips:
        print("k_geom_disp dip_ladder %.9f (90 %+.3g) worst %.3g" % (dip, dip - 90.0, err[rows[:, 4] == dip].max()))
    assert np.isfinite(u).all()
    away = np.abs(rows[:, 4] - 90.0)
    bound = np.where(rows[:, 4] <= 89.0, 1e-11, np.where(away >= 0.01 - 1e-9, 1e-8, 2e-6))
    assert sorted(np.unique(bound)) == [1e-11, 1e-8, 2e-6]
    bad = err > bound
    assert not bad.any(), list(zip(rows[bad, 4], err[bad], bound[bad]))


# ------------------------------------------------------------------------------------------------- k_geom_los
SOURCE_PARAMS = ("east_shift", "north_shift", "depth", "strike", "dip", "rake", "length", "width", "slip",
                 "opening_fraction")
LOWER = dict(east_shift=-5.0, north_shift=-5.0, depth=0.5, strike=0.0, dip=5.0, rake=-180.0, length=0.5, width=0.5,
             slip=0.01, opening_fraction=-1.0, h_SAR=-2.0)
UPPER = dict(east_shift=5.0, north_shift=5.0, depth=9.0, strike=360.0, dip=85.0, rake=180.0, length=10.0, width=8.0,
             slip=1.0, opening_fraction=1.0, h_SAR=2.0)


def _los_problem(rng, nsrc, nobs, corrections=None, extra=()):
    """every source parameter sampled, one entry per source; rectangular, Mogi, rectangular"""
    from beat_amd.models import GeodeticGeometryProblem, ParameterLayout
    sources = ["rectangular", "mogi", "rectangular"][:nsrc]
    lay = ParameterLayout(OrderedDict([(n, nsrc) for n in SOURCE_PARAMS] + [("h_SAR", 1)] + [(n, 1) for n in extra]))
    east, north = rng.uniform(-15, 15, nobs), rng.uniform(-15, 15, nobs)
    los = rng.standard_normal((nobs, 3))
    los /= np.linalg.norm(los, axis=1)[:, None]
    data, odw = 0.01 * rng.standard_normal(nobs), 0.5 + rng.random(nobs)
    prob = GeodeticGeometryProblem(lay, sources, east, north, los, data, odw, (nobs,), [1.0], [0.0], [("h_SAR", 0)],
                                   corrections=corrections)
    return prob, lay


def _draw(rng, lay, C, nsrc, extra_bounds=None):
    lower, upper = dict(LOWER), dict(UPPER)
    for n, (a, b) in (extra_bounds or {}).items():
        lower[n], upper[n] = a, b
    lo, up = lay.bounds(lower, upper)
    Q = lo + (up - lo) * rng.random((C, lay.size))
    if nsrc > 1:
        Q[:, lay.offset("slip", 1)] *= 1e6              # Mogi volume change [m^3]
    return Q


def _source_params(lay, Q, nsrc):
    return np.ascontiguousarray(np.stack([np.stack([Q[:, lay.offset(n, s)] for n in SOURCE_PARAMS], axis=1)
                                          for s in range(nsrc)], axis=1))


def _own_constants_instance(nsrc, nobs):
    """launch_geom_los: more (chain, source) pairs in a workgroup of 256 (chain, point) pairs than the LDS table of 48"""
    return ((255 + nobs - 1) // nobs + 1) * nsrc > 48


# C * Nobs is no multiple of 256 (but for Nobs = 256); chains straddle workgroups wherever Nobs does not divide 256
@pytest.mark.parametrize("nsrc,nobs,C,own", [(1, 1, 103, True), (1, 5, 103, True), (1, 6, 97, False),
                                             (2, 11, 89, True), (2, 12, 83, False), (3, 16, 61, True),
                                             (3, 17, 79, False), (1, 256, 61, False), (1, 257, 67, False)])
def test_los_synthetics_at_the_dispatch_edges(ctx, nsrc, nobs, C, own):
    """mu of k_geom_los = (un*l0 + ue*l1) + uz*l2 of the sources' summed k_geom_disp components, to 1e-13 of the
    sources' amplitude (25 times the 3.8e-15 two compilations of this arithmetic differ by).  (3, 17) fills the
    table of 48 exactly; (3, 16), (2, 11) and (1, 5) are the first shapes beyond it"""
    assert _own_constants_instance(nsrc, nobs) == own and ((C * nobs) % 256 != 0 or nobs % 256 == 0)
    if not own and nobs < 256:
        assert _own_constants_instance(nsrc, nobs - 1)    # the edge itself
    rng = np.random.default_rng(1000 * nsrc + nobs)
    prob, lay = _los_problem(rng, nsrc, nobs)
    f = prob.compile(ctx)
    Q = _draw(rng, lay, C, nsrc)
    mu = f.geodetic_residuals(Q, residuals=False)
    f.release()
    assert mu.shape == (C, nobs) and np.isfinite(mu).all()
    kinds = [1 if s == "mogi" else 0 for s in prob.sources]
    prm = _source_params(lay, Q, nsrc)
    comp = ctx.halfspace_displacements_batch(kinds, prm, prob.east, prob.north, prob.nu)   # (C, nsrc, nobs, [n, e, up])
    tot = np.zeros((C, nobs, 3))
    scale = np.zeros(C)
    for s in range(nsrc):
        tot += comp[:, s]
        scale += np.abs(comp[:, s]).max(axis=(1, 2)) if kinds[s] else np.abs(prm[:, s, 8])
    l = prob.los
    ref = (tot[:, :, 0] * l[None, :, 0] + tot[:, :, 1] * l[None, :, 1]) + tot[:, :, 2] * l[None, :, 2]
    err = np.abs(mu - ref).max(axis=1) / scale
    print("k_geom_los nsrc %d Nobs %3d C %3d (%s): worst %.3g" % (nsrc, nobs, C, "own" if own else "LDS", err.max()))
    assert np.abs(ref).max() > 1e-4 and err.max() <= 1e-13


def test_own_constants_residual_with_a_ramp_is_numpy_s_bit_for_bit(ctx):
    """k_geom_los<2, false, true> (one source, five points, a ramp): the residual is ((d - mu) * odw) - corr with
    plain products and sums (kernels.hpp, geo_corrected_residual), mu being the uncorrected model's synthetics"""
    import corrections_ref as cref
    from beat_amd.models import RampConfig
    nsrc, nobs, C = 1, 5, 103
    assert _own_constants_instance(nsrc, nobs)
    out = {}
    for ramped in (False, True):                         # the same draws for both models
        rng = np.random.default_rng(77)
        base, _ = _los_problem(np.random.default_rng(77), nsrc, nobs)
        ramp = RampConfig(dataset_names=["scene"], enabled=True).init_correction()
        ramp.setup_correction(base.north * 1e3, base.east * 1e3, None, None, "scene")
        names = list(ramp.correction_names)
        prob, lay = _los_problem(rng, nsrc, nobs, corrections=[[ramp]] if ramped else None, extra=names)
        Q = _draw(rng, lay, C, nsrc, dict((n, (-0.1, 0.1)) for n in names))
        f = prob.compile(ctx)
        out[ramped] = (f.geodetic_residuals(Q, residuals=ramped), Q, prob, lay, ramp, names)
        f.release()
    mu, Q0 = out[False][:2]
    res, Q, prob, lay, ramp, names = out[True]
    assert np.array_equal(Q, Q0)
    want = np.empty_like(res)
    for c in range(C):
        corr = cref.ramp(ramp.north_shifts, ramp.east_shifts, *[Q[c, lay.offset(n)] for n in names])
        want[c] = ((prob.data - mu[c]) * prob.odws) - corr
    assert np.abs(want - (prob.data - mu) * prob.odws).max() > 1e-3      # the ramp is there
    assert np.array_equal(res, want)
