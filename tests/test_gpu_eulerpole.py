"""The Euler-pole correction on the device (corrections.py:90-140, heart.py:4326-4392; fault.py:1436-1517): the derived
coefficients (k_pole_coef) against 50-digit values, the FFI and geometry composites and the other consumers of the
correction table against the one-chain host composition with ``EulerPoleCorrection.get_displacements`` (pinned to the
reference's numbers by tests/test_eulerpole_host.py) at the tolerances of tests/test_gpu_corrections.py, parity with
the pole-free model, the fused step, and the coupling map against the reference's ``backslip2coupling`` values.

Observed on an MI355X: k_pole_coef <= 3 of the 16 units 2^-53 |w'| from the mpmath coefficients (the test prints it)."""
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

import eulerpole_ref as eref
import test_gpu_corrections as tc
from conftest import ROOT, load_golden
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

POLE_BOUNDS = {"pole_lat": 90.0, "pole_lon": 180.0, "omega": 10.0}


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


# ------------------------------------------------------------------------------------------------- inputs
def _earth(g):
    from beat_amd.models import EarthModel
    return EarthModel(*g["earth"])


def _pole(lats, lons, los, mask, name, number, earth):
    from beat_amd.models import EulerPoleConfig
    corr = EulerPoleConfig(dataset_names=[name], enabled=True).init_correction()
    corr.setup_correction(lats, lons, los, mask, name, number=number, earth=earth)
    return corr


def _block(rng, n, name):
    """a GNSS-like block of n rows on seeded stations (every fifth row masked) with a full covariance"""
    b = rng.standard_normal((n, n))
    C = 1e-6 * (b @ b.T / n + np.eye(n))
    los = rng.normal(size=(n, 3))
    los /= np.linalg.norm(los, axis=1)[:, None]
    mask = np.arange(n) % 5 == 3
    return dict(name=name, data=2e-2 * rng.standard_normal(n), odw=0.5 + rng.random(n), C=C, W=orc.cov_chol_inverse(C),
                sl=orc.cov_log_pdet(C), lats=rng.uniform(-44.0, -38.0, n), lons=rng.uniform(170.0, 178.0, n), los=los,
                mask=mask, north=rng.uniform(-80e3, 80e3, n), east=rng.uniform(-80e3, 80e3, n))


def _bounds(names):
    lo, up = tc._bounds_for(names)
    for n in names:
        for s, b in POLE_BOUNDS.items():
            if n.endswith("_" + s):
                lo[n], up[n] = -b, b
    return lo, up


def _problem(blocks, corrections, free, fixed=None, seed=1, slips=tc.SLIPS, npatch=tc.NPATCH, laplacian=None):
    """tests/test_gpu_corrections.py's FFI problem over `blocks` with the pole variables' own prior box; optionally a
    laplacian (L, logdet) with h_laplacian"""
    from beat_amd.ffi import GeodeticGFLibrary, GeodeticGFLibraryConfig
    from beat_amd.models import FFIProblem, GeodeticData, ParameterLayout
    rng = np.random.default_rng(seed)
    sizes = [b["data"].size for b in blocks]
    nobs = sum(sizes)
    gfs, Gs = {}, []
    for v in slips:
        gg = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=(npatch, nobs), component=v))
        gg.setup(npatch, nobs, allocate=True)
        gg._gfmatrix[:] = 1e-2 * rng.standard_normal((npatch, nobs))
        gfs[v] = gg
        Gs.append(gg._gfmatrix)
    extra = [("h_laplacian", 1)] if laplacian is not None else []
    lay = ParameterLayout(OrderedDict([(v, npatch) for v in slips] + [(n, 1) for n in free] + [("h_SAR", 1)] + extra))
    lower = dict((v, -1.0) for v in slips)
    upper = dict((v, 1.0) for v in slips)
    clo, cup = _bounds(free)
    lower.update(clo, h_SAR=-1.0)
    upper.update(cup, h_SAR=1.0)
    if laplacian is not None:
        lower["h_laplacian"], upper["h_laplacian"] = 0.5, 1.0
    data = np.concatenate([b["data"] for b in blocks])
    odw = np.concatenate([b["odw"] for b in blocks])
    geo = GeodeticData(gfs, data, odw, sizes, [b["W"] for b in blocks], [b["sl"] for b in blocks],
                       [("h_SAR", 0)] * len(blocks), corrections=corrections, fixed=fixed)
    if laplacian is None:
        prob = FFIProblem(lay, [], [], [], slips, geodetic=geo, lower=lower, upper=upper)
    else:
        prob = FFIProblem(lay, [laplacian[2]], [laplacian[3]], [1.0], list(slips), [], geo, laplacian[:2], lower, upper)
    host = dict(Gs=Gs, data=data, odw=odw, sizes=sizes, W=[b["W"] for b in blocks], sl=[b["sl"] for b in blocks],
                corrections=corrections, fixed=dict(fixed or {}), slips=slips)
    return prob, lay, host


def _ordered(cs):
    return sorted(cs or [], key=lambda c: c.order)


def _corr_value(corr, val):
    """one correction on the host: the pole through get_displacements (the reference's order), the others through
    the numpy restatement of tests/corrections_ref.py"""
    from beat_amd.models import EulerPoleCorrection
    if isinstance(corr, EulerPoleCorrection):
        return corr.get_displacements({}, point=dict((n, val(n)) for n in corr.correction_names))
    return tc._corr_value(corr, val)


def _corrected(res, sizes, corrections, val):
    """residual blocks minus the dataset's corrections one after the other in the reference's order"""
    parts, o = [], 0
    for d, n in enumerate(sizes):
        r = res[o:o + n].copy()
        for c in _ordered((corrections or [[]] * len(sizes))[d]):
            r = r - _corr_value(c, val)
        parts.append(r)
        o += n
    return parts


def _residual_parts(host, lay, q, what="weighted"):
    """the corrected residual blocks: (d - mu) * odw ("weighted"), d - mu ("raw": the noise update's) or d ("data":
    the least-squares right-hand side's)"""
    pt = lay.rmap(q)
    mu = np.zeros(host["data"].size)
    for G, v in zip(host["Gs"], host["slips"]):
        mu += orc.geo_stack(G, pt[v])
    res = {"weighted": (host["data"] - mu) * host["odw"], "raw": host["data"] - mu, "data": host["data"].copy()}[what]

    def val(name):
        return pt[name][0] if name in lay.offsets else host["fixed"][name]
    return _corrected(res, host["sizes"], host["corrections"], val), pt


def _ffi_ref(host, lay, q):
    parts, pt = _residual_parts(host, lay, q)
    out = [orc.mvn_chol_logp(W, r, sl, pt["h_SAR"][0]) for W, r, sl in zip(host["W"], parts, host["sl"])]
    return np.array(out + [sum(out)])


def _three_blocks(seed=3):
    rng = np.random.default_rng(seed)
    return [_block(rng, n, "gnss_%d" % d) for d, n in enumerate((2, 65, 33))]


def _poles_for(blocks, earth, which=(0, 1, 2)):
    return [[_pole(b["lats"], b["lons"], b["los"], b["mask"], b["name"], d, earth)] if d in which else []
            for d, b in enumerate(blocks)]


# ------------------------------------------------------------------------------------------------- k_pole_coef
@pytest.mark.parametrize("C,npole", [(1, 1), (63, 3), (64, 1), (65, 3), (530, 1), (530, 3)])
def test_pole_coef_vs_mpmath(ctx, C, npole):
    """the kernel the model launches, through beatamd_pole_coefficients_batch: every fixture set (forced poles
    included) in a batch of C rows, every variable sampled and each fixed in turn; 16 * 2^-53 * |w'| per coefficient"""
    g = load_golden("euler_pole")
    co, mp, earth = g["coefs"], g["mp_coef"], g["earth"]
    rng = np.random.default_rng(C + npole)
    pick = np.concatenate([np.arange(co.shape[0]), rng.integers(0, co.shape[0], C * npole)])[:C * npole]
    pick = pick.reshape(C, npole)
    np_ = 2 + 3 * npole
    Q = rng.standard_normal((C, np_))
    off = np.array([[2 + 3 * j, 3 + 3 * j, 4 + 3 * j] for j in range(npole)])
    for j in range(npole):
        Q[:, off[j]] = co[pick[:, j]]
    wp = eref.omega_prime(co[pick][..., 2], earth)
    out = ctx.pole_coefficients_batch(Q, off, np.zeros((npole, 3)), np.tile(earth, (npole, 1)))
    assert out.shape == (C, npole, 4) and np.all(out[..., 3] == 0.0)
    err = np.abs(out[..., :3] - mp[pick])
    assert np.all(err <= 16 * eref.U * wp[..., None])
    ok = wp > 0
    print("k_pole_coef C=%d npole=%d: worst %.2f units (bound 16)" % (C, npole, float(np.max(err[ok] / (eref.U * wp[ok][:, None])))))
    assert np.all(out[..., :3][~ok] == 0.0)
    # each variable fixed in turn: the rows that hold the fixed value give the same bits
    for k in range(3):
        v = co[pick[0, 0], k]
        off_k, fix_k = off.copy(), np.zeros((npole, 3))
        off_k[0, k], fix_k[0, k] = -1, v
        Qk = Q.copy()
        Qk[:, off[0, k]] = v
        a = ctx.pole_coefficients_batch(Qk, off, np.zeros((npole, 3)), np.tile(earth, (npole, 1)))
        Qk[:, off[0, k]] = 1e300        # (not read)
        b = ctx.pole_coefficients_batch(Qk, off_k, fix_k, np.tile(earth, (npole, 1)))
        assert np.array_equal(a, b)
    # the sphere is data, not a branch: a = r, f = 0
    sph = np.array([earth[0], earth[0], 0.0])
    s = ctx.pole_coefficients_batch(Q, off, np.zeros((npole, 3)), np.tile(sph, (npole, 1)))
    want = eref.coefficients(co[pick][..., 0], co[pick][..., 1], co[pick][..., 2], sph)
    assert np.all(np.abs(s[..., :3] - want) <= 16 * eref.U * wp[..., None])


# ------------------------------------------------------------------------------------------------- FFI composite
@pytest.fixture(scope="module")
def ffi_poled(ctx):
    g = load_golden("euler_pole")
    blocks = _three_blocks()
    corrs = _poles_for(blocks, _earth(g))
    free = [n for cs in corrs for c in cs for n in c.correction_names]
    prob, lay, host = _problem(blocks, corrs, free)
    return prob, lay, host, prob.compile(ctx, return_rvs=False)


@pytest.mark.parametrize("C", [1, 63, 64, 530])
def test_ffi_pole_terms_vs_one_chain_composition(ctx, ffi_poled, C):
    """datasets of (2, 65, 33) rows, a pole term each (three records per chain): wavefronts inside one chain (scalar
    loads of the records) and straddling chains (per-lane loads); 1 / 63 / 64 / 530 chains grow the record buffer"""
    prob, lay, host, f = ffi_poled
    Q = tc._draw(lay, prob.lower, prob.upper, C, np.random.default_rng(200 + C))
    LL = f.batch(Q)
    assert LL.shape == (C, 4)
    worst = 0.0
    for c in tc._check_chains(C):
        ref = _ffi_ref(host, lay, Q[c])
        worst = max(worst, float(np.max(np.abs(LL[c] - ref) / np.abs(ref))))
        np.testing.assert_allclose(LL[c], ref, rtol=1e-9, atol=1e-9)
    print("ffi pole C=%d: worst relative difference %.3g" % (C, worst))
    host0 = dict(host, corrections=None)
    assert abs(_ffi_ref(host0, lay, Q[0])[-1] - LL[0, -1]) > 1e-3 * abs(LL[0, -1])


def test_ffi_ramp_pole_strain_in_reference_order(ctx):
    """ramp + pole + strain rate on one dataset, handed over out of order: subtracted ramp, pole, strain rate; a pole
    variable and a strain coefficient fixed; a second dataset without terms is bitwise the uncorrected model's"""
    from beat_amd.models import StrainRateConfig
    g = load_golden("euler_pole")
    rng = np.random.default_rng(9)
    blocks = [_block(rng, 65, "gnss"), _block(rng, 33, "other")]
    b = blocks[0]
    ramp = tc._ramp(["gnss"], "gnss", b["north"], b["east"])
    pole = _pole(b["lats"], b["lons"], b["los"], b["mask"], "gnss", 0, _earth(g))
    strain = StrainRateConfig(dataset_names=["gnss"], enabled=True).init_correction()
    strain.setup_correction(b["lats"], b["lons"], b["los"], b["mask"], "gnss", number=0,
                            local_coordinates=(b["north"], b["east"]))
    corrs = [[strain, pole, ramp], []]
    fixed = {"0_pole_lon": 171.25, "0_rotation": -55.0}
    free = ramp.correction_names + ["0_pole_lat", "0_omega"] + strain.correction_names[:3]
    prob, lay, host = _problem(blocks, corrs, free, fixed, seed=4)
    f = prob.compile(ctx)
    C = 70
    Q = tc._draw(lay, prob.lower, prob.upper, C, rng)
    LL = f.batch(Q)
    for c in range(0, C, 3):
        np.testing.assert_allclose(LL[c], _ffi_ref(host, lay, Q[c]), rtol=1e-9, atol=1e-9)
    prob0, _, _ = _problem(blocks, None, free, fixed, seed=4)
    LL0 = prob0.compile(ctx).batch(Q)
    assert np.array_equal(LL[:, 1], LL0[:, 1]) and not np.array_equal(LL[:, 0], LL0[:, 0])


# ------------------------------------------------------------------------------------------------- geometry composite
def _geometry_problem(rng, sizes, two_sources, earth, poled=(True, True), fixed_corr=None, free=None):
    from beat_amd.models import GeodeticGeometryProblem, ParameterLayout
    from test_geometry import _problem as _gproblem
    base, lay0, lower, upper = _gproblem(rng, sizes, two_sources=two_sources)
    corrs, o = [], 0
    for d, n in enumerate(sizes):
        los = rng.normal(size=(n, 3))
        corrs.append([_pole(rng.uniform(36.0, 40.0, n), rng.uniform(20.0, 26.0, n), los, np.arange(n) % 7 == 2,
                            "scene_%d" % d, d, earth)] if poled[d] else [])
        o += n
    allnames = [n for cs in corrs for c in cs for n in c.correction_names]
    free = allnames if free is None else list(free)
    lay = ParameterLayout(OrderedDict(list(lay0.varsizes.items()) + [(n, 1) for n in free]))
    clo, cup = _bounds(free)
    # velocities of metres per year against scenes of centimetres: a narrow omega keeps the likelihood in range
    for n in free:
        if n.endswith("_omega"):
            clo[n], cup[n] = -0.5, 0.5
    lower, upper = dict(lower, **clo), dict(upper, **cup)
    fixed = dict(base.fixed, **(fixed_corr or {}))
    prob = GeodeticGeometryProblem(lay, base.sources, base.east, base.north, base.los, base.data, base.odws, sizes,
                                   base.weights, base.slog_pdets, base.hypers, fixed=fixed, lower=lower, upper=upper,
                                   corrections=corrs if any(poled) else None)
    return prob, lay, lower, upper


def _geom_ref(prob, lay, q):
    """the one-chain geometry composition (the oracle's sources, line of sight, weighted residual, this file's
    corrections, the oracle's MVN) -- tests/test_gpu_corrections.py's with the pole among the terms"""
    from oracle import okada_oracle as ok
    pt = lay.rmap(q)
    mu = np.zeros(prob.east.size)
    for s, kind in enumerate(prob.sources):
        def val(name):
            if name in lay.offsets:
                return pt[name][s if lay.varsizes[name] > 1 else 0]
            return np.atleast_1d(prob.fixed.get(name, 0.0))[min(s, np.size(prob.fixed.get(name, 0.0)) - 1)]
        if kind == "mogi":
            ue, un, uz = ok.mogi(prob.east, prob.north, val("east_shift"), val("north_shift"), val("depth"),
                                 val("slip"), prob.nu)
        else:
            ue, un, uz = ok.rect_source(prob.east, prob.north, val("east_shift"), val("north_shift"), val("depth"),
                                        val("strike"), val("dip"), val("rake"), val("length"), val("width"),
                                        val("slip"), val("opening_fraction"), prob.nu)
        mu += (un * prob.los[:, 0] + ue * prob.los[:, 1]) + uz * prob.los[:, 2]
    res = (prob.data - mu) * prob.odws

    def cval(name):
        return pt[name][0] if name in lay.offsets else float(prob.fixed[name])
    parts = _corrected(res, prob.sizes, prob.corrections, cval)
    out = [orc.mvn_chol_logp(W, r, sl, pt["h_SAR"][0]) for W, r, sl in zip(prob.weights, parts, prob.slog_pdets)]
    return np.array(out + [sum(out)])


@pytest.mark.parametrize("sizes,two,own", [((60, 41), True, False), ((6, 4), True, True)])
def test_geometry_pole_terms_vs_one_chain_composition(ctx, sizes, two, own):
    g = load_golden("euler_pole")
    rng = np.random.default_rng(7 + sizes[0])
    prob, lay, lower, upper = _geometry_problem(rng, sizes, two, _earth(g))
    assert tc._own_constants_instance(prob) == own
    f = prob.compile(ctx)
    for C in (1, 63, 64, 530):
        Q = tc._draw(lay, lower, upper, C, rng)
        Q[:, lay.offset("slip", 1)] *= 1e6  # Mogi volume change [m^3]
        LL = f.batch(Q)
        assert LL.shape == (C, len(sizes) + 1)
        for c in list(range(0, C, 53)) + [C - 1]:
            np.testing.assert_allclose(LL[c], _geom_ref(prob, lay, Q[c]), rtol=1e-9)
    f.release()


# ------------------------------------------------------------------------------------------------- parity
def test_omega_zero_is_bitwise_the_uncorrected_model_and_kind0_the_old_entry(ctx):
    g = load_golden("euler_pole")
    blocks = _three_blocks()
    corrs = _poles_for(blocks, _earth(g))
    fixed = {}
    for cs in corrs:
        for c in cs:
            fixed.update(dict(zip(c.correction_names, (33.0, -120.0, 0.0))))
    rng = np.random.default_rng(12)
    LLs = []
    for corrections, fx in [(None, None), (corrs, fixed)]:
        prob, lay, _ = _problem(blocks, corrections, [], fx)
        f = prob.compile(ctx)
        if not LLs:
            Q = tc._draw(lay, prob.lower, prob.upper, 530, rng)
        LLs.append(f.batch(Q).copy())
        f.release()
    assert np.isfinite(LLs[0]).all() and np.array_equal(LLs[0], LLs[1])
    # a table of kind-0 terms through the new entry is the model built through the old entry, bit for bit
    from beat_amd.models.corrections import correction_tables
    sc = tc.scenes()
    names = [s["name"] for s in sc]
    ramps = [[tc._ramp(names, s["name"], s["north"], s["east"])] for s in sc]
    free = [n for cs in ramps for c in cs for n in c.correction_names]
    out = []
    for kinds in (False, True):
        prob, lay, _ = tc._ffi_problem(sc, None, free)
        f = prob.compile(ctx)
        ctx.ffi_model_add_geodetic_corrections(f.model_id, *correction_tables(ramps, prob.geodetic.sizes, lay, kinds=kinds))
        Q = tc._draw(lay, prob.lower, prob.upper, 300, np.random.default_rng(13))
        out.append(f.batch(Q).copy())
        f.release()
    assert np.isfinite(out[0]).all() and np.array_equal(out[0], out[1])


def test_c_abi_rejects_bad_pole_tables(ctx):
    g = load_golden("euler_pole")
    blocks = _three_blocks()
    prob0, lay0, _ = _problem(blocks, None, [])
    B = np.ones((65, 3))
    e = [tuple(g["earth"])]
    for args, msg in [(([1], [3], [B], [[-1] * 3], [[0.0] * 3], [2], e), "unknown kind"),
                      (([1], [2], [B[:, :2]], [[-1] * 2], [[0.0] * 2], [1], e), "not 3"),
                      (([1], [3], [B], [[0, 1, 10 ** 6]], [[0.0] * 3], [1], e), "outside q"),
                      (([1], [3], [B], [[-1] * 3], [[0.0] * 3], [1], [(0.0, 1.0, 0.0)]), "earth")]:
        f0 = prob0.compile(ctx)
        with pytest.raises(ValueError, match=msg):
            ctx.ffi_model_add_geodetic_corrections(f0.model_id, *args)
        f0.release()
    # the library's own checks, behind the ones the Python binding makes first
    import ctypes
    from beat_amd import _lib
    for nc, kd, msg in ((3, 2, b"unknown kind"), (2, 1, b"not 3")):
        f0 = prob0.compile(ctx)
        ds, ncs, kds = np.ones(1, np.int32), np.array([nc], np.int32), np.array([kd], np.int32)
        off, fix, ea = -np.ones(4, np.int64), np.zeros(4), np.array(e[0])
        rc = ctx._lib.beatamd_ffi_model_add_geodetic_corrections_kinds(
            ctx._h, f0.model_id, 1, _lib.ptr(ds), _lib.ptr(ncs), _lib.ptr(np.ones(65 * 3)), _lib.ptr(off), _lib.ptr(fix),
            _lib.ptr(kds), _lib.ptr(ea))
        assert rc == _lib.EINVAL and msg in ctypes.c_char_p(ctx._lib.beatamd_last_error()).value
        f0.release()
    with pytest.raises(ValueError, match="outside q"):
        ctx.pole_coefficients_batch(np.zeros((2, 4)), [[0, 1, 4]], [[0.0] * 3], e)
    with pytest.raises(ValueError, match="outside q"):
        ctx.pole_coupling_batch(np.zeros((2, 4)), [0, 1, 2], [0.0] * 3, e[0], np.ones((3, 3)), 2)


# ------------------------------------------------------------------------------------------------- fused step
def test_fused_step_with_a_pole_term(ctx):
    """40 Metropolis steps through the fused step: every step's decisions and likelihood bookkeeping equal the host
    composition chain by chain; a proposal whose omega leaves the prior box is parked and rejected"""
    g = load_golden("euler_pole")
    blocks = _three_blocks()
    corrs = _poles_for(blocks, _earth(g), which=(1,))
    free = corrs[1][0].correction_names
    prob, lay, host = _problem(blocks, corrs, free, slips=("uparr",), npatch=6)
    f = prob.compile(ctx)
    lo, up = lay.bounds(prob.lower, prob.upper)
    rng = np.random.default_rng(17)
    C = 24
    Q = tc._draw(lay, prob.lower, prob.upper, C, rng)
    L = f.batch(Q)
    beta = 1e-4
    ioff = lay.offset("1_omega")
    n_acc = 0
    for step in range(40):
        delta = rng.standard_normal((C, lay.size)) * (up - lo) * 0.02
        parked = step % C
        delta[parked] = 0.0
        delta[parked, ioff] = 45.0          # omega alone leaves [-10, 10] at every scaling >= 0.5
        scaling = rng.uniform(0.5, 1.5, C)
        log_u = np.log(rng.random(C))
        Q0, L0 = Q.copy(), L.copy()
        acc = f.astep_batch(Q, L, delta, scaling, lo, up, log_u, beta)
        for c in range(C):
            q = Q0[c] + delta[c] * scaling[c]
            a_ref = False
            if np.all((q >= lo) & (q <= up)):
                lp = _ffi_ref(host, lay, q)
                a_ref = orc.metrop_accept(beta, lp[-1], L0[c, -1], log_u[c])
            assert bool(acc[c]) == a_ref, (step, c)
            if a_ref:
                np.testing.assert_array_equal(Q[c], q)
                np.testing.assert_allclose(L[c], lp, rtol=1e-9)
            else:
                assert np.array_equal(Q[c], Q0[c]) and np.array_equal(L[c], L0[c])
            n_acc += a_ref
        assert acc[parked] == 0
    assert 0 < n_acc < 40 * C
    np.testing.assert_allclose(f.batch(Q), L, rtol=1e-12)


def test_fused_step_graph_replay_equals_the_eager_loop(ctx):
    """graph replay bitwise the eager loop; the second pair runs more chains than the first, so the record buffer grows
    between captures (in the eager step ahead of the capture)"""
    import torch
    from beat_amd.sampler import SMC
    g = load_golden("euler_pole")
    prob, lay, lower, upper = _geometry_problem(np.random.default_rng(19), (60, 41), False, _earth(g))
    f = prob.compile(ctx)
    lo, up = lay.bounds(lower, upper)
    dev = torch.device("cuda", 0)
    for n_chains in (128, 320):
        out = {}
        for use_graph in (False, True):
            step = SMC(f, lo, up, n_chains=n_chains, tune_interval=7, device=dev, random_seed=2, use_graph=use_graph)
            Q = step.initialize_population()
            L = step.stepper.evaluate(Q)
            step.select_end_points(Q, L)
            step.transition()
            step.stage += 1
            Q, L = step.sample_stage(40)
            torch.cuda.synchronize()
            out[use_graph] = (Q.cpu().numpy(), L.cpu().numpy(), list(step.stage_acceptance))
        (Qa, La, acca), (Qb, Lb, accb) = out[False], out[True]
        assert np.array_equal(Qa, Qb) and np.array_equal(La, Lb) and acca == accb
        assert np.isfinite(La[:, -1]).all() and 0.0 < acca[-1] < 1.0
        np.testing.assert_allclose(La[5], _geom_ref(prob, lay, Qa[5]), rtol=1e-9)


def _run_shard(nproc, mode, out):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "BEATAMD_GF_SPLIT"):
        env.pop(k, None)
    env.update(BEATAMD_TEST_OUT=out, BEATAMD_TEST_MODE=mode, OMP_NUM_THREADS="1")
    worker = os.path.join(ROOT, "tests", "_shard_pole_gpu_worker.py")
    if nproc == 1:
        cmd = [sys.executable, worker]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(tc._free_port()), worker]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("SHARD_POLE_WORKER_OK") == nproc, r.stdout[-2000:]
    return np.load(out)


def test_pole_term_beside_a_target_sharded_wavemap(tmp_path):
    """the replicated geodetic composite takes its pole term along: 2 ranks give the replicated model's likelihood
    vectors bit for bit, and those differ from the uncorrected model's in the pole dataset's column (and `like`) only"""
    rep = _run_shard(1, "replicated", str(tmp_path / "rep.npz"))
    two = _run_shard(2, "targets", str(tmp_path / "two.npz"))
    assert rep["LL"].shape == two["LL"].shape == (300, 9) and np.isfinite(rep["LL"]).all()
    assert np.array_equal(rep["LL"], two["LL"])
    assert np.array_equal(rep["LL"][:, :6], rep["LL_plain"][:, :6]) and np.array_equal(rep["LL"][:, 7], rep["LL_plain"][:, 7])
    assert not np.array_equal(rep["LL"][:, 6], rep["LL_plain"][:, 6])


# ------------------------------------------------------------------------------------------------- other consumers
@pytest.mark.parametrize("C", [1, 64, 530])
def test_update_llks_and_residuals_vs_one_chain_composition(ctx, ffi_poled, C):
    prob, lay, host, f = ffi_poled
    Q = tc._draw(lay, prob.lower, prob.upper, C, np.random.default_rng(300 + C))
    llks = f.update_llks(Q)
    res = f.geodetic_residuals(Q, residuals=True)
    assert llks.shape == (C, 3) and res.shape == (C, sum(host["sizes"]))
    for c in tc._check_chains(C):
        parts, _ = _residual_parts(host, lay, Q[c])
        ref = np.concatenate(parts)
        np.testing.assert_allclose(res[c], ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())
        np.testing.assert_allclose(llks[c], [float((W @ r) @ (W @ r)) for W, r in zip(host["W"], parts)], rtol=1e-9)


def test_noise_update_residual_takes_the_pole_off(ctx, ffi_poled):
    """GeodeticNoiseCovarianceUpdate.residuals: d - mu - corrections without odw, the pole's three coefficients derived on
    the host by the statement the device kernel follows"""
    from beat_amd.covariance import GeodeticNoiseCovarianceUpdate
    prob, lay, host, f = ffi_poled
    upd = GeodeticNoiseCovarianceUpdate(f, [np.zeros((n, 2)) for n in host["sizes"]], [None] * 3, 0.2, typs=["GNSS"] * 3)
    q = tc._draw(lay, prob.lower, prob.upper, 1, np.random.default_rng(77))[0]
    res = upd.residuals(q).cpu().numpy()
    ref = np.concatenate(_residual_parts(host, lay, q, what="raw")[0])
    np.testing.assert_allclose(res, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())
    plain = np.concatenate(_residual_parts(dict(host, corrections=None), lay, q, what="raw")[0])
    assert np.max(np.abs(res - plain)) > 1e-3 * np.abs(plain).max()


def test_lsq_right_hand_side_with_a_pole_term(ctx):
    """b = G (d - corr) of the least-squares start (launch_lsq_finish): geodetic composite with a pole term and a
    laplacian, no seismic rows"""
    from beat_amd.synthetic import smoothing_operator_nearest_neighbor
    g = load_golden("euler_pole")
    blocks = _three_blocks()[1:]
    corrs = _poles_for(blocks, _earth(g), which=(0,))
    free = corrs[0][0].correction_names
    nd, ns = 2, 3
    Lm = smoothing_operator_nearest_neighbor(ns, nd, 1.0, 1.0)
    prob, lay, host = _problem(blocks, corrs, free, slips=("uparr", "uperp"), npatch=nd * ns, laplacian=(Lm, 0.0, nd, ns))
    f = prob.compile(ctx)
    for C in (1, 67):
        Q = tc._draw(lay, prob.lower, prob.upper, C, np.random.default_rng(400 + C))
        Nm, b = f.lsq_normal_equations(Q)
        assert b.shape == (C, nd * ns)
        for c in range(C):
            parts, _ = _residual_parts(host, lay, Q[c], what="data")
            r = np.concatenate(parts)
            ref = host["Gs"][0] @ r
            tol = 1e-9 * (np.abs(host["Gs"][0]) @ np.abs(r))
            assert np.all(np.abs(b[c] - ref) <= tol)
    # the pole matters
    r0 = host["Gs"][0] @ host["data"]
    assert np.max(np.abs(b[0] - r0)) > 1e-6 * np.max(np.abs(r0))
    f.release()


# ------------------------------------------------------------------------------------------------- end to end
def test_smc_recovers_a_known_poles_velocity_field(ctx):
    """wiring, not accuracy: 24 stations x 3 components, data = G . slip + the velocity field of a known pole + noise;
    SMC with 256 chains.  pole_lat / pole_lon trade off against omega (and the antipodal pole with -omega is the same
    rotation), so the criterion of the ramp test is applied to the correction itself: per unmasked row the posterior
    mean of the correction lies within 3 posterior standard deviations of the truth, and its posterior spread is
    under half its spread over the prior.  The network spans a plate (80 x 80 degrees), not the few degrees of the
    fixture's: over a small aperture the pole's position and rate trade off along a long curved ridge, which is a
    test of the sampler's mixing in 30 steps per stage, not of this wiring (on the fixture's network, 1 mm noise:
    worst |z| = 12 at a posterior / prior spread of 1.4e-3)"""
    import torch
    from beat_amd.models.corrections import pole_coefficients
    from beat_amd.sampler import SMC, smc_sample
    g = load_golden("euler_pole")
    rng = np.random.default_rng(23)
    n = g["lats"].size
    sigma = 5e-3
    blk = dict(name="gnss", data=np.zeros(n), odw=np.ones(n), W=np.eye(n) / sigma, sl=2 * n * np.log(sigma),
               lats=np.repeat(rng.uniform(-60.0, 20.0, n // 3), 3), lons=np.repeat(rng.uniform(100.0, 180.0, n // 3), 3),
               los=g["los1"], mask=g["mask"])
    pole = _pole(blk["lats"], blk["lons"], blk["los"], blk["mask"], "gnss", 0, _earth(g))
    prob, lay, host = _problem([blk], [[pole]], pole.correction_names, slips=("uparr",), npatch=3, seed=6)
    prob.lower.update(h_SAR=-0.5)
    prob.upper.update(h_SAR=0.5)
    truth = {"uparr": np.array([0.3, -0.2, 0.5]), "0_pole_lat": 48.0, "0_pole_lon": -95.0, "0_omega": 0.7, "h_SAR": 0.0}
    qt = lay.map(truth)
    corr_t = pole.get_displacements({}, point=truth)
    data = orc.geo_stack(host["Gs"][0], truth["uparr"]) + corr_t + sigma * rng.standard_normal(n)
    prob.geodetic.data = np.ascontiguousarray(data)
    host["data"] = data
    f = prob.compile(ctx)
    lo, up = lay.bounds(prob.lower, prob.upper)
    np.testing.assert_allclose(f.batch(qt[None])[0], _ffi_ref(host, lay, qt), rtol=1e-9)
    step = SMC(f, lo, up, n_chains=256, tune_interval=10, device=torch.device("cuda", 0), random_seed=5)
    pop, lp, betas = smc_sample(30, step)
    assert betas[-1] == 1.0 and np.isfinite(lp).all() and np.all((pop >= lo) & (pop <= up))
    B = pole.basis()
    o = [lay.offset(k) for k in pole.correction_names]
    post = pole_coefficients(pop[:, o[0]], pop[:, o[1]], pop[:, o[2]], pole.earth) @ B.T        # (chains, n)
    prior = pole_coefficients(*[rng.uniform(lo[k], up[k], 4096) for k in o], pole.earth) @ B.T
    rows = ~g["mask"]
    z = (post.mean(0)[rows] - corr_t[rows]) / post.std(0)[rows]
    print("pole field: worst |z| = %.2f; posterior / prior spread <= %.3g" % (np.abs(z).max(),
                                                                            (post.std(0)[rows] / prior.std(0)[rows]).max()))
    assert np.all(np.abs(z) < 3.0)
    assert np.all(post.std(0)[rows] < 0.5 * prior.std(0)[rows])


# ------------------------------------------------------------------------------------------------- coupling
@pytest.mark.parametrize("P", [1, 63, 65])
def test_coupling_vs_reference_values(ctx, P):
    from beat_amd.summary import pole_patch_basis
    g = load_golden("euler_pole")
    earth = g["earth"]
    sv = g["patch_strikevectors_enu"][:P]
    Bp = pole_patch_basis(g["patch_lats"][:P], g["patch_lons"][:P], sv, _earth(g))
    neu = np.stack([sv[:, 1], sv[:, 0], 0 * sv[:, 2]], axis=1)
    co, up = g["coefs"], g["patch_uparr"][:, :P]
    ns = co.shape[0]
    Q = np.ascontiguousarray(np.hstack([np.zeros((ns, 2)), up, co]))
    off = [2 + P, 3 + P, 4 + P]
    es, cp = ctx.pole_coupling_batch(Q, off, [0.0] * 3, earth, Bp, 2)
    assert es.shape == cp.shape == (ns, P)
    ref_es, ref_cp = g["euler_slips"][:, :P], g["coupling"][:, :P]
    for i in range(ns):
        assert np.all(np.abs(es[i] - ref_es[i]) <= eref.bound(co[i, 2], earth, neu))
    # the clip and the IEEE cases are those of numpy's lines on the device's own slips, bit for bit ...
    assert np.array_equal(cp, eref.backslip2coupling(up.copy(), es), equal_nan=True)
    # ... and the reference's wherever its ratio is away from the clip's edges (there a last-bit difference of the
    # slips cannot change the branch): saturated and zero values exactly, the others through the slips' bound
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = up / ref_es
    sat = (ratio > 1.001) | (ratio < -0.001) | np.isnan(ratio)
    assert np.array_equal(cp[sat], ref_cp[sat], equal_nan=True)
    inner = (ratio > 0.001) & (ratio < 0.999)
    np.testing.assert_allclose(cp[inner], ref_cp[inner], rtol=1e-9)
    zero = co[:, 2] == 0.0                       # omega = 0: zero Euler slip -> 100 / 0 / NaN
    assert zero.any() and np.all(es[zero] == 0.0)
    assert np.all(cp[zero][up[zero] > 0] == 100.0) and np.all(cp[zero][up[zero] < 0] == 0.0)
    if P > 3:
        assert np.isnan(cp[zero][:, 3]).all()    # 0 / 0
    assert (up < 0).any() and np.all(cp[up < 0] == 0.0)


def test_coupling_split_calls_are_bitwise_one_call_and_ensemble(ctx, ffi_poled):
    from types import SimpleNamespace

    from beat_amd.models import ParameterLayout
    from beat_amd.summary import coupling_ensemble, pole_patch_basis
    g = load_golden("euler_pole")
    P = 65
    Bp = pole_patch_basis(g["patch_lats"], g["patch_lons"], g["patch_strikevectors_enu"], _earth(g))
    rng = np.random.default_rng(31)
    C = 530
    lay = ParameterLayout(OrderedDict([("uparr", P), ("0_pole_lat", 1), ("0_omega", 1)]))
    Q = np.ascontiguousarray(np.hstack([rng.uniform(-0.01, 0.06, (C, P)), rng.uniform(-90, 90, (C, 1)),
                                        rng.uniform(-10, 10, (C, 1))]))
    off, fix = [P, -1, P + 1], [0.0, 174.5, 0.0]
    es, cp = ctx.pole_coupling_batch(Q, off, fix, g["earth"], Bp, 0)
    parts = [ctx.pole_coupling_batch(np.ascontiguousarray(Q[a:b]), off, fix, g["earth"], Bp, 0)
             for a, b in ((0, 1), (1, 65), (65, 530))]
    assert np.array_equal(es, np.concatenate([p[0] for p in parts]))
    assert np.array_equal(cp, np.concatenate([p[1] for p in parts]))
    f = SimpleNamespace(ctx=ctx, problem=SimpleNamespace(layout=lay, geodetic=SimpleNamespace(fixed={"0_pole_lon": 174.5})))
    out = coupling_ensemble(f, Q, Bp, ("0_pole_lat", "0_pole_lon", "0_omega"), earth=_earth(g), batch=200)
    assert np.array_equal(out["coupling"], cp) and np.array_equal(out["euler_slips"], es)
    np.testing.assert_allclose(out["mean"], cp.mean(0), rtol=1e-12)
    np.testing.assert_allclose(out["std"], cp.std(0), rtol=1e-9)
    with pytest.raises(KeyError, match="1_omega"):
        coupling_ensemble(f, Q, Bp, ("0_pole_lat", "0_pole_lon", "1_omega"))
