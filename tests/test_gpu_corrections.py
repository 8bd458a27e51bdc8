"""Hierarchical dataset corrections of the geodetic likelihood on the device (geodetic.py:1072-1077, 411-427;
corrections.py:46-87, 143-205): the FFI composite (k_geo_residual) and the geometry composite (the residual epilogue
of k_geom_los) against the one-chain composition -- the existing oracle functions for mu and the MVN, the numpy
restatement of the corrections (tests/corrections_ref.py, pinned to the reference's numbers by the CPU tests) in
between -- at the tolerances of the neighbouring tests: rtol = atol = 1e-9 (test_ffi_logp_batch_vs_oracle) and
rtol = 1e-9 (tests/test_geometry.py)."""
import os
import socket
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

import corrections_ref as cref
from conftest import ROOT, load_golden
from oracle import okada_oracle as ok
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SLIPS = ("uparr", "uperp", "utens")
NPATCH = 24


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


# ------------------------------------------------------------------------------------------------- inputs
def _scenes():
    """the Laquila scenes with their full covariances and the local coordinates geo_corrections.npz records"""
    g, gc = load_golden("laquila_geodetic"), load_golden("geo_corrections")
    out = []
    for d in range(2):
        C = g["d%d_C" % d]
        out.append(dict(name=str(gc["ramp_names"][d]), data=g["d%d_displacement" % d], odw=g["d%d_odw" % d], C=C,
                        W=orc.cov_chol_inverse(C), sl=orc.cov_log_pdet(C), east=gc["ramp%d_east_shifts" % d],
                        north=gc["ramp%d_north_shifts" % d], los=g["d%d_los" % d]))
    return out


_SCENES = None


def scenes():
    global _SCENES
    if _SCENES is None:
        _SCENES = _scenes()
    return _SCENES


def _ramp(names, name, north, east):
    from beat_amd.models import RampConfig
    corr = RampConfig(dataset_names=names, enabled=True).init_correction()
    corr.setup_correction(north, east, None, None, name)
    return corr


def _gnss_block(rng):
    """a synthetic GNSS block on the stations of the strain-rate fixture (masked stations included)"""
    from beat_amd.models import StrainRateConfig
    gc = load_golden("geo_corrections")
    n = gc["strain_mask"].size
    b = rng.standard_normal((n, n))
    C = b @ b.T / n + np.eye(n)
    strain = StrainRateConfig(dataset_names=["gnss"], enabled=True).init_correction()
    strain.setup_correction(gc["strain_lats"], gc["strain_lons"], gc["strain1_los"], gc["strain_mask"], "gnss", number=0,
                            local_coordinates=(gc["strain_norths"], gc["strain_easts"]))
    return dict(name="gnss", data=1e-3 * rng.standard_normal(n), odw=0.5 + rng.random(n), C=C,
                W=orc.cov_chol_inverse(C), sl=orc.cov_log_pdet(C), east=gc["strain_easts"], north=gc["strain_norths"],
                los=gc["strain1_los"]), strain


def _corr_value(corr, val):
    """one correction through the numpy restatement; val(name) -> coefficient"""
    from beat_amd.models import RampCorrection
    co = [val(n) for n in corr.correction_names]
    if isinstance(corr, RampCorrection):
        return cref.ramp(corr.north_shifts, corr.east_shifts, *co)
    return cref.strain_rate(corr.norths, corr.easts, corr.los_vector, corr.data_mask, *co)


def _corrected(res, sizes, corrections, val):
    parts, o = [], 0
    for n in sizes:
        parts.append(res[o:o + n])
        o += n
    corrs = [[_corr_value(c, val) for c in (cs or [])] for cs in (corrections or [[]] * len(sizes))]
    return cref.apply_corrections(parts, corrs)


def _bounds_for(names):
    lo, up = {}, {}
    for n in names:
        if n.endswith("_ramp"):
            lo[n], up[n] = -0.1, 0.1
        elif n.endswith("_offset"):
            lo[n], up[n] = -0.05, 0.05
        else:
            lo[n], up[n] = -200.0, 200.0
    return lo, up


# ------------------------------------------------------------------------------------------------- FFI composite
def _ffi_problem(blocks, corrections, free, fixed=None, seed=1):
    """FFI problem with a geodetic composite over `blocks` (scene dicts), three slip variables; `free`: names of the
    correction variables that are sampled"""
    from beat_amd.ffi import GeodeticGFLibrary, GeodeticGFLibraryConfig
    from beat_amd.models import FFIProblem, GeodeticData, ParameterLayout
    rng = np.random.default_rng(seed)
    sizes = [b["data"].size for b in blocks]
    nobs = sum(sizes)
    gfs, Gs = {}, []
    for v in SLIPS:
        gg = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=(NPATCH, nobs), component=v))
        gg.setup(NPATCH, nobs, allocate=True)
        gg._gfmatrix[:] = 1e-2 * rng.standard_normal((NPATCH, nobs))
        gfs[v] = gg
        Gs.append(gg._gfmatrix)
    lay = ParameterLayout(OrderedDict([(v, NPATCH) for v in SLIPS] + [(n, 1) for n in free] + [("h_SAR", 1)]))
    lower = dict((v, -1.0) for v in SLIPS)
    upper = dict((v, 1.0) for v in SLIPS)
    clo, cup = _bounds_for(free)
    lower.update(clo, h_SAR=-1.0)
    upper.update(cup, h_SAR=1.0)
    data = np.concatenate([b["data"] for b in blocks])
    odw = np.concatenate([b["odw"] for b in blocks])
    geo = GeodeticData(gfs, data, odw, sizes, [b["W"] for b in blocks], [b["sl"] for b in blocks],
                       [("h_SAR", 0)] * len(blocks), corrections=corrections, fixed=fixed)
    prob = FFIProblem(lay, [], [], [], SLIPS, geodetic=geo, lower=lower, upper=upper)
    host = dict(Gs=Gs, data=data, odw=odw, sizes=sizes, W=[b["W"] for b in blocks], sl=[b["sl"] for b in blocks],
                corrections=corrections, fixed=dict(fixed or {}))
    return prob, lay, host


def _ffi_ref(host, lay, q):
    pt = lay.rmap(q)
    mu = np.zeros(host["data"].size)
    for G, v in zip(host["Gs"], SLIPS):
        mu += orc.geo_stack(G, pt[v])
    res = (host["data"] - mu) * host["odw"]

    def val(name):
        return pt[name][0] if name in lay.offsets else host["fixed"][name]
    parts = _corrected(res, host["sizes"], host["corrections"], val)
    out = [orc.mvn_chol_logp(W, r, sl, pt["h_SAR"][0]) for W, r, sl in zip(host["W"], parts, host["sl"])]
    return np.array(out + [sum(out)])


def _draw(lay, lower, upper, C, rng):
    lo, up = lay.bounds(lower, upper)
    return lo + (up - lo) * rng.random((C, lay.size))


def _check_chains(C):
    return range(C) if C <= 64 else sorted(set(list(range(0, C, 11)) + [63, 64, 65, C - 2, C - 1]))


@pytest.fixture(scope="module")
def ffi_ramped(ctx):
    sc = scenes()
    names = [s["name"] for s in sc]
    corrs = [[_ramp(names, s["name"], s["north"], s["east"])] for s in sc]
    free = [n for cs in corrs for c in cs for n in c.correction_names]
    prob, lay, host = _ffi_problem(sc, corrs, free)
    return prob, lay, host, prob.compile(ctx, return_rvs=False)


@pytest.mark.parametrize("C", [1, 63, 64, 530])
def test_ffi_both_scenes_ramped_vs_one_chain_composition(ctx, ffi_ramped, C):
    """1 / 63 / 64 / 530 chains: both chain tiles of k_geo_stack and a ragged last block of k_geo_residual; wavefronts
    inside one chain (scalar coefficient loads) and straddling two (per-lane loads)"""
    prob, lay, host, f = ffi_ramped
    Q = _draw(lay, prob.lower, prob.upper, C, np.random.default_rng(100 + C))
    LL = f.batch(Q)
    assert LL.shape == (C, 3) and prob.out_names == ["geo_like_0", "geo_like_1", "like"]
    worst = 0.0
    for c in _check_chains(C):
        ref = _ffi_ref(host, lay, Q[c])
        worst = max(worst, float(np.max(np.abs(LL[c] - ref) / np.abs(ref))))
        np.testing.assert_allclose(LL[c], ref, rtol=1e-9, atol=1e-9)
    print("ffi ramped C=%d: worst relative difference %.3g" % (C, worst))
    # the terms matter: the same points without them are far away
    host0 = dict(host, corrections=None)
    assert abs(_ffi_ref(host0, lay, Q[0])[-1] - LL[0, -1]) > 1e-3 * abs(LL[0, -1])


def test_rvs_listed_with_the_correction_variables(ctx, ffi_ramped):
    prob, lay, host, _ = ffi_ramped
    f = prob.compile(ctx, return_rvs=True)
    want = list(SLIPS) + ["scene_0_azimuth_ramp", "scene_0_range_ramp", "scene_0_offset", "scene_1_azimuth_ramp",
                          "scene_1_range_ramp", "scene_1_offset", "h_SAR", "geo_like", "like"]
    assert f.out_names == want
    q = _draw(lay, prob.lower, prob.upper, 1, np.random.default_rng(3))[0]
    out = f(q)
    assert len(out) == len(want) and float(out[3][0]) == q[lay.offset("scene_0_azimuth_ramp")]
    np.testing.assert_allclose(float(out[-1]), _ffi_ref(host, lay, q)[-1], rtol=1e-9, atol=1e-9)
    f.release()


def test_ffi_mixed_terms(ctx):
    """one scene ramped and one not; one ramp coefficient fixed and two free; a GNSS block with two terms (ramp, then
    strain rate with masked stations) subtracted in list order; a coefficient of the strain rate fixed"""
    rng = np.random.default_rng(8)
    sc = scenes()
    gnss, strain = _gnss_block(rng)
    names = [sc[0]["name"], "gnss"]
    r0 = _ramp(names, sc[0]["name"], sc[0]["north"], sc[0]["east"])
    rg = _ramp(names, "gnss", gnss["north"], gnss["east"])
    corrs = [[r0], [], [rg, strain]]
    fixed = {r0.correction_names[1]: 0.037, strain.correction_names[3]: -55.0}
    free = [r0.correction_names[0], r0.correction_names[2]] + rg.correction_names + strain.correction_names[:3]
    prob, lay, host = _ffi_problem([sc[0], sc[1], gnss], corrs, free, fixed, seed=4)
    f = prob.compile(ctx)
    C = 70
    Q = _draw(lay, prob.lower, prob.upper, C, rng)
    LL = f.batch(Q)
    for c in range(0, C, 3):
        np.testing.assert_allclose(LL[c], _ffi_ref(host, lay, Q[c]), rtol=1e-9, atol=1e-9)
    # the uncorrected scene's column is that of the model without any correction, bit for bit
    prob0, lay0, _ = _ffi_problem([sc[0], sc[1], gnss], None, free, fixed, seed=4)
    LL0 = prob0.compile(ctx).batch(Q)
    assert np.array_equal(LL[:, 1], LL0[:, 1]) and not np.array_equal(LL[:, 0], LL0[:, 0])
    assert not np.array_equal(LL[:, 2], LL0[:, 2])
    with pytest.raises(KeyError, match=r0.correction_names[1]):
        _ffi_problem([sc[0], sc[1], gnss], corrs, free, None, seed=4)[0].compile(ctx)


def test_c_abi_rejects_bad_tables(ctx, ffi_ramped):
    prob, lay, host, f = ffi_ramped
    B = np.ones((214, 3))
    with pytest.raises(ValueError, match="already"):
        ctx.ffi_model_add_geodetic_corrections(f.model_id, [0], [3], [B], [[-1, -1, -1]], [[0.0, 0.0, 0.0]])
    prob0, _, _ = _ffi_problem(scenes(), None, [])
    for args, msg in [(([2], [3], [B], [[-1] * 3], [[0.0] * 3]), "dataset"),
                      (([1, 0], [3, 3], [np.ones((205, 3)), B], [[-1] * 3] * 2, [[0.0] * 3] * 2), "decrease"),
                      (([0], [3], [B], [[0, 1, 10 ** 6]], [[0.0] * 3]), "outside q"),
                      (([0] * 33, [1] * 33, [np.ones((214, 1))] * 33, [[-1]] * 33, [[0.0]] * 33), "table holds")]:
        f0 = prob0.compile(ctx)
        with pytest.raises(ValueError, match=msg):
            ctx.ffi_model_add_geodetic_corrections(f0.model_id, *args)
        f0.release()
    import ctypes
    from beat_amd import _lib
    f0 = prob0.compile(ctx)
    ds, nc = np.zeros(1, np.int32), np.array([5], np.int32)
    off, fix = -np.ones(4, np.int64), np.zeros(4)
    rc = ctx._lib.beatamd_ffi_model_add_geodetic_corrections(ctx._h, f0.model_id, 1, _lib.ptr(ds), _lib.ptr(nc),
                                                             _lib.ptr(np.ones(214 * 4)), _lib.ptr(off), _lib.ptr(fix))
    assert rc == _lib.EINVAL and b"columns" in ctypes.c_char_p(ctx._lib.beatamd_last_error()).value
    f0.release()
    # a model without a geodetic composite
    from beat_amd.synthetic import SyntheticSpec, build_problem
    fs = build_problem(SyntheticSpec((4,), (4,), (1.0,), T=2, N=32, D=3, S=25))[0].compile(ctx)
    with pytest.raises(ValueError, match="no geodetic composite"):
        ctx.ffi_model_add_geodetic_corrections(fs.model_id, [0], [3], [B], [[-1] * 3], [[0.0] * 3])
    fs.release()


# ------------------------------------------------------------------------------------------------- geometry composite
def _geometry_problem(rng, sizes, two_sources, ramped=(True, True), fixed_corr=None, free=None, empty=False):
    """the _problem shapes of tests/test_geometry.py with ramps on the scenes flagged in `ramped`"""
    from beat_amd.models import GeodeticGeometryProblem, ParameterLayout
    from test_geometry import _problem
    base, lay0, lower, upper = _problem(rng, sizes, two_sources=two_sources)
    names = ["scene_%d" % d for d in range(len(sizes))]
    corrs, o = [], 0
    for d, n in enumerate(sizes):
        corrs.append([_ramp(names, names[d], base.north[o:o + n] * 1e3, base.east[o:o + n] * 1e3)] if ramped[d] else [])
        o += n
    allnames = [n for cs in corrs for c in cs for n in c.correction_names]
    free = allnames if free is None else list(free)
    lay = ParameterLayout(OrderedDict(list(lay0.varsizes.items()) + [(n, 1) for n in free]))
    clo, cup = _bounds_for(free)
    lower, upper = dict(lower, **clo), dict(upper, **cup)
    fixed = dict(base.fixed, **(fixed_corr or {}))
    if not any(ramped):
        corrs = [[] for _ in sizes] if empty else None
    prob = GeodeticGeometryProblem(lay, base.sources, base.east, base.north, base.los, base.data, base.odws, sizes,
                                   base.weights, base.slog_pdets, base.hypers, fixed=fixed, lower=lower, upper=upper,
                                   corrections=corrs)
    return prob, lay, lower, upper


def _geom_ref(prob, lay, q):
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


def _own_constants_instance(prob):
    """launch_geom_los: k_geom_los<2, false> (every thread its own source constants) runs when a workgroup of 256
    (chain, point) pairs can touch more (chain, source) pairs than the LDS table of 48 holds"""
    nobs = prob.east.size
    return ((255 + nobs - 1) // nobs + 1) * len(prob.sources) > 48


@pytest.mark.parametrize("sizes,two,ramped,own", [((214, 205), False, (True, True), False),
                                                  ((60, 41), True, (True, True), False),
                                                  ((60, 41), True, (False, True), False),
                                                  ((6, 4), True, (True, True), True)])
def test_geometry_ramped_vs_one_chain_composition(ctx, sizes, two, ramped, own):
    rng = np.random.default_rng(5 + two + len(sizes) + sizes[0])
    prob, lay, lower, upper = _geometry_problem(rng, sizes, two, ramped)
    assert _own_constants_instance(prob) == own
    f = prob.compile(ctx)
    C = 70
    Q = _draw(lay, lower, upper, C, rng)
    if two:
        Q[:, lay.offset("slip", 1)] *= 1e6  # Mogi volume change [m^3]
    LL = f.batch(Q)
    assert LL.shape == (C, len(sizes) + 1)
    worst = 0.0
    for c in range(0, C, 3):
        ref = _geom_ref(prob, lay, Q[c])
        worst = max(worst, float(np.max(np.abs(LL[c] - ref) / np.abs(ref))))
        np.testing.assert_allclose(LL[c], ref, rtol=1e-9)
    print("geometry ramped %s: worst relative difference %.3g" % (sizes, worst))
    ref0 = _geom_ref(_geometry_problem(np.random.default_rng(5 + two + len(sizes) + sizes[0]), sizes, two,
                                       (False, False))[0], lay, Q[0])
    assert abs(ref0[-1] - LL[0, -1]) > 1e-6 * abs(LL[0, -1])


# ------------------------------------------------------------------------------------------------- no-op equivalence
def test_noop_terms_are_bitwise_the_uncorrected_model_ffi(ctx):
    sc = scenes()
    names = [s["name"] for s in sc]
    corrs = [[_ramp(names, s["name"], s["north"], s["east"])] for s in sc]
    zeros = dict((n, 0.0) for cs in corrs for c in cs for n in c.correction_names)
    rng = np.random.default_rng(12)
    LLs = []
    for corrections, fixed in [(None, None), ([[], []], None), (corrs, zeros)]:
        prob, lay, _ = _ffi_problem(sc, corrections, [], fixed)
        f = prob.compile(ctx)
        if not LLs:
            Q = _draw(lay, prob.lower, prob.upper, 530, rng)
        LLs.append(f.batch(Q).copy())
        f.release()
    assert np.isfinite(LLs[0]).all()
    assert np.array_equal(LLs[0], LLs[1]) and np.array_equal(LLs[0], LLs[2])


@pytest.mark.parametrize("sizes,two", [((214, 205), False), ((6, 4), True)])
def test_noop_terms_are_bitwise_the_uncorrected_model_geometry(ctx, sizes, two):
    LLs = []
    for ramped, empty in [((False, False), False), ((False, False), True), ((True, True), False)]:
        rng = np.random.default_rng(31)
        zeros = dict(("scene_%d_%s" % (d, s), 0.0) for d in range(2) for s in ("azimuth_ramp", "range_ramp", "offset"))
        prob, lay, lower, upper = _geometry_problem(rng, sizes, two, ramped, fixed_corr=zeros, free=[], empty=empty)
        assert (prob.corrections is None) == (not any(ramped) and not empty)
        f = prob.compile(ctx)
        Q = _draw(lay, lower, upper, 300, rng)
        LLs.append(f.batch(Q).copy())
        f.release()
    assert np.isfinite(LLs[0]).all()
    assert np.array_equal(LLs[0], LLs[1]) and np.array_equal(LLs[0], LLs[2])


# ------------------------------------------------------------------------------------------------- fused step
def test_fused_step_on_the_ramped_geometry_problem(ctx):
    """40 Metropolis steps through the fused step kernel sequence: every step's decisions and likelihood bookkeeping
    equal the host composition chain by chain (metropolis.py:313-385, from the state the device holds before the
    step); a proposal whose offset leaves the prior box is parked and rejected"""
    rng = np.random.default_rng(17)
    prob, lay, lower, upper = _geometry_problem(rng, (60, 41), False)
    f = prob.compile(ctx)
    lo, up = lay.bounds(lower, upper)
    C = 24
    Q = _draw(lay, lower, upper, C, rng)
    L = f.batch(Q)
    beta = 0.4
    ioff = lay.offset("scene_1_offset")
    n_acc = 0
    for step in range(40):
        delta = rng.standard_normal((C, lay.size)) * (up - lo) * 0.02
        parked = step % C
        delta[parked] = 0.0
        delta[parked, ioff] = 0.2          # the offset alone leaves [-0.05, 0.05]
        scaling = rng.uniform(0.5, 1.5, C)
        log_u = np.log(rng.random(C))
        Q0, L0 = Q.copy(), L.copy()
        acc = f.astep_batch(Q, L, delta, scaling, lo, up, log_u, beta)
        for c in range(C):
            q = Q0[c] + delta[c] * scaling[c]
            a_ref = False
            if np.all((q >= lo) & (q <= up)):
                lp = _geom_ref(prob, lay, q)
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
    import torch
    from beat_amd.sampler import SMC
    prob, lay, lower, upper = _geometry_problem(np.random.default_rng(19), (214, 205), False)
    f = prob.compile(ctx)
    lo, up = lay.bounds(lower, upper)
    dev = torch.device("cuda", 0)
    out = {}
    for use_graph in (False, True):
        step = SMC(f, lo, up, n_chains=256, tune_interval=7, device=dev, random_seed=2, use_graph=use_graph)
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


# ------------------------------------------------------------------------------------------------- sharded
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_shard(nproc, mode, out):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "BEATAMD_GF_SPLIT"):
        env.pop(k, None)
    env.update(BEATAMD_TEST_OUT=out, BEATAMD_TEST_MODE=mode, OMP_NUM_THREADS="1")
    worker = os.path.join(ROOT, "tests", "_shard_corr_gpu_worker.py")
    if nproc == 1:
        cmd = [sys.executable, worker]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("SHARD_CORR_WORKER_OK") == nproc, r.stdout[-2000:]
    return np.load(out)


def test_ramped_geodetic_composite_beside_a_target_sharded_wavemap(tmp_path):
    """the geodetic composite stays replicated on every rank of a target-sharded model and takes its correction terms
    with it: 2 ranks on one GPU give the likelihood vectors of the replicated model bit for bit, and those differ
    from the uncorrected model's in the geodetic columns only"""
    rep = _run_shard(1, "replicated", str(tmp_path / "rep.npz"))
    two = _run_shard(2, "targets", str(tmp_path / "two.npz"))
    assert rep["LL"].shape == two["LL"].shape == (300, 9) and np.isfinite(rep["LL"]).all()
    assert np.array_equal(rep["LL"], two["LL"])
    assert np.array_equal(rep["LL"][:, :5], rep["LL_plain"][:, :5]) and np.array_equal(rep["LL"][:, 7], rep["LL_plain"][:, 7])
    assert not np.array_equal(rep["LL"][:, 5], rep["LL_plain"][:, 5])
    assert not np.array_equal(rep["LL"][:, 6], rep["LL_plain"][:, 6])


# ------------------------------------------------------------------------------------------------- sampler wiring
def test_smc_recovers_a_known_ramp(ctx):
    """wiring (prior box, layout, stage transition), not accuracy: data = synthetics of a known source + a known ramp
    on each scene + noise drawn from the scenes' covariances; SMC with 256 chains; the posterior mean of every ramp
    coefficient lies within 3 posterior standard deviations of the truth"""
    import torch
    from beat_amd.models import GeodeticGeometryProblem, ParameterLayout, los_vectors
    from beat_amd.sampler import SMC, smc_sample
    rng = np.random.default_rng(23)
    g = load_golden("laquila_geodetic")
    sc = scenes()
    sizes = [s["data"].size for s in sc]
    east = np.concatenate([s["east"] for s in sc]) / 1e3
    north = np.concatenate([s["north"] for s in sc]) / 1e3
    los = np.concatenate([los_vectors(g["d%d_incidence" % d], g["d%d_heading" % d]) for d in range(2)])
    names = [s["name"] for s in sc]
    corrs = [[_ramp(names, s["name"], s["north"], s["east"])] for s in sc]
    cnames = [n for cs in corrs for c in cs for n in c.correction_names]
    lay = ParameterLayout(OrderedDict([("depth", 1), ("slip", 1)] + [(n, 1) for n in cnames] + [("h_SAR", 1)]))
    clo, cup = _bounds_for(cnames)
    lower = dict(clo, depth=2.0, slip=0.1, h_SAR=-0.5)
    upper = dict(cup, depth=8.0, slip=1.5, h_SAR=0.5)
    fixed = dict(east_shift=0.0, north_shift=0.0, strike=140.0, dip=50.0, rake=-90.0, length=12.0, width=8.0,
                 opening_fraction=0.0)
    truth = dict(zip(cnames, [0.004, -0.003, 0.02, -0.002, 0.005, -0.015]), depth=4.0, slip=0.6, h_SAR=0.0)
    odw = np.ones(sum(sizes))
    prob = GeodeticGeometryProblem(lay, ["rectangular"], east, north, los, np.zeros(sum(sizes)), odw, sizes,
                                   [s["W"] for s in sc], [s["sl"] for s in sc], [("h_SAR", 0)] * 2, fixed=fixed,
                                   lower=lower, upper=upper, corrections=corrs)
    qt = lay.map(truth)
    ue, un, uz = ok.rect_source(east, north, 0.0, 0.0, truth["depth"], 140.0, 50.0, -90.0, 12.0, 8.0, truth["slip"],
                                0.0, prob.nu)
    mu = (un * los[:, 0] + ue * los[:, 1]) + uz * los[:, 2]
    noise = np.concatenate([np.linalg.cholesky(s["C"]) @ rng.standard_normal(s["data"].size) for s in sc])
    ramp = np.concatenate([_corr_value(c[0], lambda n: truth[n]) for c in corrs])
    prob.data[:] = mu + ramp + noise
    f = prob.compile(ctx)
    lo, up = lay.bounds(lower, upper)
    np.testing.assert_allclose(f.batch(qt[None])[0], _geom_ref(prob, lay, qt), rtol=1e-9)
    step = SMC(f, lo, up, n_chains=256, tune_interval=10, device=torch.device("cuda", 0), random_seed=5)
    pop, lp, betas = smc_sample(30, step)
    assert betas[-1] == 1.0 and np.isfinite(lp).all()
    assert np.all((pop >= lo) & (pop <= up))
    for n in cnames:
        x = pop[:, lay.offset(n)]
        z = (x.mean() - truth[n]) / x.std()
        print("%s: truth %.4f posterior %.4f +- %.4f (z = %.2f)" % (n, truth[n], x.mean(), x.std(), z))
        assert abs(z) < 3.0, n
        assert x.std() < 0.5 * (up - lo)[lay.offset(n)] / np.sqrt(3)     # tighter than the prior
