"""The geodetic FFI library builder and the resolution-based discretization on the device (csrc/geolib.hip,
csrc/resolution.hip, beat_amd.ffi, beat_amd.discretization): the library against the half-space displacements the
engine already serves and the numpy projection; the correlated operator against the recorded reference operator; the
resolution matrix against the reference's expression in numpy; the rating against the numpy restatement; the loop
against the restated loop of the fixture problem (tests/discretization_ref.py, tests/golden/discretization_fixture.npz);
and the optimized fault's library in a geodetic FFI problem."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import discretization_ref as dref  # noqa: E402
from conftest import load_golden  # noqa: E402
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
COMPS = ("uparr", "uperp", "utens")


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.fixture(scope="module")
def fp():
    return dref.fixture_problem()


@pytest.fixture(scope="module")
def fix():
    return load_golden("discretization_fixture")


@pytest.fixture(scope="module")
def restated(fp):
    """the restated loop, computed once and left unchanged"""
    return dref.optimize(fp["cfg"], fp["subfaults"], fp["east"], fp["north"], fp["los"], fp["odw"], fp["nu"],
                         fp["varnames"])


@pytest.fixture(scope="module")
def engine(ctx, fp):
    from beat_amd.heart import HalfspaceEngine
    return HalfspaceEngine(nu=fp["nu"], ctx=ctx)


@pytest.fixture(scope="module")
def datasets(fp):
    from beat_amd.heart import GeodeticDataset
    out, o = [], 0
    for n in fp["sizes"]:
        s = slice(o, o + n)
        out.append(GeodeticDataset(fp["east"][s] * 1e3, fp["north"][s] * 1e3, fp["los"][s], odw=fp["odw"][s]))
        # metres and back give the fixture's kilometres exactly (multiples of 1/64 km)
        assert np.array_equal(out[-1].east_shifts / 1e3, fp["east"][s])
        assert np.array_equal(out[-1].north_shifts / 1e3, fp["north"][s])
        o += n
    return out


def _dev(a, ctx):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", ctx.device))


def _patches67(fp):
    """45 + 22 patches of the two subfaults"""
    return np.vstack([dref.patches(fp["subfaults"][0], 9, 5), dref.patches(fp["subfaults"][1], 11, 2)])


def _projection_and_bound(ctx, rows, fp):
    """(disp * los).sum(1) * odw from halfspace_displacements_batch and the rounding bound of that projection: three
    products, two sums, one scale, each within eps / 2 (a contracted product not at all) -> 8 eps sum|u S| odw is safe"""
    disp = ctx.halfspace_displacements_batch(np.zeros(len(rows), dtype=np.int32), rows[None], fp["east"], fp["north"],
                                             fp["nu"])[0]
    terms = disp * fp["los"][None]
    return terms.sum(axis=2) * fp["odw"], 8 * EPS * np.abs(terms).sum(axis=2) * fp["odw"]


# ------------------------------------------------------------------------------------------------- library
@pytest.mark.parametrize("npatch", [1, 67])
def test_library_equals_displacements_projected(ctx, engine, datasets, fp, npatch):
    from beat_amd import discretization as dz
    from beat_amd.ffi import geo_construct_gf_linear_patches
    base = _patches67(fp)[:npatch] if npatch > 1 else _patches67(fp)[50:51]      # (the single one: vertical)
    rows = np.vstack([dz.component_parameters(base, c) for c in COMPS])
    G = geo_construct_gf_linear_patches(engine, datasets=datasets, patches=rows)
    assert G.shape == (3 * npatch, 70) and G.dtype == np.float64
    ref, bound = _projection_and_bound(ctx, rows, fp)
    ratio = np.abs(G - ref) / bound
    print("library %d patches: worst |G - ref| / bound = %.3g" % (npatch, ratio.max()))
    assert np.all(np.abs(G - ref) <= bound)
    assert np.abs(ref).max() > 1e-4          # the rows are not trivially zero
    # the device tensor holds the same bits; the mapping is the samples per dataset
    Gd, sizes = geo_construct_gf_linear_patches(engine, datasets=datasets, patches=rows, device=True, return_mapping=True)
    assert Gd.is_cuda and sizes == fp["sizes"]
    np.testing.assert_array_equal(Gd.cpu().numpy(), G)
    # a PatchSet and sources with kernel_parameters are accepted alike
    ps = dz.PatchSet(rows[:npatch], np.zeros(npatch, dtype=np.int64))
    np.testing.assert_array_equal(geo_construct_gf_linear_patches(engine, datasets=datasets, patches=ps), G[:npatch])


def test_library_against_the_float64_oracle(ctx, engine, datasets, fp):
    """the half-space arithmetic itself is pinned elsewhere (tests/test_gpu_geometry_mp.py); here only that the rows are
    the right sources: vertical and dipping patches of all three components against oracle/okada_oracle.py"""
    from beat_amd import discretization as dz
    from beat_amd.ffi import geo_construct_gf_linear_patches
    base = _patches67(fp)[[0, 44, 45, 66]]
    rows = np.vstack([dz.component_parameters(base, c) for c in COMPS])
    G = geo_construct_gf_linear_patches(engine, datasets=datasets, patches=rows)
    ref = dref.library(rows, fp["east"], fp["north"], fp["los"], fp["odw"], fp["nu"])
    np.testing.assert_allclose(G, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())


def test_saved_library_loads_and_stacks_to_the_whole_fault(ctx, engine, datasets, fp, tmp_path):
    from beat_amd import discretization as dz
    from beat_amd.ffi import geo_construct_gf_linear, load_gf_library
    fault = dz.DiscretizedFault(fp["subfaults"])
    fault.set_patches(_patches67(fp), [45, 22])
    libs = geo_construct_gf_linear(engine, str(tmp_path), crust_ind=0, datasets=datasets, fault=fault,
                                   varnames=["uparr", "utens"])
    assert sorted(os.listdir(str(tmp_path))) == ["geodetic_uparr_static_0.traces.npy", "geodetic_uparr_static_0.yaml",
                                                 "geodetic_utens_static_0.traces.npy", "geodetic_utens_static_0.yaml"]
    for var in ("uparr", "utens"):
        gf = load_gf_library(str(tmp_path), "geodetic_%s_static_0" % var)
        assert (gf.npatches, gf.nsamples) == (67, 70) and gf.config.component == var
        np.testing.assert_array_equal(np.asarray(gf.get_all()), libs[var].get_all())
        gf.init_optimization(ctx)
        mu = gf.stack_all(np.ones(67))
        # the whole fault at unit slip, evaluated directly: every patch a source of one call, summed over the sources
        ref, bound = _projection_and_bound(ctx, dz.component_parameters(fault.patches.params, var), fp)
        total = ref.sum(axis=0)
        # 67 rows of the library summed in some order: (67 + 8) eps sum|terms|
        tol = bound.sum(axis=0) + 67 * EPS * np.abs(ref).sum(axis=0)
        assert np.all(np.abs(mu - total) <= tol), np.max(np.abs(mu - total) / tol)
    # an existing file is kept unless forced
    again = geo_construct_gf_linear(engine, str(tmp_path), datasets=datasets, fault=fault, varnames=["uparr"])
    np.testing.assert_array_equal(np.asarray(again["uparr"].get_all()), libs["uparr"].get_all())


# ------------------------------------------------------------------------------------------------- operator
@pytest.mark.parametrize("tag", ["a", "b"])
def test_correlated_operator_on_the_device(ctx, tag):
    gold = load_golden("discretization_reference")
    c = gold["coords_" + tag]
    P = c.shape[0]
    off = ~np.eye(P, dtype=bool)
    # gaussian: sqrt, the product and the division are correctly rounded on both sides -> bit for bit, diagonal included
    Lg = ctx.smoothing_correlated(c, "gaussian")
    np.testing.assert_array_equal(Lg, gold["gauss_" + tag])
    # exponential: the device exp is not numpy's to the last place: held to 2 ulp off the diagonal
    Le = ctx.smoothing_correlated(c, "exponential")
    ref = gold["expo_" + tag]
    ulp = np.abs(Le[off] - ref[off]) / np.spacing(np.abs(ref[off]))
    print("exponential operator P=%d: worst off-diagonal difference %.1f ulp, %d entries differ" % (P, ulp.max(),
                                                                                                 int((ulp > 0).sum())))
    assert ulp.max() <= 2.0
    # the diagonal is bit for bit the documented order over the device's own entries: rows ascending from zero
    a = Le.copy()
    np.fill_diagonal(a, 0.0)
    s = np.zeros(P)
    for i in range(P):
        s = s + a[i]
    np.testing.assert_array_equal(np.diag(Le), -s)
    # device in, device out
    Ld = ctx.smoothing_correlated(_dev(c, ctx), "gaussian")
    assert Ld.is_cuda
    np.testing.assert_array_equal(Ld.cpu().numpy(), Lg)
    with pytest.raises(ValueError):
        ctx.smoothing_correlated(c, "nearest_neighbor")


# ------------------------------------------------------------------------------------------------- resolution
def test_resolution_on_the_fixture_generations(ctx, fp, fix, restated):
    eps = fp["cfg"]["epsilon"]
    worst = 0.0
    for g, gen in enumerate(restated["generations"]):
        for k in range(len(fp["varnames"])):
            gfs = np.ascontiguousarray(gen["gfs"][k])            # (P, nobs) library rows
            R, diag = ctx.model_resolution(gfs, gen["L"], eps)
            ref = dref.resolution(gfs.T, gen["L"], eps)
            bound = float(fix["g%d_bound" % g][k])
            err = np.abs(R - ref).max() / np.abs(ref).max()
            worst = max(worst, err / bound)
            print("generation %d %s P=%d: |R - ref| / max|R| = %.3g, bound %.3g" % (g, fp["varnames"][k], len(gfs), err,
                                                                                   bound))
            assert err <= bound
            np.testing.assert_array_equal(diag, np.diag(R))
    print("worst ratio to the bound %.3g" % worst)


def test_resolution_random_130x67_and_device_arguments(ctx, fix):
    G, c, eps = fix["rand_G"], fix["rand_coords"], float(fix["rand_eps"])
    L = dref.smoothing_correlated(c, "gaussian")
    ref = dref.resolution(G, L, eps)
    R, diag = ctx.model_resolution(np.ascontiguousarray(G.T), L, eps)
    err = np.abs(R - ref).max() / np.abs(ref).max()
    print("random 130 x 67: |R - ref| / max|R| = %.3g, bound %.3g" % (err, float(fix["rand_bound"])))
    assert err <= float(fix["rand_bound"])
    Rd, dd = ctx.model_resolution(_dev(G.T, ctx), _dev(L, ctx), eps)
    assert Rd.is_cuda and dd.is_cuda
    np.testing.assert_array_equal(Rd.cpu().numpy(), R)
    np.testing.assert_array_equal(dd.cpu().numpy(), diag)


def test_resolution_of_a_singular_normal_matrix_raises(ctx):
    with pytest.raises(np.linalg.LinAlgError):
        ctx.model_resolution(np.zeros((5, 9)), np.zeros((5, 5)), 0.1)
    # the context works afterwards
    R, _ = ctx.model_resolution(np.eye(5), np.zeros((5, 5)), 0.1)
    np.testing.assert_allclose(R, np.eye(5), atol=1e-15)


# ------------------------------------------------------------------------------------------------- rating
def test_rating_on_the_fixture_generations(ctx, fp, restated):
    from beat_amd import discretization as dz
    data = np.stack([fp["east"], fp["north"]], axis=1)
    bottom_m = np.array([dz.bottom_depth(sf) for sf in fp["subfaults"]]) * 1e3
    n = 0
    for gen in restated["generations"]:
        if gen["rating"] is None:
            continue
        p = gen["params"]
        sf_of = np.repeat(np.arange(2), gen["subfault_npatches"])
        cen = dref.centers(p)
        rt, dmin = ctx.division_rating(p[:, 7], p[:, 6], cen, bottom_m[sf_of], fp["cfg"]["depth_penalty"], data,
                                       gen["mean_R"])
        np.testing.assert_allclose(rt, gen["rating"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(dmin, gen["dmin"], rtol=1e-14, atol=0)
        np.testing.assert_array_equal(rt.argsort(), gen["rating"].argsort())
        n += 1
    assert n >= 3


# ------------------------------------------------------------------------------------------------- the loop
def _run(engine, datasets, fp, epsilon=None):
    from beat_amd import discretization as dz
    cfg = dz.ResolutionDiscretizationConfig(**fp["cfg"])
    if epsilon is not None:
        cfg.epsilon = epsilon
    hist = []
    fault, mean_R = dz.optimize_discretization(cfg, dz.DiscretizedFault(fp["subfaults"]), datasets, fp["varnames"],
                                               engine=engine, history=hist)
    return fault, mean_R, hist


@pytest.fixture(scope="module")
def optimized(engine, datasets, fp):
    return _run(engine, datasets, fp)


def test_loop_equals_the_restated_loop(optimized, fp, fix, restated):
    fault, mean_R, hist = optimized
    assert len(hist) == int(fix["ngen"])
    for g, h in enumerate(hist):
        np.testing.assert_array_equal(h["sf_div_idxs"], fix["g%d_sf_div_idxs" % g])
        np.testing.assert_array_equal(h["fixed_idxs"], fix["g%d_fixed_idxs" % g])
        np.testing.assert_array_equal(h["subfault_npatches"], fix["g%d_subfault_npatches" % g])
    np.testing.assert_array_equal(fault.subfault_npatches, fix["subfault_npatches"])
    # the patch table is host arithmetic of the same formulas: equal to the rounding of a different association
    np.testing.assert_allclose(fault.patches.params, fix["params"], rtol=0, atol=1e-13)
    np.testing.assert_array_equal(fault.patches.params, restated["params"])
    assert fault.npatches % 16 != 0
    bound = float(fix["g%d_bound" % (int(fix["ngen"]) - 1)].max())
    R = fault.get_model_resolution()
    err = np.abs(R - fix["R_matrix"]).max() / np.abs(fix["R_matrix"]).max()
    print("final R_matrix: %.3g of max|R|, bound %.3g" % (err, bound))
    assert err <= bound
    assert np.abs(mean_R - fix["mean_R"]).max() <= bound * np.abs(fix["R_matrix"]).max()


def test_loop_is_reproducible_bit_for_bit(optimized, engine, datasets, fp):
    fault, mean_R, hist = optimized
    fault2, mean_R2, hist2 = _run(engine, datasets, fp)
    np.testing.assert_array_equal(mean_R2, mean_R)
    np.testing.assert_array_equal(fault2.get_model_resolution(), fault.get_model_resolution())
    np.testing.assert_array_equal(fault2.patches.params, fault.patches.params)
    for a, b in zip(hist, hist2):
        np.testing.assert_array_equal(a["R_diag"], b["R_diag"])
        if a["rating"] is not None:
            np.testing.assert_array_equal(a["rating"], b["rating"])


def test_optimize_damping_picks_the_fixture_optimum(engine, datasets, fp, fix, tmp_path):
    from beat_amd import discretization as dz
    cfg = dz.ResolutionDiscretizationConfig(**fp["cfg"])
    best, result = dz.optimize_damping(str(tmp_path), cfg, dz.DiscretizedFault(fp["subfaults"]), datasets,
                                       fp["varnames"], engine=engine)
    assert cfg.epsilon == fp["cfg"]["epsilon"]
    np.testing.assert_allclose(result.epsilons, fix["damp_epsilons"], rtol=1e-15)
    assert result.faults_npatches == fix["damp_npatches"].tolist()
    # |d spread| <= |dR|_F / P <= max|dR|: the resolution bound of each run's last generation (the generator's)
    assert np.all(np.abs(np.array(result.normalized_rspreads) - fix["damp_spreads"]) <= fix["damp_atol"])
    assert result.optimum["idx"] == int(fix["damp_idx"])
    assert best.npatches == result.faults_npatches[result.optimum["idx"]]
    assert os.path.exists(os.path.join(str(tmp_path), "discretization", "resolution_result_%g_%i.yaml"
                                       % (fp["cfg"]["epsilon"], 3)))


# ------------------------------------------------------------------------------------------------- end to end
def test_optimized_fault_in_a_geodetic_ffi_problem(ctx, optimized, engine, datasets, fp):
    from beat_amd.ffi import geo_construct_gf_linear
    from beat_amd.models import FFIProblem, GeodeticData, ParameterLayout
    from beat_amd.models.laplacian import get_smoothing_operator_correlated
    fault = optimized[0]
    P, sizes, slips = fault.npatches, fp["sizes"], tuple(fp["varnames"])
    gfs = geo_construct_gf_linear(engine, "", datasets=datasets, fault=fault, varnames=slips)
    L = get_smoothing_operator_correlated(fault.get_event_relative_patch_centers(), "gaussian")
    np.testing.assert_array_equal(L, fault.get_smoothing_operator(None, "gaussian"))
    logdet = orc.log_determinant(L.T * L)            # elementwise, laplacian.py:58
    rng = np.random.default_rng(7)
    Ws, sls = [], []
    for n in sizes:
        b = rng.standard_normal((n, n))
        C = b @ b.T / n + np.eye(n)
        Ws.append(orc.cov_chol_inverse(C))
        sls.append(orc.cov_log_pdet(C))
    truth = {v: rng.random(P) for v in slips}
    data = sum(orc.geo_stack(gfs[v].get_all(), truth[v]) for v in slips) / fp["odw"] + 1e-3 * rng.standard_normal(70)
    lay = ParameterLayout(OrderedDict([(v, P) for v in slips] + [("h_SAR", 1), ("h_laplacian", 1)]))
    lower = dict([(v, 0.0) for v in slips] + [("h_SAR", -1.0), ("h_laplacian", -1.0)])
    upper = dict([(v, 2.0) for v in slips] + [("h_SAR", 1.0), ("h_laplacian", 1.0)])
    geo = GeodeticData(gfs, data, fp["odw"], sizes, Ws, sls, [("h_SAR", 0)] * len(sizes))
    prob = FFIProblem(lay, [], [], [], slips, geodetic=geo, laplacian=(L, logdet), lower=lower, upper=upper)
    f = prob.compile(ctx, return_rvs=False)
    lo, up = lay.bounds(lower, upper)
    q = lo + (up - lo) * rng.random((1, lay.size))
    LL = f.batch(q)[0]
    pt = lay.rmap(q[0])
    mu = sum(orc.geo_stack(gfs[v].get_all(), pt[v]) for v in slips)
    res = (data - mu) * fp["odw"]
    out, o = [], 0
    for n, W, sl in zip(sizes, Ws, sls):
        out.append(orc.mvn_chol_logp(W, res[o:o + n], sl, pt["h_SAR"][0]))
        o += n
    out.append(sum(orc.laplacian_logp(L, pt[v], logdet, pt["h_laplacian"][0]) for v in slips))
    ref = np.array(out + [sum(out)])
    assert prob.out_names[-2:] == ["laplacian_like", "like"] and LL.shape == ref.shape
    np.testing.assert_allclose(LL, ref, rtol=1e-9, atol=1e-9)      # the tolerance of the geodetic parity tests
