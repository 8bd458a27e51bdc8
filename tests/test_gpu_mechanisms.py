"""Mechanism ensembles on the device (csrc/mechanisms.hip) against tests/mechanisms_ref.py and tests/golden/mechanisms.npz.

Decomposed quantities carry the bounds of test_mechanisms_host.py (4 x the worse of the host build and numpy on the
fixture); the (pixel, draw) accumulations are given their unit tensors, so both sides read the same bits, and are held to
``array_equal``."""
from collections import OrderedDict

import numpy as np
import pytest

import mechanisms_ref as ref
from beat_amd import mechanisms as M, mechanisms_binding as mb
from conftest import load_golden
from test_mechanisms_host import BOUND, MEASURED, U, frobenius, units_off

pytestmark = pytest.mark.gpu

WAVES = ("any_P", "any_SV", "any_SH")
SHAPES = (None, "wide", "narrow")
DRAWS = (1, 2, 63, 64, 65, 257, mb.CHUNK + 1)      # the last crosses a draw-chunk boundary by one


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.fixture(scope="module")
def gold():
    return load_golden("mechanisms")


def _units(n, P, seed):
    """(n, P, 6) unit tensors of random tensors, made on the host"""
    rng = np.random.default_rng(seed)
    return np.array([[ref.unit6(m) for m in row] for row in rng.normal(size=(n, P, 6))])


def _sphere(res, wave="any_P", projection="lambert"):
    rw, pix, x, y = M.focal_sphere(res, projection, wave)
    return rw, pix, ref.focal_grid(res, projection)[0]


# ------------------------------------------------------------------------------------------------ k_mt_decompose
def _check_rows(got, m6, want=None):
    """the device's rows against the restatement (or ``want``) within BOUND, and the identities of an eigen-system"""
    if want is None:
        want = {"evals": [], "moments": [], "ratios": [], "parts": [], "uv": []}
        for m in m6:
            mo, ra, pa = ref.standard_decomposition(m)
            for k, v in (("evals", np.linalg.eigvalsh(ref.symmat6(m))), ("moments", mo), ("ratios", ra), ("parts", pa),
                         ("uv", ref.hudson_of(m))):
                want[k].append(v)
    worst = {}
    for name in MEASURED:
        off = units_off(name, got[name], np.asarray(want[name]), m6)
        worst[name] = off.max()
    fro = frobenius(m6)
    for i, m in enumerate(m6):
        V, w = got["evecs"][i], got["evals"][i]
        assert np.all(np.diff(w) >= 0.0)
        np.testing.assert_allclose(V.T @ V, np.eye(3), rtol=0, atol=32 * U)
        np.testing.assert_allclose(V @ np.diag(w) @ V.T, ref.symmat6(m), rtol=0, atol=64 * U * fro[i])
        for p in range(5):
            np.testing.assert_allclose(got["unit"][i, p], ref.unit6(got["parts"][i, p]), rtol=4 * U, atol=0, equal_nan=True)
    return worst


def test_decompose_meets_the_fixture(ctx, gold):
    m6 = gold["m6"]
    got = mb.mt_decompose(ctx, m6)
    worst = _check_rows(got, m6, want=gold)
    print("device worst, units of the bound's scale:", dict((k, round(float(v), 2)) for k, v in worst.items()))
    for name in MEASURED:
        assert worst[name] <= BOUND[name], (name, worst[name])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_decompose_against_the_restatement(ctx, n):
    import torch
    from beat_amd.sources import dc_m6
    rng = np.random.default_rng(n)
    m6 = rng.normal(size=(n, 6)) * 10.0 ** rng.integers(-3, 4, size=(n, 1))
    got = mb.mt_decompose(ctx, m6)
    assert np.array_equal(got["parts"][:, 4], m6)
    worst = _check_rows(got, m6)
    for name in MEASURED:
        assert worst[name] <= BOUND[name], (name, worst[name])
    # strike, dip, rake: the device forms the double couple of the polarity likelihood, then the same arithmetic
    sdr = np.column_stack([rng.uniform(0, 360, n), rng.uniform(0, 90, n), rng.uniform(-180, 180, n)])
    dc = mb.mt_decompose(ctx, sdr)
    twin = np.array([dc_m6(*row) for row in sdr])
    np.testing.assert_allclose(dc["parts"][:, 4], twin, rtol=0, atol=8 * U)
    again = mb.mt_decompose(ctx, np.ascontiguousarray(dc["parts"][:, 4]))
    for k in again:
        assert np.array_equal(again[k], dc[k], equal_nan=True), k
    assert np.all(np.abs(dc["ratios"][:, 1] - 1.0) <= BOUND["ratios"] * U) and np.all(np.abs(dc["uv"]) <= BOUND["uv"] * U)
    # how the population is cut into calls changes no bit; device tensors give the same bits
    cuts = [0, 1, n // 2, n] if n > 2 else [0, n]
    for k in got:
        pieces = np.concatenate([mb.mt_decompose(ctx, np.ascontiguousarray(m6[a:b]), want=(k,))[k]
                                 for a, b in zip(cuts[:-1], cuts[1:]) if b > a])
        assert np.array_equal(pieces, got[k], equal_nan=True), k
    dev = mb.mt_decompose(ctx, torch.from_numpy(m6).cuda())
    for k in got:
        assert dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy(), got[k], equal_nan=True), k


def test_public_decomposition_functions(ctx):
    m6 = np.random.default_rng(11).normal(size=(65, 6))
    full = mb.mt_decompose(ctx, m6)
    e = M.eigensystems(m6)
    d = M.standard_decompositions(m6, ctx=ctx)
    assert np.array_equal(e.evals, full["evals"]) and np.array_equal(e.evecs, full["evecs"])
    assert np.array_equal(d.moments, full["moments"]) and np.array_equal(d.ratios, full["ratios"])
    assert np.array_equal(d.parts, full["parts"]) and d.names == ref.PARTS and np.array_equal(d.part("clvd"), full["parts"][:, 2])
    for mt_type, p in (("full", 4), ("deviatoric", 3), ("dc", 1)):
        assert np.array_equal(M.deco_parts(m6, mt_type), full["parts"][:, p])
    u, v = M.hudson_project(m6)
    assert np.array_equal(u, full["uv"][:, 0]) and np.array_equal(v, full["uv"][:, 1])
    np.testing.assert_allclose(d.ratios[:, 0] + d.ratios[:, 3], 1.0, rtol=0, atol=8 * U)


# ------------------------------------------------------------------------------------------------ k_fuzzy_accum, counts
@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("res", [3, 4, 65])
def test_counts_equal_the_sequential_restatement(ctx, res, P):
    rw, pix, inside = _sphere(res)
    for n in DRAWS:
        unit = _units(n, P, 1000 * res + n)
        if n >= 63:
            unit[n // 2, 0] = np.nan           # an all-zero part: 0 / 0, counts nothing
        want = ref.to_grid(ref.fuzzy_count(unit, rw), inside, n, res)
        for shape in SHAPES:
            got = mb.fuzzy_amps(ctx, unit, rw, pix, res, res, mask=True, shape=shape)
            assert got.shape == (P, res, res)
            assert np.array_equal(got, want, equal_nan=True), (res, P, n, shape)


def test_counts_at_resolution_200(ctx):
    import torch
    rw, pix, inside = _sphere(200)
    unit = _units(65, 1, 200)
    want = ref.to_grid(ref.fuzzy_count(unit, rw), inside, 65, 200)
    got = mb.fuzzy_amps(ctx, torch.from_numpy(unit).cuda(), rw, pix, 200, 200)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want, equal_nan=True)


@pytest.mark.parametrize("wave", WAVES)
@pytest.mark.parametrize("projection", M.PROJECTIONS)
def test_counts_of_the_three_waves(ctx, wave, projection):
    rw, pix, inside = _sphere(65, wave, projection)
    unit = _units(65, 1, 65)
    want = ref.to_grid(ref.fuzzy_count(unit, rw), inside, 65, 65)
    for shape in SHAPES:
        assert np.array_equal(mb.fuzzy_amps(ctx, unit, rw, pix, 65, 65, shape=shape), want, equal_nan=True)


def test_exact_zero_amplitude_and_identical_draws(ctx):
    strike_slip = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0])      # vertical strike-slip: no P amplitude straight down
    for res in (3, 65):
        inside = ref.focal_grid(res)[0].reshape(res, res)
        for n in (1, 65):
            amps, x, y = M.mts2amps(np.tile(strike_slip, (n, 1)), "lambert", "full", res)
            assert amps.shape == (res, res) and np.array_equal(np.isnan(amps), ~inside)
            assert amps[res // 2, res // 2] == 0.0                                # an exact 0 adds nothing
            values = set(np.unique(amps[inside]).tolist())                        # n identical draws: exact 0s and 1s
            assert values <= {0.0, 1.0} and (res == 3 or values == {0.0, 1.0})
            assert np.array_equal(x, np.linspace(-1, 1, res)) and np.array_equal(y, x)
    # the four quadrants: compression where x y > 0 (north-east and south-west)
    amps, x, y = M.mts2amps(strike_slip[None], "lambert", "full", 65)
    assert amps[48, 48] == 1.0 and amps[16, 16] == 1.0 and amps[16, 48] == 0.0 and amps[48, 16] == 0.0


# ------------------------------------------------------------------------------------------------ k_fuzzy_accum, sums
@pytest.mark.parametrize("n", [1, 65])
def test_sums_equal_the_sequential_loop(ctx, n):
    for res, P in ((4, 1), (65, 5)):
        rw, pix, inside = _sphere(res)
        unit = _units(n, P, 7 * res + n)
        want = ref.to_grid(ref.fuzzy_sum(unit, rw), inside, n, res)
        for shape in SHAPES:
            got = mb.fuzzy_amps(ctx, unit, rw, pix, res, res, mask=False, shape=shape)
            assert np.array_equal(got, want, equal_nan=True), (res, P, n, shape)


# ------------------------------------------------------------------------------------------------ end to end
def test_mts2amps_against_numpys_own_decomposition(ctx):
    """The two sides decompose with different roundings, so a (pixel, draw) sign may differ only where the amplitude is
    rounding noise: per pixel |amps - ref| n is at most the number of its draws with |a| <= 64 2^-53 sum |r_k u_k|, and
    that band holds at most 1e-5 of all pairs (0 of 6 418 000 for the restatement alone with 2000 draws)."""
    n, res = 500, 65
    mts = np.random.default_rng(1).normal(size=(n, 6))
    rw, pix, inside = _sphere(res)
    want, unit = ref.mts2amps(mts, "lambert", "deviatoric", res, rw)
    got, x, y = M.mts2amps(mts, "lambert", "deviatoric", res)
    a = np.array([ref.amplitudes(rw, u[0]) for u in unit])                            # (n, npix)
    size = np.array([np.abs(rw * u[0][:, None]).sum(axis=0) for u in unit])
    band = np.abs(a) <= 64 * U * size
    print("pairs in the rounding band: %d of %d" % (band.sum(), band.size))
    assert band.sum() <= 1e-5 * band.size, band.sum()
    diff = np.abs(got - want).ravel()[inside] * n
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.all(diff <= band.sum(axis=0) + 1e-9), (diff.max(), band.sum())
    # mask=False: the mean amplitude.  A deviatoric part is off by at most BOUND["parts"] 2^-53 ||M|| an entry on either
    # side, so an entry of its unit tensor (part sqrt 2 / ||part||, entries <= sqrt 2) by at most 8 times that over ||dev||,
    # and an amplitude by that times sum |r_k|; the mean over the draws adds its own roundings (16 2^-53 sum |r_k u_k|)
    m = 65
    want_s, unit_s = ref.mts2amps(mts[:m], "lambert", "deviatoric", res, rw, mask=False)
    got_s, _, _ = M.mts2amps(mts[:m], "lambert", "deviatoric", res, mask=False)
    dev = np.array([frobenius([ref.standard_decomposition(t)[2][3]])[0] for t in mts[:m]])
    per_draw = 2 * 8 * BOUND["parts"] * U * frobenius(mts[:m]) / dev
    tol = (per_draw[:, None] * np.abs(rw).sum(axis=0)[None, :]).mean(axis=0) + 16 * U * size[:m].max(axis=0)
    keep = inside.reshape(res, res)
    assert np.all(np.abs(got_s[keep] - want_s[keep]) <= tol)


def test_decomposition_amps_is_five_calls_and_numpys_percentiles(ctx):
    import torch
    n, res = 257, 65
    mts = np.random.default_rng(5).normal(size=(n, 6))
    d = M.decomposition_amps(mts, res)
    dec = M.standard_decompositions(mts)
    assert d.names == ref.PARTS and d.amps.shape == (5, res, res)
    for p in range(5):
        one, _, _ = M.mts2amps(np.ascontiguousarray(dec.parts[:, p]), "lambert", "full", res)
        assert np.array_equal(d.amps[p], one, equal_nan=True), ref.PARTS[p]
    assert np.array_equal(d.ratio_percent, np.percentile(dec.ratios * 100.0, [2.5, 97.5], axis=0).T)
    assert np.array_equal(d.ratio_spread, dec.ratios.max(axis=0) - dec.ratios.min(axis=0))
    np.testing.assert_allclose(d.ratio_mean, dec.ratios.mean(axis=0), rtol=1e-13)
    dd = M.decomposition_amps(torch.from_numpy(mts).cuda(), res)
    assert dd.amps.is_cuda and np.array_equal(dd.amps.cpu().numpy(), d.amps, equal_nan=True)
    assert np.array_equal(dd.ratio_percent.cpu().numpy(), d.ratio_percent)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_row(ctx):
    import torch
    mts = np.random.default_rng(9).normal(size=(130, 6))
    for row, value in ((3, np.nan), (129, np.inf), (64, 0.0)):
        bad = mts.copy()
        if value == 0.0:
            bad[row] = 0.0
        else:
            bad[row, 4] = value
        for arr in (bad, torch.from_numpy(bad).cuda()):
            for call in (lambda: M.mts2amps(arr, "lambert", "full", 5), lambda: M.hudson_project(arr),
                         lambda: M.decomposition_amps(arr, 5), lambda: mb.mt_decompose(ctx, arr)):
                with pytest.raises(ValueError, match=r"row %d\b" % row):
                    call()
    sdr = np.array([[10.0, 20.0, 30.0], [np.nan, 1.0, 2.0]])
    with pytest.raises(ValueError, match=r"row 1\b"):
        M.hudson_project(sdr)
    assert np.all(np.isfinite(M.hudson_project(np.zeros((2, 3)))[0]))       # strike = dip = rake = 0 is a double couple
    # two bad rows: the first is named
    bad = mts.copy()
    bad[[100, 7]] = np.nan
    with pytest.raises(ValueError, match=r"row 7\b"):
        M.eigensystems(bad)
    rw, pix, inside = _sphere(4)
    with pytest.raises(IndexError):
        mb.fuzzy_amps(ctx, _units(2, 1, 0), rw, pix + 13, 4, 4)


# ------------------------------------------------------------------------------------------------ a compiled model feeds it
def test_moment_tensors_of_a_compiled_model_feed_the_figures(ctx):
    import torch
    from beat_amd.models import ParameterLayout, PolarityMap, PolarityProblem
    c38 = 3.0 * np.pi / 8.0
    box = OrderedDict([("w", (-c38, c38)), ("v", (-1.0 / 3.0, 1.0 / 3.0)), ("kappa", (0.0, 2.0 * np.pi)),
                       ("sigma", (-np.pi / 2.0, np.pi / 2.0)), ("h", (0.0, 1.0)), ("h_any_P_pol_0", (0.02, 2.0))])
    rng = np.random.default_rng(21)
    lay = ParameterLayout(OrderedDict((k, 1) for k in box))
    maps = [PolarityMap("any_P", rng.uniform(0.0, np.pi, 12), rng.uniform(0.0, 2.0 * np.pi, 12), rng.choice([-1, 1], 12))]
    lower, upper = dict((k, v[0]) for k, v in box.items()), dict((k, v[1]) for k, v in box.items())
    prob = PolarityProblem(lay, "mtqt", maps, fixed={}, lower=lower, upper=upper)
    f = prob.compile(ctx)
    lo, up = lay.bounds(lower, upper)
    Q = lo + (up - lo) * rng.random((65, lay.size))
    Qd = torch.from_numpy(Q).cuda()
    m6d = f.moment_tensors(Qd)
    amps, x, y = M.mts2amps(m6d, "lambert", "full", 33)
    u, v = M.hudson_project(m6d)
    assert amps.is_cuda and x.is_cuda and u.is_cuda and v.is_cuda and amps.shape == (33, 33) and u.shape == (65,)
    m6 = f.moment_tensors(Q)
    amps_h, _, _ = M.mts2amps(m6, "lambert", "full", 33)
    u_h, v_h = M.hudson_project(m6)
    assert isinstance(amps_h, np.ndarray) and np.array_equal(amps.cpu().numpy(), amps_h, equal_nan=True)
    assert np.array_equal(u.cpu().numpy(), u_h) and np.array_equal(v.cpu().numpy(), v_h)
    inside = ref.focal_grid(33)[0].reshape(33, 33)
    assert np.all((amps_h[inside] >= 0.0) & (amps_h[inside] <= 1.0)) and np.all(np.abs(v_h) <= 1.0)
    f.release()
