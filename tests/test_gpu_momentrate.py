"""GPU tests of moment magnitudes, moment-rate functions (csrc/momentrate.hip) and the ranged density grid: against the
fixture written from the reference's own methods (tests/golden/moment_rate.npz), against the numpy restatement that
tests/test_momentrate_host.py pins to it (tests/momentrate_ref.py), and bit for bit where an order is fixed.

The tolerance of the rates is derived, not tuned: an amplitude is a difference of two cosines in [-1, 1] divided by a sum
of about 2; with a device cosine within 2 ulp (assumed) its absolute error stays below about 4 - 6 eps, so per sample
    |dev - ref|_j <= 16 eps sum_{p covering j} m_p + 4 eps n_j |ref_j|,  n_j = patches covering sample j.
Largest |diff| / bound observed on an MI355X: 0.048 against the fixture (case "two"), 0.037 against the restatement;
per case in profiles/momentrate_timing.json ("rate_bound_ratio")."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_ref as dref  # noqa: E402
import momentrate_ref as mr  # noqa: E402
from test_density_host import case_shape  # noqa: E402
from test_gpu_hypers import _dev  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = mr.load_cases(os.path.join(HERE, "golden", "moment_rate.npz"))
NAMES = sorted(CASES)
TD = np.load(os.path.join(HERE, "golden", "trace_density.npz"), allow_pickle=False)
EPS = mr.EPS


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


class _Model(object):
    """a bare device model with the fault and the layout of a fixture case (no composite: the onsets are handed in)"""

    def __init__(self, ctx, case):
        from beat_amd import _lib
        self.ctx, self.case, self.a = ctx, case, mr.case_arrays(case)
        a = self.a
        L = _lib.FfiLayout()
        L.nparams = a["Q"].shape[1]
        L.nvar = len(a["comps"])
        for i in range(4):
            L.slip_off[i] = a["offs"][a["comps"][i]] if i < L.nvar else -1
        L.durations_off = a["dur_off"]
        L.velocities_off = L.nuc_strike_off = L.nuc_dip_off = L.time_off = L.h_laplacian_off = -1
        self.mid = ctx.ffi_model_create(L, case["ndip"], case["nstrike"], np.ones(a["nsub"]))
        self.deltat = float(case["deltat"])
        self.rate_off = [a["offs"][v] for v in ("uparr", "uperp")]

    def spans(self, rows=slice(None), **kw):
        a = self.a
        return self.ctx.ffi_moment_rate_spans_batch(self.mid, a["Q"][rows], a["nsub"], a["P"], self.deltat,
                                                    start_times=a["starts"][rows], **kw)

    def rates(self, rows=slice(None), kbase=None, NT=None, **kw):
        a, case = self.a, self.case
        kbase = int(case["kbase"]) if kbase is None else kbase
        NT = case["rates"].shape[2] if NT is None else NT
        return self.ctx.ffi_moment_rates_batch(self.mid, a["Q"][rows], case["k"], a["nsub"], a["P"], self.deltat, kbase, NT,
                                               comp_off=self.rate_off, start_times=a["starts"][rows], **kw)

    def close(self):
        self.ctx.ffi_model_destroy(self.mid)


@pytest.fixture(scope="module")
def models(ctx):
    ms = dict((name, _Model(ctx, CASES[name])) for name in NAMES)
    yield ms
    for m in ms.values():
        m.close()


@pytest.fixture(scope="module")
def restated():
    """the restatement's rates, covers and counts of every case, computed once"""
    out = {}
    for name in NAMES:
        case, a = CASES[name], mr.case_arrays(CASES[name])
        offs = [a["offs"][v] for v in ("uparr", "uperp")]
        out[name] = [mr.moment_rates(a["Q"][c], offs, case["k"], a["starts"][c], a["dur_off"], a["sub_off"], a["sub_n"],
                                     float(case["deltat"]), int(case["kbase"]), case["rates"].shape[2])
                     for c in range(a["Q"].shape[0])]
    return out


# ------------------------------------------------------------------------------------------------- 1 the fixture
@pytest.mark.parametrize("name", NAMES)
def test_1_spans_and_supports_are_exact(models, restated, name):
    m, case = models[name], CASES[name]
    sp = m.spans()
    assert sp.dtype == np.int64 and np.array_equal(sp, case["spans"])
    sp_d = m.ctx.ffi_moment_rate_spans_batch(m.mid, _dev(m.a["Q"], m.ctx), m.a["nsub"], m.a["P"], m.deltat,
                                             start_times=_dev(m.a["starts"], m.ctx))
    assert sp_d.is_cuda and np.array_equal(sp_d.cpu().numpy(), case["spans"])
    assert int(sp[:, -1, 0].min()) == int(case["kbase"])
    assert int((sp[:, -1, 0] + sp[:, -1, 1]).max()) - int(case["kbase"]) == case["rates"].shape[2]
    # every sample the device writes lies within the (k0, nt) of a patch of the fixture, and within its row's span
    rates = m.rates()
    kbase, NT = int(case["kbase"]), rates.shape[2]
    j = np.arange(NT) + kbase
    for c in range(rates.shape[0]):
        support = np.zeros((m.a["nsub"] + 1, NT), dtype=bool)
        for s, (o, n) in enumerate(zip(m.a["sub_off"], m.a["sub_n"])):
            for p in range(o, o + n):
                k0, nt = case["patch_k0"][c, p], case["patch_nt"][c, p]
                support[s, k0 - kbase:k0 - kbase + nt] = True
        support[-1] = support[:-1].any(axis=0)
        assert np.array_equal(support, restated[name][c][2] > 0)
        assert not (rates[c] != 0.0)[~support].any()
        inside = (j[None, :] >= case["spans"][c, :, :1]) & (j[None, :] < case["spans"][c].sum(axis=1)[:, None])
        assert not (rates[c] != 0.0)[~inside].any()


@pytest.mark.parametrize("name", NAMES)
def test_1_rates_within_the_derived_bound(models, restated, name, capsys):
    m, case = models[name], CASES[name]
    host = m.rates()
    dev = m.ctx.ffi_moment_rates_batch(m.mid, _dev(m.a["Q"], m.ctx), _dev(case["k"], m.ctx), m.a["nsub"], m.a["P"], m.deltat,
                                       int(case["kbase"]), host.shape[2], comp_off=m.rate_off,
                                       start_times=_dev(m.a["starts"], m.ctx))
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
    worst_fix = worst_res = 0.0
    for c in range(host.shape[0]):
        ref, cover, count = restated[name][c]
        worst_fix = max(worst_fix, mr.worst_ratio(host[c] - case["rates"][c], mr.rate_bound(case["rates"][c], cover, count)))
        worst_res = max(worst_res, mr.worst_ratio(host[c] - ref, mr.rate_bound(ref, cover, count)))
    with capsys.disabled():
        print("\n%s: largest |diff| / bound: %.4f vs the fixture, %.4f vs the restatement" % (name, worst_fix, worst_res))
    for c in range(host.shape[0]):
        ref, cover, count = restated[name][c]
        assert (np.abs(host[c] - case["rates"][c]) <= mr.rate_bound(case["rates"][c], cover, count)).all()
        assert (np.abs(host[c] - ref) <= mr.rate_bound(ref, cover, count)).all()


@pytest.mark.parametrize("name", NAMES)
def test_1_rates_sum_to_the_moment(models, name):
    m, case = models[name], CASES[name]
    rates = m.rates()
    for c in range(rates.shape[0]):
        mom = mr.patch_moments(m.a["Q"][c], m.rate_off, case["k"]).sum()
        assert abs(rates[c, -1].sum() - mom) <= (m.a["P"] + rates.shape[2]) * EPS * mom


@pytest.mark.parametrize("name", NAMES)
def test_1_magnitudes(models, name, capsys):
    m, case, a = models[name], CASES[name], models[name].a
    P = a["P"]
    M0, Mw = m.ctx.ffi_magnitudes_batch(m.mid, a["Q"], case["k"], P)                # comp_off None: the layout's variables
    offs = [a["offs"][v] for v in a["comps"]]
    M0x, Mwx = m.ctx.ffi_magnitudes_batch(m.mid, _dev(a["Q"], m.ctx), _dev(case["k"], m.ctx), P, comp_off=offs)
    assert np.array_equal(M0x.cpu().numpy(), M0) and np.array_equal(Mwx.cpu().numpy(), Mw)
    r0, rw = mr.magnitudes(a["Q"], offs, case["k"])
    with capsys.disabled():
        nz = case["Mw"] != 0
        print("\n%s: Mw largest |diff| / (4 eps |Mw|) = %.3f" % (name, (np.abs(Mw - case["Mw"])[nz] / (4 * EPS * np.abs(case["Mw"][nz]))).max()))
    assert np.array_equal(M0, r0)                                                   # the patch order is the restatement's
    assert (np.abs(M0 - case["M0"]) <= P * EPS * np.abs(case["M0"])).all()
    assert (np.abs(Mw - case["Mw"]) <= 4 * EPS * np.abs(case["Mw"])).all()
    assert ((M0 == 0.0) == (case["M0"] == 0.0)).all() and (Mw[M0 == 0.0] == 0.0).all()
    if "utens" in a["comps"]:                                                       # a subset of the components
        M0s, _ = m.ctx.ffi_magnitudes_batch(m.mid, a["Q"], case["k"], P, comp_off=m.rate_off)
        assert np.array_equal(M0s, mr.magnitudes(a["Q"], m.rate_off, case["k"])[0]) and not np.array_equal(M0s, M0)


# ------------------------------------------------------------------------------------------------- 2 bit for bit
def test_2_cuts_and_permutations_give_the_same_bits(models):
    m = models["two"]
    C = m.a["Q"].shape[0]
    whole, sp = m.rates(), m.spans()
    M0, Mw = m.ctx.ffi_magnitudes_batch(m.mid, m.a["Q"], m.case["k"], m.a["P"])
    for cut in (1, 3, 7):
        for a in range(0, C, cut):
            rows = slice(a, a + cut)
            assert np.array_equal(m.rates(rows), whole[rows], equal_nan=True)
            assert np.array_equal(m.spans(rows), sp[rows])
            part = m.ctx.ffi_magnitudes_batch(m.mid, m.a["Q"][rows], m.case["k"], m.a["P"])
            assert np.array_equal(part[0], M0[rows]) and np.array_equal(part[1], Mw[rows])
    perm = np.random.default_rng(5).permutation(C)
    assert np.array_equal(m.rates(perm), whole[perm]) and np.array_equal(m.spans(perm), sp[perm])
    part = m.ctx.ffi_magnitudes_batch(m.mid, m.a["Q"][perm], m.case["k"], m.a["P"])
    assert np.array_equal(part[0], M0[perm]) and np.array_equal(part[1], Mw[perm])


@pytest.mark.parametrize("name", NAMES)
def test_2_total_row_is_the_in_order_sum_of_the_subfault_rows(models, name):
    rates = models[name].rates()
    nsub = models[name].a["nsub"]
    tot = np.zeros_like(rates[:, 0])
    for s in range(nsub):
        tot = tot + rates[:, s]
    assert np.array_equal(rates[:, nsub], tot)


def test_2_a_wider_grid_holds_the_same_rows(models):
    m = models["long"]
    kbase, NT = int(m.case["kbase"]), m.case["rates"].shape[2]
    wide = m.rates(kbase=kbase - 5, NT=NT + 70)
    assert np.array_equal(wide[:, :, 5:5 + NT], m.rates()) and not wide[:, :, :5].any() and not wide[:, :, 5 + NT:].any()
    big = m.rates(kbase=kbase - 5, NT=9000)          # above 64 KiB of LDS
    assert np.array_equal(big[:, :, 5:5 + NT], m.rates()) and not big[:, :, 5 + NT:].any()


# ------------------------------------------------------------------------------------------------- 3 errors
def test_3_a_grid_too_small_flags_the_draw_alone(models):
    m, case = models["two"], CASES["two"]
    whole, kbase = m.rates(), int(case["kbase"])
    ends = case["spans"][:, -1].sum(axis=1)
    late = int(np.argmax(ends))
    NT = int(np.sort(ends)[-2]) - kbase                       # every draw but the latest-ending ones fits
    out = np.full((whole.shape[0], whole.shape[1], NT), 7.0)
    with pytest.raises(ValueError, match="does not lie within the index grid"):
        m.rates(NT=NT, out=out)
    cut = ends - kbase > NT
    assert cut[late] and not cut.all()
    assert np.isnan(out[cut]).all()
    assert np.array_equal(out[~cut], whole[~cut][:, :, :NT])
    assert np.array_equal(m.rates(), whole)                   # the next call is clean
    early = int(np.argmin(case["spans"][:, -1, 0]))
    out = np.full(whole.shape, 7.0)
    with pytest.raises(ValueError):
        m.rates(kbase=kbase + 1, out=out)
    assert np.isnan(out[early]).all() and not np.isnan(out).all()


def test_3_flagged_and_non_finite_draws(models):
    m, case = models["single"], CASES["single"]
    C = m.a["Q"].shape[0]
    bad = np.zeros(C, dtype=np.int32)
    bad[2] = 1
    sp = np.full(case["spans"].shape, -1, dtype=np.int64)
    m.spans(chain_bad=bad, out=sp)                            # (the flag is the caller's: no status is raised for it)
    assert not sp[2].any() and np.array_equal(np.delete(sp, 2, 0), np.delete(case["spans"], 2, 0))
    whole = m.rates()
    got = m.rates(chain_bad=bad)
    assert np.isnan(got[2]).all() and np.array_equal(np.delete(got, 2, 0), np.delete(whole, 2, 0))
    starts = m.a["starts"].copy()
    starts[4, 1] = np.nan
    sp = np.full(case["spans"].shape, -1, dtype=np.int64)
    with pytest.raises(ValueError, match="not finite"):
        m.ctx.ffi_moment_rate_spans_batch(m.mid, m.a["Q"], 1, m.a["P"], m.deltat, start_times=starts, out=sp)
    assert not sp[4].any() and np.array_equal(np.delete(sp, 4, 0), np.delete(case["spans"], 4, 0))
    Q = m.a["Q"].copy()
    Q[5, m.a["dur_off"] + 3] = -0.5                           # a negative duration
    out = np.zeros_like(whole)
    with pytest.raises(ValueError):
        m.ctx.ffi_moment_rates_batch(m.mid, Q, case["k"], 1, m.a["P"], m.deltat, int(case["kbase"]), whole.shape[2],
                                     comp_off=m.rate_off, start_times=m.a["starts"], out=out)
    assert np.isnan(out[5]).all() and np.array_equal(np.delete(out, 5, 0), np.delete(whole, 5, 0))


def test_3_argument_errors(models):
    m, case = models["single"], CASES["single"]
    with pytest.raises(ValueError, match="samples per row"):
        m.rates(NT=20225)
    with pytest.raises(ValueError, match="samples per row"):
        m.rates(NT=0)
    with pytest.raises(ValueError, match="source-time function"):
        m.rates(stf=1)
    with pytest.raises(ValueError, match="deltat"):
        m.ctx.ffi_moment_rate_spans_batch(m.mid, m.a["Q"], 1, m.a["P"], 0.0, start_times=m.a["starts"])
    with pytest.raises(ValueError, match="outside q"):
        m.ctx.ffi_magnitudes_batch(m.mid, m.a["Q"], case["k"], m.a["P"], comp_off=[m.a["Q"].shape[1] - 2])
    with pytest.raises(ValueError, match="slip components"):
        m.ctx.ffi_magnitudes_batch(m.mid, m.a["Q"], case["k"], m.a["P"], comp_off=[0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="rupture variables"):             # no onsets and no sweep variables in the layout
        m.ctx.ffi_moment_rate_spans_batch(m.mid, m.a["Q"], 1, m.a["P"], m.deltat)
    with pytest.raises(ValueError):
        m.ctx.ffi_magnitudes_batch(m.mid, m.a["Q"], case["k"][:-1], m.a["P"])
    assert m.ctx.ffi_magnitudes_batch(m.mid, m.a["Q"][:0], case["k"], m.a["P"])[0].shape == (0,)


# ------------------------------------------------------------------------------------------------- 4 the ranged density
def _fixture_density_inputs(case):
    nsub = len(case["ndip"])
    ranges = case["spans"][:, nsub:nsub + 1].copy()
    ranges[:, :, 0] -= int(case["kbase"])
    Y = np.ascontiguousarray(case["rates"][:, nsub:nsub + 1])
    return Y, np.array([int(case["kbase"]) * float(case["deltat"])]), case["density_extent"][None, :], ranges


def test_4_fixture_grid_bit_for_bit(ctx):
    from beat_amd.summary import truncate_density
    case = CASES["two"]
    ny, nx, lw = (int(v) for v in case["density_shape"])
    Y, tmin, extent, ranges = _fixture_density_inputs(case)
    deltat = float(case["deltat"])
    host = ctx.trace_density_update_ranges(Y, tmin, deltat, extent, ranges, (ny, nx), lw)
    dev = ctx.trace_density_update_ranges(_dev(Y, ctx), _dev(tmin, ctx), deltat, _dev(extent, ctx), _dev(ranges, ctx), (ny, nx), lw).cpu().numpy()
    assert np.array_equal(host[0], case["density_raw"]) and np.array_equal(dev, host)
    assert np.array_equal(truncate_density(host[0], Y.shape[0]), case["density"])
    # zero padding would have drawn along rate 0: the plain call differs
    assert not np.array_equal(ctx.trace_density_update(Y, tmin, deltat, extent, (ny, nx), lw)[0], case["density_raw"])
    # cutting the ensemble, and the strip width
    grid = None
    for a, b in ((0, 1), (1, 8), (8, Y.shape[0])):
        grid = ctx.trace_density_update_ranges(Y[a:b], tmin, deltat, extent, ranges[a:b], (ny, nx), lw, grid)
    assert np.array_equal(grid[0], case["density_raw"])


def test_4_strip_width_does_not_matter(ctx, monkeypatch):
    case = CASES["two"]
    ny, nx, lw = (int(v) for v in case["density_shape"])
    Y, tmin, extent, ranges = _fixture_density_inputs(case)
    for strip in ("1", "7", "31"):
        monkeypatch.setenv("BEATAMD_TD_STRIP", strip)
        got = ctx.trace_density_update_ranges(Y, tmin, float(case["deltat"]), extent, ranges, (ny, nx), lw)
        assert np.array_equal(got[0], case["density_raw"]), "strip %s" % strip


@pytest.mark.parametrize("key", ["16_12_10_7_unit", "65_40_24_3_narrow", "130_33_47_7_small", "300_20_16_7_unit",
                                 "256_64_8_3_transposed"])
def test_4_no_ranges_and_full_ranges_are_the_plain_call(ctx, key):
    from beat_amd._lib import check, ptr
    N, ny, nx, lw = case_shape(key)
    Y, tmin, deltat, extent = TD[key + "_Y"], TD[key + "_tmin"], float(TD[key + "_deltat"]), TD[key + "_extent"]
    E, T = Y.shape[:2]
    plain = ctx.trace_density_update(Y, tmin, deltat, extent, (ny, nx), lw)
    assert np.array_equal(plain, TD[key + "_grid"])
    full = np.zeros((E, T, 2), dtype=np.int64)
    full[:, :, 1] = N
    assert np.array_equal(ctx.trace_density_update_ranges(Y, tmin, deltat, extent, full, (ny, nx), lw), plain)
    wider = full.copy()
    wider[:, :, 0], wider[:, :, 1] = -3, N + 9                       # a range is cut to [0, N)
    assert np.array_equal(ctx.trace_density_update_ranges(Y, tmin, deltat, extent, wider, (ny, nx), lw), plain)
    grid = np.zeros((T, ny, nx))                                     # ranges == NULL through the new entry
    check(ctx._lib.beatamd_trace_density_update_ranges(ctx._h, E, T, N, ptr(Y), ptr(tmin), deltat, ptr(extent), None, ny, nx,
                                                       float(lw), ptr(grid)))
    assert np.array_equal(grid, plain)


def test_4_ranges_against_the_restatement_of_the_plain_grid(ctx):
    """every trace drawn over its own stretch alone = the plain restatement on the slices, added in ensemble order; counts
    of 0, 1 (nothing drawn) and 2; several strips and chunks"""
    rng = np.random.default_rng(11)
    E, T, N, deltat = 9, 2, 300, 0.5
    Y = rng.uniform(0.0, 1.0, (E, T, N)) * np.sin(np.arange(N) / 17.0) ** 2
    tmin = np.array([-4.0, 2.5])
    first = rng.integers(0, 120, (E, T))
    count = rng.integers(30, 180, (E, T))
    count[0, 0], count[1, 0], count[2, 1], count[3, 1] = 0, 1, 2, N      # (first + N reaches beyond the row: cut)
    first[4, 0], count[4, 0] = 50, 100
    ranges = np.stack([first, count], axis=2).astype(np.int64)
    extent = np.array([[tmin[t], tmin[t] + (N - 1) * deltat, 0.0, 1.0] for t in range(T)])
    ref = np.zeros((T, 64, 80))
    for e in range(E):
        for t in range(T):
            f, n = int(first[e, t]), int(min(count[e, t], N - first[e, t]))
            if count[e, t] >= 2 and n >= 2:
                ref[t:t + 1] = dref.trace_density(Y[e:e + 1, t:t + 1, f:f + n], tmin[t:t + 1] + f * deltat, deltat,
                                                  extent[t:t + 1], (64, 80), 5, grid=ref[t:t + 1])
    got = ctx.trace_density_update_ranges(Y, tmin, deltat, extent, ranges, (64, 80), 5)
    assert ref.any() and np.array_equal(got, ref)
    # a sample above the extent outside every range is not looked at; inside a range it is the reference's TypeError
    Y2 = Y.copy()
    Y2[4, 0, 49] = Y2[4, 0, 150] = 5.0
    assert np.array_equal(ctx.trace_density_update_ranges(Y2, tmin, deltat, extent, ranges, (64, 80), 5), ref)
    Y2[4, 0, 51] = 5.0
    with pytest.raises(TypeError):
        ctx.trace_density_update_ranges(Y2, tmin, deltat, extent, ranges, (64, 80), 5)
    assert np.array_equal(ctx.trace_density_update_ranges(Y, tmin, deltat, extent, ranges, (64, 80), 5), ref)


# ------------------------------------------------------------------------------------------------- 5 end to end
def _end_to_end_specs():
    from beat_amd.synthetic import SyntheticSpec
    return {"one": SyntheticSpec((6,), (5,), (1.0,), T=4, N=128, D=3, S=25),
            "two": SyntheticSpec((4, 3), (5, 3), (1.0, 1.0), T=2, N=64, D=3, S=25, slip_varnames=("uparr", "uperp"),
                                 time_bounds=(-2.0, 3.0))}


@pytest.mark.parametrize("which", ["one", "two"])
def test_5_end_to_end(ctx, which):
    from beat_amd import summary
    from beat_amd.synthetic import build_problem, draw_population
    spec = _end_to_end_specs()[which]
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    try:
        lay, P, nsub, deltat = host["layout"], spec.P, spec.nsub, 0.25
        n, E = 37, 6
        pop = draw_population(spec, lay, host["lower"], host["upper"], n)
        k = np.random.default_rng(7).uniform(1.0e16, 4.0e17, P)
        offs = [lay.offset(v, 0) for v in spec.slip_varnames]
        dur_off = lay.offset("durations", 0)
        sub_n = [d * s for d, s in zip(spec.n_patch_dip, spec.n_patch_strike)]
        sub_off = [int(v) for v in np.cumsum([0] + sub_n[:-1])]
        starts = f.start_times(pop)
        res = f.moment_rates(pop, k, deltat, individual=True)
        assert set(res) == {"rates", "kbase", "times", "spans"} and isinstance(res["rates"], np.ndarray)
        kbase, NT = res["kbase"], res["rates"].shape[2]
        assert res["rates"].shape == (n, nsub + 1, NT) and res["spans"].shape == (n, nsub + 1, 2)
        assert np.array_equal(res["times"], (kbase + np.arange(NT)) * deltat)
        assert kbase == res["spans"][:, -1, 0].min() and kbase + NT == res["spans"][:, -1].sum(axis=1).max()
        for c in range(n):
            assert np.array_equal(res["spans"][c], mr.spans(starts[c], pop[c, dur_off:dur_off + P], sub_off, sub_n, deltat))
            ref, cover, count = mr.moment_rates(pop[c], offs, k, starts[c], dur_off, sub_off, sub_n, deltat, kbase, NT)
            assert (np.abs(res["rates"][c] - ref) <= mr.rate_bound(ref, cover, count)).all()
        tot = f.moment_rates(_dev(pop, ctx), _dev(k, ctx), deltat)
        assert tot["rates"].is_cuda and np.array_equal(tot["rates"].cpu().numpy(), res["rates"][:, nsub])
        assert np.array_equal(tot["times"].cpu().numpy(), res["times"])
        M0, Mw = f.magnitudes(pop, k)
        r0, rw = mr.magnitudes(pop, offs, k)
        assert np.array_equal(M0, r0) and (np.abs(Mw - rw) <= 4 * EPS * np.abs(rw)).all()

        dp = summary.derived_parameters(f, pop, k, batch=16)
        assert isinstance(dp, np.ndarray) and dp.shape == (n, 1) and np.array_equal(dp[:, 0], Mw)
        dpd = summary.derived_parameters(f, _dev(pop, ctx), k)
        assert dpd.is_cuda and np.array_equal(dpd.cpu().numpy(), dp)

        best = pop[11]
        for individual in (False, True):
            R = nsub + 1 if individual else 1
            rows = slice(0, nsub + 1) if individual else slice(nsub, nsub + 1)
            ens = summary.moment_rate_ensemble(f, pop, best, E, k, deltat, individual=individual, density=(50, 70),
                                               linewidth=7, batch=4)
            idx = summary.ensemble_indices(n, E)
            assert np.array_equal(ens["indices"], idx)
            sel = f.moment_rates(pop[idx], k, deltat, individual=True)
            kb, nt = sel["kbase"], sel["rates"].shape[2]
            assert ens["kbase"] == kb and np.array_equal(ens["times"], sel["times"])
            assert np.array_equal(ens["spans"], sel["spans"][:, rows])
            Y = np.ascontiguousarray(sel["rates"][:, rows])
            state, seen = ctx.ensemble_moments_update(Y.reshape(len(idx), R * nt))
            for key, v in zip(("mean", "std", "min", "max"), ctx.ensemble_moments_finish(state, seen)):
                assert ens[key].shape == (R, nt) and np.array_equal(ens[key], v.reshape(R, nt))
            extent = np.array([summary.moment_rate_extent(Y[:, r], ens["spans"][:, r], kb, deltat) for r in range(R)])
            assert ens["extent"].shape == (R, 4) and np.array_equal(ens["extent"], extent)
            ranges = ens["spans"].copy()
            ranges[:, :, 0] -= kb
            grid = ctx.trace_density_update_ranges(Y, np.full(R, kb * deltat), deltat, extent, ranges, (50, 70), 7)
            assert grid.any() and ens["density"].shape == (R, 50, 70)
            assert np.array_equal(ens["density"], summary.truncate_density(grid.copy(), len(idx)))
            b = f.moment_rates(best[None], k, deltat, individual=True)
            assert np.array_equal(ens["best"]["rates"], b["rates"][0, rows]) and ens["best"]["kbase"] == b["kbase"]
            assert np.array_equal(ens["best"]["times"], b["times"])

        # a hypocentre outside the patch grid: count 0, NaN rows, the status raised
        bad = pop[:5].copy()
        bad[3, lay.offset("nucleation_strike", 0)] = 1.0e3
        flags = np.zeros(5, dtype=np.int32)
        with pytest.raises(ValueError, match="nucleation index"):
            f.start_times(bad, chain_bad=flags)
        assert flags.tolist() == [0, 0, 0, 1, 0]
        sp = np.full((5, nsub + 1, 2), -1, dtype=np.int64)
        with pytest.raises(ValueError, match="nucleation index"):
            ctx.ffi_moment_rate_spans_batch(f.model_id, bad, nsub, P, deltat, out=sp)
        assert not sp[3].any() and np.array_equal(np.delete(sp, 3, 0), np.delete(res["spans"][:5], 3, 0))
        out = np.zeros((5, nsub + 1, NT))
        with pytest.raises(ValueError, match="nucleation index"):
            ctx.ffi_moment_rates_batch(f.model_id, bad, k, nsub, P, deltat, kbase, NT, comp_off=offs, out=out)
        assert np.isnan(out[3]).all() and np.array_equal(np.delete(out, 3, 0), np.delete(res["rates"][:5], 3, 0))
        with pytest.raises(ValueError):
            f.moment_rates(bad, k, deltat)
        assert np.array_equal(f.moment_rates(pop[:5], k, deltat, individual=True)["spans"], res["spans"][:5])
    finally:
        f.release()
