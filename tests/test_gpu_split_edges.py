"""Edges of the patch split of short-trace libraries (gfstack.hip launch_gfstack_split: the view [T*R, P/R, D, S, N],
k_split_tslot, k_split_combine with its four epilogues) against an independent float64 reference.

Synthetics are compared with oracle.stack_all / problem_oracle.forward under a bound of rounding, not a fixed rtol: the same
index maps applied to |G| and |slips| give sum_i |term_i| per sample, and a sum of n products in float64 is off by at most
about n 2^-53 sum |terms| in either code -- 2 n 2^-53 sum |terms| for the difference, n = P * nvar (x 4 for multilinear: four
library rows per patch).  A missing range, a range in the wrong table slot or a dropped tail is off by a whole patch term.
Misfits are sums of squares of the residuals: checked against numpy on the reference residuals with the error those
residuals may carry.  Reference arithmetic: beat/ffi/base.py:607-709 (stack_all), beat/models/seismic.py:1283-1349,
beat/models/distributions.py:119-138."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


def _num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rule(T, P, N):
    from beat_amd import _lib
    return int(_lib.load().beatamd_gf_patch_ranges(T, P, N, _num_cu()))


def _assert_ranges(ctx, R):
    plan = ctx.gf_plan(passes=False)["plan"]
    if R > 1:
        assert "stacked in %d ranges of" % R in plan, (R, plan)
    else:
        assert "ranges" not in plan, plan


def _assert_within(gpu, ref, bound, n, what):
    tol = 2.0 * n * U * bound
    err = np.abs(gpu - ref)
    bad = err > tol
    assert not bad.any(), "%s: %d samples beyond the rounding bound, worst err %.3e at tol %.3e" % (
        what, int(bad.sum()), float(err[bad].max()), float(tol[bad][np.argmax(err[bad])]))


# ---- mode 0 through the library API: explicit start times, one table per virtual target ------------------------------
# (T, P, N, interpolation, forced R or None = the rule)
_LIB_CASES = [
    (4, 64, 1, "nearest_neighbor", None), (4, 64, 2, "multilinear", None), (3, 66, 63, "nearest_neighbor", None),
    (4, 96, 64, "multilinear", None), (2, 128, 65, "nearest_neighbor", "32"), (4, 400, 128, "multilinear", None),
    (5, 128, 129, "nearest_neighbor", "2"), (3, 64, 192, "multilinear", "32"), (4, 400, 193, "nearest_neighbor", "2"),
    (6, 96, 255, "multilinear", "32"), (4, 128, 256, "nearest_neighbor", None), (4, 128, 256, "multilinear", "2"),
    (4, 128, 257, "nearest_neighbor", None), (4, 128, 257, "multilinear", "2"), (4, 97, 120, "nearest_neighbor", None),
    (4, 66, 120, "multilinear", "4"),
]


@pytest.mark.parametrize("T,P,N,interp,force", _LIB_CASES)
def test_stack_all_batch_of_split_library_within_rounding(ctx, monkeypatch, T, P, N, interp, force):
    from beat_amd.ffi import SeismicGFLibrary, SeismicGFLibraryConfig
    from oracle import oracle as orc
    D, S = 3, 20
    rng = np.random.default_rng(T * 100003 + P * 1009 + N)
    G = rng.standard_normal((T, P, D, S, N))
    cfg = SeismicGFLibraryConfig(dimensions=(T, P, D, S, N), starttime_sampling=0.5, duration_sampling=0.5,
                                 starttime_min=0.0, duration_min=0.5)
    gf = SeismicGFLibrary(cfg)
    gf.setup(T, P, D, S, N, allocate=False)
    gf._gfmatrix = G
    gf.init_optimization(ctx)
    C = 70
    dur = rng.uniform(0.5, 1.5, (C, P))
    st = rng.uniform(0.0, 9.0, (C, T, P))
    sl = rng.uniform(-2.0, 3.0, (C, P))
    if force is not None:
        monkeypatch.setenv("BEATAMD_GF_SPLIT", force)
        want = int(force) if (P % int(force) == 0 and N <= 256) else 1
    else:
        want = _rule(T, P, N)
    out = gf.stack_all_batch(dur, st, sl, interpolation=interp)
    _assert_ranges(ctx, want)
    if N == 257:
        assert want == 1
    if P == 97 or (force == "4" and P == 66):
        assert want == 1                          # a prime count of patches / a forced count that does not divide P
    assert out.shape == (C, T, N) and np.isfinite(out).all()
    assert np.array_equal(out, gf.stack_all_batch(dur, st, sl, interpolation=interp))
    n = P * (4 if interp == "multilinear" else 1)
    G_abs = np.abs(G)
    for c in range(C):
        ref = orc.stack_all(G, dur[c], st[c], sl[c], 0.5, 0.5, 0.0, 0.5, interpolation=interp)
        bnd = orc.stack_all(G_abs, dur[c], st[c], np.abs(sl[c]), 0.5, 0.5, 0.0, 0.5, interpolation=interp)
        _assert_within(out[c], ref, bnd, n, "chain %d" % c)


# ---- the fused model: synthetics (R or nslot * R table slots), residuals, the three misfit epilogues --------------------
def _model(T, geom, N, nvar, interp, cov, shifts, seed=20250711):
    from beat_amd.synthetic import SyntheticSpec, build_problem
    names = ("uparr", "uperp", "utens")[:nvar]
    spec = SyntheticSpec(geom[0], geom[1], (1.0,), T=T, N=N, D=3, S=25, covariance=cov, slip_varnames=names,
                         station_shifts=shifts, interpolation=interp, st_dt=1.0, seed=seed)
    prob, host = build_problem(spec)
    if shifts:
        # repeated and out-of-order stations (k_split_tslot: virtual target t*R + r -> slot (station of t)*R + r)
        name, _ = host["time_shifts"]
        sidx = np.array([2, 0, 0, 1, 2, 2][:T]) % host["layout"].varsizes[name]     # (T // 2 stations)
        prob.wavemaps[0].time_shifts = (name, sidx)
        host["time_shifts"] = (name, sidx)
    return spec, prob, host


def _reference(host, q):
    """(synthetics, sum |terms|) of one chain through the oracle: the second from |G| and |slips| on the same index maps"""
    from oracle import problem_oracle
    spec, lay = host["spec"], host["layout"]
    _, ex = problem_oracle.forward(host, q)
    qa = np.array(q, dtype=np.float64)
    for v in spec.slip_varnames:
        o = lay.offset(v)
        qa[o:o + spec.P] = np.abs(qa[o:o + spec.P])
    ha = dict(host, Gs=[np.abs(G) for G in host["Gs"]])
    _, exa = problem_oracle.forward(ha, qa)
    return ex["synthetics"], exa["synthetics"]


def _logpt_check(host, q, logpt_gpu, resid_ref, resid_tol):
    """logpt of every target (distributions.py:119-138) from numpy on the reference residuals; tolerance: the residuals'
    rounding bound carried through W and the square, plus the rounding of the sums"""
    spec, lay = host["spec"], host["layout"]
    pt = lay.rmap(np.asarray(q, dtype=np.float64))
    hyp = pt["h_any_P_0_Z"]
    for t in range(spec.T):
        hp = float(hyp[host["hypers"][t][1]])
        W = host["weights"][t]
        N = resid_ref.shape[1]
        if np.ndim(W) == 0:
            y, dy = W * resid_ref[t], abs(W) * resid_tol[t]
        else:
            y, dy = W @ resid_ref[t], np.abs(W) @ resid_tol[t]
        quad = float(y @ y)
        dquad = 2.0 * float(np.abs(y) @ dy) + float(dy @ dy) + 4 * N * U * quad
        norm = float(np.int16(N)) * (2 * hp + np.log(2 * np.pi))
        e = np.exp(-2 * hp)
        ref = -0.5 * (host["slog"][t] + norm + e * quad)
        tol = 0.5 * e * dquad + 8 * U * (abs(host["slog"][t]) + abs(norm) + e * quad)
        assert abs(logpt_gpu[t] - ref) <= tol, (t, logpt_gpu[t], ref, tol)


# (T, geometry -> P, N, nvar, interpolation, covariance, station shifts, forced R or None)
_G64, _G66, _G96, _G128, _G400 = ((8,), (8,)), ((6,), (11,)), ((8,), (12,)), ((8,), (16,)), ((16,), (25,))
_MODEL_CASES = [
    (4, _G64, 1, 1, "nearest_neighbor", "scalar", False, None),
    (6, _G128, 1, 2, "multilinear", "toeplitz", True, None),
    (3, _G66, 2, 1, "multilinear", "scalar", True, "2"),
    (5, _G96, 63, 3, "nearest_neighbor", "scalar", False, None),
    (4, _G64, 64, 1, "multilinear", "toeplitz", False, None),
    (6, _G128, 65, 2, "nearest_neighbor", "toeplitz", True, "32"),
    (4, _G400, 128, 2, "multilinear", "scalar", True, None),
    (6, _G96, 129, 1, "nearest_neighbor", "toeplitz", True, None),
    (3, _G128, 192, 3, "multilinear", "scalar", False, "2"),
    (6, _G64, 193, 2, "multilinear", "toeplitz", True, "2"),
    (2, _G66, 255, 1, "nearest_neighbor", "scalar", True, None),
    (4, _G128, 256, 1, "multilinear", "toeplitz", True, None),
    (6, _G400, 120, 1, "nearest_neighbor", "toeplitz", True, "2"),
    (4, _G64, 257, 1, "nearest_neighbor", "toeplitz", False, None),
]


@pytest.mark.parametrize("T,geom,N,nvar,interp,cov,shifts,force", _MODEL_CASES)
def test_fused_model_on_split_library_within_rounding(ctx, monkeypatch, T, geom, N, nvar, interp, cov, shifts, force):
    from beat_amd.synthetic import draw_population
    spec, prob, host = _model(T, geom, N, nvar, interp, cov, shifts)
    P = spec.P
    f = prob.compile(ctx)
    if force is not None:
        monkeypatch.setenv("BEATAMD_GF_SPLIT", force)
        want = int(force) if (P % int(force) == 0 and N <= 256) else 1
    else:
        want = _rule(T, P, N)
    C = 64
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], C)
    # mode 0: synthetics
    syn = f.synthetics(Q)
    _assert_ranges(ctx, want)
    assert syn.shape == (C, T, N)
    # residuals=True (the store epilogue): data - synthetics, the same bits
    res = f.synthetics(Q, residuals=True)
    assert np.array_equal(res, host["data"][None] - syn)
    # modes 1 / 3 (scalar / bidiagonal misfit in the combine kernel), mode 2 via BEATAMD_QF_BAND=0 (dense W)
    LL = f.batch(Q)
    _assert_ranges(ctx, want)
    assert np.isfinite(LL).all()
    if cov == "toeplitz":
        band = ctx.weights_band(f.problem.wavemaps[0]._wset)
        assert band == (1 if N > 32 else -1), band          # (short traces keep the dense operator)
        monkeypatch.setenv("BEATAMD_QF_FUSE", "0")          # residual store + k_quadform_band1: the canonical order
        assert np.array_equal(LL, f.batch(Q))
        monkeypatch.delenv("BEATAMD_QF_FUSE")
        monkeypatch.setenv("BEATAMD_QF_BAND", "0")
        LD = f.batch(Q)
        monkeypatch.delenv("BEATAMD_QF_BAND")
        _assert_ranges(ctx, want)
    n = P * nvar * (4 if interp == "multilinear" else 1)
    for c in range(0, C, 9):
        ref, bnd = _reference(host, Q[c])
        _assert_within(syn[c], ref, bnd, n, "chain %d" % c)
        tol = 2.0 * n * U * bnd
        _logpt_check(host, Q[c], LL[c, :T], host["data"] - ref, tol)
        if cov == "toeplitz":
            _logpt_check(host, Q[c], LD[c, :T], host["data"] - ref, tol)
    f.release()


def test_split_out_of_grid_chain_through_station_slots(ctx):
    """a chain whose start time leaves the grid on a patch of the LAST range, through the station-slot tables: NaN like and
    an IndexError, the other chains untouched"""
    import torch
    from beat_amd.synthetic import draw_population
    spec, prob, host = _model(6, _G128, 120, 2, "multilinear", "toeplitz", True)
    f = prob.compile(ctx)
    lay = host["layout"]
    Q = draw_population(spec, lay, host["lower"], host["upper"], 64)
    A = f.batch(Q)
    _assert_ranges(ctx, _rule(6, 128, 120))
    Qb = Q.copy()
    Qb[5, lay.offset("durations") + spec.P - 1] = 99.0             # the last patch: the last range
    with pytest.raises(IndexError):
        f.batch(Qb)
    Lb = f.batch(torch.from_numpy(Qb).to(torch.device("cuda", 0))).cpu().numpy()
    with pytest.raises(IndexError):
        ctx.synchronize()
    assert np.isnan(Lb[5, -1]) and np.isfinite(np.delete(Lb[:, -1], 5)).all()
    assert np.array_equal(np.delete(Lb, 5, 0), np.delete(A, 5, 0))
    # a station correction that moves one station's traces off the grid (targets 0, 4, 5 share station 2)
    name, _ = host["time_shifts"]
    Qs = Q.copy()
    Qs[9, lay.offset(name, 2)] = -500.0
    Ls = f.batch(torch.from_numpy(Qs).to(torch.device("cuda", 0))).cpu().numpy()
    with pytest.raises(IndexError):
        ctx.synchronize()
    assert np.isnan(Ls[9, -1]) and np.isfinite(np.delete(Ls[:, -1], 9)).all()
    f.release()


# ---- a forced split on long traces is refused -----------------------------------------------------------------------
@pytest.mark.parametrize("N", [257, 300, 1030])
@pytest.mark.parametrize("kind", ["synthetics", "dense", "scalar", "toeplitz"])
def test_forced_split_of_long_traces_is_refused(ctx, monkeypatch, N, kind):
    """BEATAMD_GF_SPLIT=k > 1 on N > 256: k_split_combine holds one trace in its 256 threads, so the library is stacked as
    it is -- the same bits as BEATAMD_GF_SPLIT=0, and no ranges in the plan"""
    from beat_amd.synthetic import draw_population
    cov = "scalar" if kind in ("synthetics", "scalar") else "toeplitz"
    spec, prob, host = _model(2, _G64, N, 1, "nearest_neighbor", cov, False)
    f = prob.compile(ctx)
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], 64)

    def run():
        return f.synthetics(Q) if kind == "synthetics" else f.batch(Q)
    if kind == "dense":
        monkeypatch.setenv("BEATAMD_QF_BAND", "0")
    monkeypatch.setenv("BEATAMD_GF_SPLIT", "0")
    base = run()
    assert np.isfinite(base).all()
    for k in ("2", "4"):
        monkeypatch.setenv("BEATAMD_GF_SPLIT", k)
        out = run()
        assert "ranges" not in ctx.gf_plan(passes=False)["plan"], (k, ctx.gf_plan(passes=False))
        assert np.array_equal(out, base), (k, int((out != base).sum()))
    f.release()


# ---- bitwise invariants on a split library -------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["nearest_neighbor", "multilinear"])
def test_split_result_independent_of_batch(ctx, interp):
    """the same batch twice, and a chain's result whatever its batch (1 / 20 chains: streaming kernel, 100: the dma family,
    600: ws / runs) -- one slip variable, where every kernel sums in the same order"""
    from beat_amd.synthetic import draw_population
    spec, prob, host = _model(4, _G128, 120, 1, interp, "toeplitz", True)
    f = prob.compile(ctx)
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], 600)
    A = f.batch(Q)
    _assert_ranges(ctx, _rule(4, 128, 120))
    assert np.array_equal(A, f.batch(Q))
    for a, b in ((17, 18), (7, 27), (40, 140), (0, 600)):
        assert np.array_equal(f.batch(Q[a:b]), A[a:b]), (a, b, ctx.last_kernel())
        _assert_ranges(ctx, _rule(4, 128, 120))
    S = f.synthetics(Q)
    for a, b in ((17, 18), (7, 27), (40, 140)):
        assert np.array_equal(f.synthetics(Q[a:b]), S[a:b]), (a, b, ctx.last_kernel())
    f.release()


@pytest.mark.parametrize("split", [None, "0"])
@pytest.mark.parametrize("pair", ["1", "2"])
@pytest.mark.parametrize("nvar", [1, 2])
def test_gs_pair_with_bidiagonal_epilogue(ctx, monkeypatch, split, pair, nvar):
    """BEATAMD_GS_PAIR=1 (pair gather: never carries the fused epilogue, residual store + k_quadform_band1 behind it) and =2
    (the plain k_gfstack_ws, with the epilogue where the library is not split) with the bidiagonal misfit, behind patch
    ranges and unsplit: the canonical order of BEATAMD_QF_FUSE=0, bit for bit for one slip variable"""
    from beat_amd.synthetic import draw_population
    spec, prob, host = _model(4, _G128, 130, nvar, "nearest_neighbor", "toeplitz", True)   # (even N: chain-shared kernels)
    f = prob.compile(ctx)
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], 600)
    if split is not None:
        monkeypatch.setenv("BEATAMD_GF_SPLIT", split)
    monkeypatch.setenv("BEATAMD_GS_CG", "512")                  # (the ws family: the kernels that have the epilogue)
    monkeypatch.setenv("BEATAMD_GS_WS", "1")
    monkeypatch.setenv("BEATAMD_QF_FUSE", "0")
    ref = f.batch(Q)
    monkeypatch.delenv("BEATAMD_QF_FUSE")
    monkeypatch.setenv("BEATAMD_GS_PAIR", pair)
    A = f.batch(Q)
    assert ctx.last_kernel().startswith("k_gfstack_ws"), ctx.last_kernel()
    _assert_ranges(ctx, _rule(4, 128, 130) if split is None else 1)
    assert np.isfinite(A).all()
    if nvar == 1:
        assert np.array_equal(A, ref)
    np.testing.assert_allclose(A, ref, rtol=1e-12)
    f.release()


@pytest.mark.parametrize("interp", ["nearest_neighbor", "multilinear"])
def test_skip_parked_on_split_library_bitwise(ctx, monkeypatch, interp):
    """the split stacks every chain (active = nullptr): BEATAMD_SKIP_PARKED on and off give the same chain states,
    likelihoods and accept flags, for astep_batch and the device-drawn fused step"""
    import torch
    from beat_amd.synthetic import draw_population
    spec, prob, host = _model(4, _G128, 120, 1, interp, "toeplitz", True)
    f = prob.compile(ctx)
    lay = host["layout"]
    lo, up = lay.bounds(host["lower"], host["upper"])
    C = 512
    rng = np.random.default_rng(31)
    Q0 = draw_population(spec, lay, host["lower"], host["upper"], C, seed_offset=2100)
    L0 = f.batch(Q0)
    _assert_ranges(ctx, _rule(4, 128, 120))
    steps = []
    for _ in range(3):
        delta = rng.standard_normal((C, lay.size)) * (up - lo) * 1e-3
        out = np.ones(C, bool)
        out[rng.permutation(C)[:300]] = False
        delta[out] *= 1e5                               # certainly outside the box: parked, rejected
        steps.append((delta, np.log(rng.random(C))))
    res = []
    for skip in (True, False):
        monkeypatch.setenv("BEATAMD_SKIP_PARKED", "1" if skip else "0")
        Q, L = Q0.copy(), L0.copy()
        accs = [f.astep_batch(Q, L, d, np.ones(C), lo, up, lu, 0.5).copy() for d, lu in steps]
        _assert_ranges(ctx, _rule(4, 128, 120))
        res.append((Q, L, np.array(accs)))
    (Qa, La, aa), (Qb, Lb, ab) = res
    assert np.array_equal(aa, ab) and np.array_equal(Qa, Qb) and np.array_equal(La, Lb)
    assert aa.any() and not aa.all()
    scales = torch.from_numpy((up - lo) * 5e-4).cuda()
    lo_d, up_d = torch.from_numpy(lo).cuda(), torch.from_numpy(up).cuda()
    ones = torch.ones(C, dtype=torch.float64, device="cuda")
    res = []
    for skip in (True, False):
        monkeypatch.setenv("BEATAMD_SKIP_PARKED", "1" if skip else "0")
        Q, L = torch.from_numpy(Q0).cuda(), torch.from_numpy(L0).cuda()
        acc = torch.zeros(C, dtype=torch.int32, device="cuda")
        acc_sum = torch.zeros(C, dtype=torch.int32, device="cuda")
        n_acc = torch.zeros(1, dtype=torch.int64, device="cuda")
        accs = []
        for step in range(4):
            f.mstep_batch(Q, L, scales, 0, 0, 97, step, 0, ones, lo_d, up_d, 0.5, acc, acc_sum, n_acc)
            accs.append(acc.cpu().numpy().copy())
        _assert_ranges(ctx, _rule(4, 128, 120))
        res.append((Q.cpu().numpy(), L.cpu().numpy(), np.array(accs), acc_sum.cpu().numpy(), int(n_acc.item())))
    (Qa, La, aa, sa, na), (Qb, Lb, ab, sb, nb) = res
    assert np.array_equal(aa, ab) and np.array_equal(sa, sb) and na == nb
    assert np.array_equal(Qa, Qb) and np.array_equal(La, Lb)
    assert 0 < na < 4 * C
    f.release()
