"""GPU tests of the spectrum domain of a seismic wavemap (csrc/spectrum.hip): k_amp_spectrum against numpy, its exact cases
and its bit-for-bit independence of the batch; the model against the reference's numbers (tests/golden/spectrum.npz); a model
that mixes time and spectrum wavemaps; every path that evaluates the model; a short SMC run.

The bound of the kernel against numpy, per bin:   |dev - numpy| <= 8 max(1, log2 ntrans) 2^-53 |y|_2
-- the classical O(eps log n |y|_2) error of an FFT with a constant of 8; a radix-2 double FFT and numpy's rfft each sit 2.8
(ntrans 8) to 10.8 (ntrans 4096) units of 2^-53 |y|_2 from a long-double transform, the bound is 24 to 104.
Largest |diff| / bound observed on an MI355X, per ntrans: in test_1_kernel_against_numpy's docstring."""
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu

_MODELS = {}
_traces = sr.kernel_traces


def _ctx():
    import beat_amd
    return beat_amd.get_context(0)


def _case(name):
    return sr.load_case(load_golden("spectrum"), name)


def _model(name, interp="nn", weights="scalar", hps=False):
    key = (name, interp, weights, hps)
    if key not in _MODELS:
        case = _case(name)
        prob, lay = sr.build_problem(case, [sr.make_wavemap(case, interp, weights, hps)])
        _MODELS[key] = (case, prob.compile(_ctx()), lay)
    return _MODELS[key]


# ------------------------------------------------------------------------------------------------- 1 kernel against numpy
@pytest.mark.parametrize("N", sr.KERNEL_SIZES)
def test_1_kernel_against_numpy(N):
    """every (R, band) of a trace length within the bound of the module docstring; the trace lengths cover every ntrans
    from 2 to 8192.  Largest |diff| / bound this test printed on an MI355X, per ntrans: 2: 0, 4: 0.16, 8: 0.19, 16: 0.25
    (N = 9), 32: 0.21, 64: 0.18, 128: 0.20, 256: 0.18, 512: 0.21 (the largest one-wavefront shape), 1024: 0.19 (the smallest
    one-workgroup shape, odd stage count), 2048: 0.21, 4096: 0.17, 8192: 0.15 (profiles/spectrum_timing.json "bound_ratio"
    holds the lengths that tools/spectrum_timing.py was last run with)"""
    ntrans, worst, where = sr.kernel_bound_ratio(_ctx(), N)
    print("N %d ntrans %d: largest |diff| / bound %.3g at (R, band) = %s" % (N, ntrans, worst, where))
    assert worst <= 1.0, (N, where, worst)


def test_1_bad_arguments_launch_nothing():
    ctx = _ctx()
    x = np.ones((2, 8))
    for ntrans, band in ((8, (0, 6)), (8, (3, 3)), (8, (-1, 2)), (6, (0, 2)), (4, (0, 2)), (16384, (0, 2)), (1, (0, 1))):
        with pytest.raises(ValueError, match="amp_spectrum"):
            ctx.amp_spectrum_batch(x, ntrans, band)
    assert ctx.amp_spectrum_batch(np.zeros((0, 8)), 8, (0, 5)).shape == (0, 5)


# ------------------------------------------------------------------------------------------------- 2 exact cases
@pytest.mark.parametrize("N", (5, 120, 129, 512, 513, 4096, 4097))      # 512 | 513: one wavefront | one workgroup a trace
def test_2_exact_cases(N):
    ctx = _ctx()
    ntrans = sr.nextpow2(N)
    n2 = ntrans // 2
    band = (0, n2 + 1)
    rows = np.zeros((5, N))
    jl = [0, N - 1, 3 if N > 3 else 1]                      # first, last, an odd one
    amp = [2.5, -1.0e3, 3.0e-3]
    for r, (j, a) in enumerate(zip(jl, amp)):
        rows[1 + r, j] = a
    rows[4, :] = 0.75
    got = ctx.amp_spectrum_batch(rows, ntrans, band)
    assert not got[0].any()                                 # zeros give exact zeros
    bound = sr.bin_bound(rows, ntrans)
    for r, a in enumerate(amp):                             # |X_k| = |y_j| in every bin
        assert np.abs(got[1 + r] - abs(a)).max() <= bound[1 + r], (N, r)
    assert abs(got[4, 0] - N * 0.75) <= bound[4]            # DC of a constant row


@pytest.mark.parametrize("ntrans", (8, 128, 512, 1024, 2048, 8192))
def test_2_padding_is_never_read(ntrans):
    """N = ntrans and N = ntrans/2 + 1: the same bits as the same samples handed in zero padded to ntrans"""
    ctx = _ctx()
    rng = np.random.default_rng(ntrans)
    band = (0, ntrans // 2 + 1)
    for N in (ntrans, ntrans // 2 + 1):
        y = rng.standard_normal((3, N))
        padded = np.zeros((3, ntrans))
        padded[:, :N] = y
        assert np.array_equal(ctx.amp_spectrum_batch(y, ntrans, band), ctx.amp_spectrum_batch(padded, ntrans, band)), N


# ------------------------------------------------------------------------------------------------- 3 independence
@pytest.mark.parametrize("N", (5, 120, 129, 512, 513, 4096))
def test_3_rows_do_not_depend_on_the_batch(N):
    import torch
    ctx = _ctx()
    y, ntrans, full = _traces(N)
    n2 = ntrans // 2
    band = (0, n2 + 1)
    whole = ctx.amp_spectrum_batch(np.ascontiguousarray(y), ntrans, band)
    for r in (0, 3, 64, 129):
        assert np.array_equal(ctx.amp_spectrum_batch(np.ascontiguousarray(y[r:r + 1]), ntrans, band)[0], whole[r]), r
    # the residual option == data_spec - spectra of the plain option, bit for bit (T = 7 datasets, rows r mod T)
    T = 7
    data_spec = np.random.default_rng(N).random((T, n2 + 1)) * full[:T].max()
    res = ctx.amp_spectrum_batch(np.ascontiguousarray(y), ntrans, band, data_spec=data_spec)
    assert np.array_equal(res, data_spec[np.arange(y.shape[0]) % T] - whole)
    # device tensors in, tensor out, the same bits; and through heart.fft_transforms
    from beat_amd import heart
    yd = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    assert np.array_equal(ctx.amp_spectrum_batch(yd, ntrans, band).cpu().numpy(), whole)
    lo, hi = max(n2 // 4, 0), max(3 * n2 // 4, 1)
    assert np.array_equal(heart.fft_transforms(yd, (lo, hi)).cpu().numpy(), whole[:, lo:hi])
    assert np.array_equal(heart.fft_transforms(np.asarray(y), (lo, hi)), whole[:, lo:hi])


# ------------------------------------------------------------------------------------------------- 4 model against the fixture
@pytest.mark.parametrize("hps", (False, True), ids=("hp_shared", "hp_specific"))
@pytest.mark.parametrize("weights", ("scalar", "bidiag", "dense"))
@pytest.mark.parametrize("interp", ("nn", "ml"))
@pytest.mark.parametrize("name", ("t3", "t2s"))
def test_4_model_against_the_fixture(name, interp, weights, hps):
    case, f, lay = _model(name, interp, weights, hps)
    Q = case["Q"]
    T, N = case["data"].shape
    ntrans = int(case["ntrans"])
    want = case["logpt_%s_%s_hp%d" % (interp, weights, int(hps))]
    LL = f.batch(Q)
    assert LL.shape == (Q.shape[0], T + 1)
    np.testing.assert_allclose(LL[:, :T], want, rtol=1e-6)
    np.testing.assert_allclose(LL[:, T], want.sum(axis=1), rtol=1e-6)
    if weights == "bidiag" and name == "t2s":
        assert f.ctx.weights_band(f._wsets[0]) == 1          # the "exponential" operators run on their band
    spec = f.synthetics(Q, 0)
    assert spec.shape == case["spec_" + interp].shape
    for c in range(Q.shape[0]):
        bound = sr.bin_bound(case["syn_" + interp][c], ntrans)[:, None]
        assert (np.abs(spec[c] - case["spec_" + interp][c]) <= bound).all(), (name, interp, c)
    res = f.synthetics(Q, 0, residuals=True)
    assert np.array_equal(res, case["data_spec"][None] - spec)
    assert f.dataset_nsamples == [int(case["lohi"][1] - case["lohi"][0])] * T and f.ndata == T


# ------------------------------------------------------------------------------------------------- 5 mixed model
def _mixed(with_spectrum):
    from beat_amd.ffi import GeodeticGFLibrary, GeodeticGFLibraryConfig
    from beat_amd.models import GeodeticData
    from beat_amd.synthetic import smoothing_operator_nearest_neighbor
    case = _case("t3")
    rng = np.random.default_rng(77)
    nd, ns, psz = int(case["grid"][0]), int(case["grid"][1]), float(case["grid"][2])
    P, nobs = nd * ns, 12
    ggfs = {}
    for v in ("uparr", "uperp"):
        gg = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=(P, nobs), component=v))
        gg.setup(P, nobs, allocate=True)
        gg._gfmatrix[:] = rng.integers(-127, 128, (P, nobs)) / 256.0
        ggfs[v] = gg
    geo = GeodeticData(ggfs, rng.standard_normal(nobs), 0.5 + rng.random(nobs), [nobs], [1.5], [0.25], [("h_geo", 0)])
    lap = (smoothing_operator_nearest_neighbor(ns, nd, psz, psz), 0.5)
    wms = [sr.make_wavemap(case, "nn", domain="time", name="any_P_0")]
    if with_spectrum:
        wms.append(sr.make_wavemap(case, "ml", "dense", True, name="any_P_1"))
    prob, lay = sr.build_problem(case, wms, geo, lap, extra_vars=[("h_geo", 1, -1.0, 1.0), ("h_laplacian", 1, 0.2, 0.8)])
    Q = np.concatenate([case["Q"], np.array([[0.3, 0.4], [-0.2, 0.6], [0.1, 0.7]])], axis=1)
    return case, prob.compile(_ctx()), Q


def test_5_mixed_time_and_spectrum_wavemaps():
    case, f2, Q = _mixed(True)
    _, f1, _ = _mixed(False)
    T = case["data"].shape[0]
    L2, L1 = f2.batch(Q), f1.batch(Q)
    assert L2.shape[1] == L1.shape[1] + T == 2 * T + 3
    assert np.array_equal(L2[:, :T], L1[:, :T])                         # the time-domain wavemap
    assert np.array_equal(L2[:, 2 * T:2 * T + 2], L1[:, T:T + 2])       # geodetic, laplacian
    np.testing.assert_allclose(L2[:, T:2 * T], case["logpt_ml_dense_hp1"], rtol=1e-6)
    cols = L2[:, :-1]
    # like = the sum of the columns: within the rounding of a sum of n terms, n 2^-52 sum |l_k|
    assert (np.abs(L2[:, -1] - cols.sum(axis=1)) <= cols.shape[1] * 2.0 ** -52 * np.abs(cols).sum(axis=1)).all()
    assert f2.out_names == ["seis_like_any_P_0", "seis_like_any_P_1", "geo_like", "laplacian_like", "like"]


# ------------------------------------------------------------------------------------------------- 6 paths
def _paths_model():
    return _model("t2s", "nn", "bidiag", True)


def test_6_batch_rows_equal_single_calls():
    case, f, lay = _paths_model()
    LL = f.batch(case["Q"])
    T = case["data"].shape[0]
    for c in range(case["Q"].shape[0]):
        one = f(case["Q"][c])
        assert np.array_equal(one[0], LL[c, :T]) and float(one[1]) == LL[c, T]


def test_6_llks_and_variance_reductions_against_the_restatement():
    case, f, lay = _paths_model()
    Q = case["Q"]
    lo, hi = [int(v) for v in case["lohi"]]
    W = case["w_bidiag"]
    want = np.stack([sr.misfits(W, case["data_spec"] - case["spec_nn"][c]) for c in range(Q.shape[0])])
    np.testing.assert_allclose(f.update_llks(Q), want, rtol=1e-6)
    denom = sr.misfits(W, case["data_spec"])
    np.testing.assert_allclose(f.obs_quads(), denom, rtol=1e-6)
    vr = f.variance_reductions(Q)
    np.testing.assert_allclose(1.0 - vr, want / denom, rtol=1e-6)


def test_6_chain_off_the_patch_grid_is_nan_alone():
    import torch
    case, f, lay = _paths_model()
    ctx = f.ctx
    Q = np.repeat(case["Q"], 4, axis=0)
    good = f.batch(Q)
    bad = Q.copy()
    bad[[2, 7], lay.offset("nucleation_strike")] = 100.0           # the hypocentre leaves the patch grid
    Ld = f.batch(torch.from_numpy(bad).cuda()).cpu().numpy()
    assert np.isnan(Ld[[2, 7], -1]).all()
    keep = np.setdiff1d(np.arange(Q.shape[0]), [2, 7])
    assert np.array_equal(Ld[keep], good[keep])
    with pytest.raises((IndexError, ValueError)):
        ctx.synchronize()
    ctx.synchronize()       # the status word was cleared


def test_6_astep_moves_the_chains_the_host_rule_accepts():
    import torch
    case, f, lay = _paths_model()
    rng = np.random.default_rng(5)
    lo, up = case["lower"], case["upper"]
    C = 48
    Q0 = lo + (up - lo) * (0.05 + 0.9 * rng.random((C, lo.size)))
    L0 = f.batch(Q0)
    delta = 0.03 * (up - lo) * rng.standard_normal((C, lo.size))
    scaling = 0.5 + rng.random(C)
    beta = 0.01
    qprop = Q0 + delta * scaling[:, None]
    inside = ((qprop >= lo) & (qprop <= up)).all(axis=1)
    assert 3 <= inside.sum() <= C - 3
    Lprop = f.batch(np.where(inside[:, None], qprop, Q0))
    mr = beta * (Lprop[:, -1] - L0[:, -1])
    # log u on either side of the chain's ratio, well away from it: about half of the chains inside the box move
    log_u = mr + np.where(rng.random(C) < 0.5, -1.0, 1.0) * (0.5 + rng.random(C)) * np.maximum(np.abs(mr), 1.0)
    accept = inside & np.isfinite(mr) & (log_u < mr)
    assert 0 < accept.sum() < inside.sum()
    dev = torch.device("cuda", 0)
    Qd, Ld = torch.from_numpy(Q0).to(dev), torch.from_numpy(L0).to(dev)
    acc = f.astep_batch(Qd, Ld, torch.from_numpy(delta).to(dev), torch.from_numpy(scaling).to(dev), torch.from_numpy(lo).to(dev),
                        torch.from_numpy(up).to(dev), torch.from_numpy(log_u).to(dev), beta)
    assert np.array_equal(acc.cpu().numpy().astype(bool), accept)
    assert np.array_equal(Qd.cpu().numpy(), np.where(accept[:, None], qprop, Q0))
    assert np.array_equal(Ld.cpu().numpy(), np.where(accept[:, None], Lprop, L0))


def test_6_update_weights_equals_a_fresh_model():
    case = _case("t2s")
    prob, lay = sr.build_problem(case, [sr.make_wavemap(case, "ml", "dense", True)])
    f = prob.compile(_ctx())
    T, M = case["w_dense"].shape[:2]
    before = f.batch(case["Q"])
    with pytest.raises(ValueError):
        f.update_weights(0, np.zeros((T, 120, 120)), case["slog"])          # N-sized operators are refused
    new_slog = case["slog"] + 0.5
    f.update_weights(0, case["w_bidiag"], new_slog)
    got = f.batch(case["Q"])
    assert not np.array_equal(got, before)
    wm = sr.make_wavemap(case, "ml", "bidiag", True)
    wm.slog_pdet = new_slog
    fresh = sr.build_problem(case, [wm])[0].compile(_ctx())
    assert np.array_equal(got, fresh.batch(case["Q"]))
    np.testing.assert_allclose(got[:, :T], case["logpt_ml_bidiag_hp1"] - 0.25, rtol=1e-6)
    f.release()
    fresh.release()


# ------------------------------------------------------------------------------------------------- 7 sampler
def test_7_smc_sample_reproduces_itself(tmp_path):
    import torch
    from beat_amd.sampler import SMC, smc_sample
    case, f, lay = _model("t3", "nn", "scalar", False)
    lo, up = case["lower"].copy(), case["upper"].copy()
    # the fixture's misfits are 1e3 .. 1e4 (the data are one chain's synthetics): with exp(-2 h) ~ 1e-3 the likelihoods of the
    # prior draws differ by a few units and a run of three stages keeps more than one chain's weight
    o = lay.offsets["h_any_P_T"]
    lo[o:o + lay.varsizes["h_any_P_T"]], up[o:o + lay.varsizes["h_any_P_T"]] = 3.5, 4.0
    dev = torch.device("cuda", 0)

    def run(tag):
        step = SMC(f, lo, up, n_chains=64, device=dev, random_seed=21, tune_interval=3)
        pop, lp, betas = smc_sample(3, step, max_stages=3, homepath=str(tmp_path / tag), async_stage_files=False)
        return np.asarray(pop), np.asarray(lp), betas

    pa, la, ba = run("a")
    pb, lb, bb = run("b")
    assert pa.shape == (64, lo.size) and np.isfinite(la).all() and len(ba) >= 3
    assert np.array_equal(pa, pb) and np.array_equal(la, lb) and ba == bb
