"""The seismic library producer on the GPU (beat_amd/seislib.py, csrc/seislib.hip) against its numpy restatement
(tests/seislib_ref.py, which tests/test_seislib_host.py pins to scipy): bit for bit.

The one place where the device and numpy cannot agree bit for bit is the cosine inside the source-time function's
amplitudes (a few ulp, as for the moment-rate kernel).  So the amplitude table of ``k_stf_table`` is compared with numpy's
within a bound derived from the cosines' error (``seislib_ref.stf_bound``), and the reference loop of the bit-for-bit
tests convolves with the table the device made; ``test_library_without_a_cosine`` has no cosine in it (every duration
below deltat / 2) and takes everything from numpy."""
import numpy as np
import pytest

import seislib_ref as ref
from beat_amd import seislib as sl, seislib_binding as sb
from beat_amd.ffi import SeismicGFLibrary, SeismicGFLibraryConfig, load_gf_library

pytestmark = pytest.mark.gpu

DELTAT = 0.25
TAPER = sl.ArrivalTaper(-1.5, -1.0, 3.0, 3.5)           # 16 samples in [b, c], 20 in [a, d]
TAPER4 = (TAPER.a, TAPER.b, TAPER.c, TAPER.d)
DURATIONS = np.array([0.1, 0.8])                         # below deltat / 2: nt == 1; rint(3.2) + 1: nt == 4
STARTTIMES = np.array([-0.5, 0.0, 0.5])
FILTERS = {
    "none": None,
    "stepwise": sl.Filter(0.1, 0.8, order=4, stepwise=True),
    "bandpass": sl.Filter(0.1, 0.8, order=3, stepwise=False),
    "bandpass+bandstop": [sl.Filter(0.1, 0.8, order=2, stepwise=False), sl.BandstopFilter(0.3, 0.5, order=2)],
}


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _case(T, P, L, seed=0):
    """responses, tmins, arrival_times: the first six (target, patch) pairs hold the window edge cases"""
    rng = np.random.default_rng(100 * P + L + seed)
    responses = rng.standard_normal((T, P, L))
    arrivals = 6.0 + 0.5 * np.arange(T)
    tmins = 3.0 + rng.integers(-4, 5, (T, P)) * DELTAT
    # inside, before sample 0, past Lc (the window of starttime 0 begins at sample L - 9), off the grid, outside, off
    tmins.flat[:6] = [3.0, 5.5, 5.0 - (L - 9) * DELTAT, 3.1, -20.0, 3.0 - 0.07]
    return responses, tmins, arrivals


def _stages(name):
    return sl.filter_stages(FILTERS[name], DELTAT)


def _host_twin(gfs):
    c = gfs.config
    twin = SeismicGFLibrary(SeismicGFLibraryConfig(
        dimensions=c.dimensions, starttime_sampling=c.starttime_sampling, duration_sampling=c.duration_sampling,
        starttime_min=c.starttime_min, duration_min=c.duration_min, component=c.component, mapnumber=c.mapnumber,
        wavename=c.wavename))
    twin.setup(*c.dimensions, allocate=True)
    return twin


def _reference(gfs, ctx, responses, tmins, arrivals, durations, starttimes, stages, table=None):
    """the host-filled twin of ``gfs``: _process_patch_seismic's loop through ``put``; table None: the device's amplitudes"""
    nt, A = table if table is not None else (_np(a) for a in sb.stf_table(ctx, durations, DELTAT))
    return ref.build_library(_host_twin(gfs), responses, tmins, DELTAT, arrivals, durations, starttimes, TAPER4, stages, nt, A)


# ------------------------------------------------------------------------------------------------ source-time function
@pytest.mark.parametrize("side", ["numpy", "torch"])
def test_stf_table_is_the_moment_rate_rule(ctx, side):
    durations = np.array([0.0, 0.1, 0.8, 3.3, 20.0, 16.1])      # nt = 1, 1, 4, 14, 81, 65: beyond one wavefront of samples
    like = None
    if side == "torch":
        import torch
        like = torch.zeros(1, dtype=torch.float64, device="cuda:%d" % ctx.device)
    nt, A = (_np(a) for a in sb.stf_table(ctx, durations, DELTAT, like=like))
    rnt, rA = ref.stf_table(durations, DELTAT)
    print("nt", nt.tolist(), "worst |dA| / bound", float((np.abs(A - rA) / ref.stf_bound(rA, rnt)).max()))
    assert nt.dtype == np.int32 and nt.tolist() == rnt.tolist() == [1, 1, 4, 14, 81, 65]
    assert A.shape == rA.shape == (6, 81)
    assert (np.abs(A - rA) <= ref.stf_bound(rA, rnt)).all()
    np.testing.assert_array_equal(A[:2], rA[:2])                # nt == 1: [1, 0, ...] exactly
    for d in range(6):
        assert (A[d, nt[d]:] == 0.0).all() and (A[d, :nt[d]] > 0.0).all()
    nt2, A2 = (_np(a) for a in sb.stf_table(ctx, durations[:3], DELTAT, ntmax=9))      # a wider table: the same rows
    np.testing.assert_array_equal(A2[:, :4], A[:3, :4])
    assert (A2[:, 4:] == 0.0).all() and nt2.tolist() == [1, 1, 4]
    with pytest.raises(ValueError, match="holds 3 samples"):
        sb.stf_table(ctx, durations[:3], DELTAT, ntmax=3)


# ------------------------------------------------------------------------------------------------ filter alone
@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("R,L", [(1, 37), (64, 64), (65, 65)])
def test_trace_filter_batch_is_the_restatement(ctx, filt, R, L):
    traces = np.random.default_rng(R + L).standard_normal((R, L))
    nt, A = sb.stf_table(ctx, DURATIONS, DELTAT)
    stages = _stages(filt)
    Y = sb.trace_filter_batch(ctx, traces, nt, A, stages)
    want = ref.filtered_traces(traces, nt, A, stages)
    assert Y.shape == (R, 2, L + 3)
    for d in range(2):
        np.testing.assert_array_equal(Y[:, d, :L + nt[d] - 1], want[d])
        assert (Y[:, d, L + nt[d] - 1:] == 0.0).all()
    assert np.isfinite(Y).all()


# ------------------------------------------------------------------------------------------------ the library
@pytest.mark.parametrize("filt", list(FILTERS))
@pytest.mark.parametrize("T,P,L", [(2, 3, 37), (2, 65, 37), (2, 3, 64), (2, 3, 65)])
def test_library_is_the_reference_loop(ctx, filt, T, P, L):
    responses, tmins, arrivals = _case(T, P, L)
    gfs = sl.construct_seismic_library(responses, tmins, DELTAT, arrivals, DURATIONS, STARTTIMES, TAPER, FILTERS[filt], ctx=ctx)
    N = TAPER.nsamples(1.0 / DELTAT)
    assert gfs.dimensions == (T, P, 2, 3, N) and N == 16
    assert (gfs.duration_min, gfs.starttime_min, gfs.starttime_sampling) == (0.1, -0.5, 0.5)
    assert abs(gfs.duration_sampling - 0.7) < 1e-15
    np.testing.assert_array_equal(gfs._tmins, arrivals)
    got = gfs._device_tensor.cpu().numpy()
    twin = _reference(gfs, ctx, responses, tmins, arrivals, DURATIONS, STARTTIMES, _stages(filt))
    np.testing.assert_array_equal(got, twin._gfmatrix)
    np.testing.assert_array_equal(twin._tmins, arrivals)
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    # the edge cases are in the inputs: assert that they occur
    i0, w0 = ref.window_tables(tmins, arrivals, STARTTIMES, DELTAT, TAPER4)
    Lc = L + 3
    assert ((i0 < 0) & (i0 + N > 0)).any(), "no window starts before sample 0"
    assert ((i0 < Lc) & (i0 + N > Lc)).any(), "no window runs past Lc"
    outside = i0 >= Lc
    assert outside.any(), "no window wholly outside"
    assert (got.transpose(0, 1, 3, 2, 4)[outside] == 0.0).all()
    raw = ((arrivals[:, None, None] - STARTTIMES[None, None, :]) + TAPER.b - tmins[:, :, None]) / DELTAT
    assert (np.floor(raw) != raw).any(), "no floor snapping"
    assert ((w0 > 0.0) & (w0 < 1.0)).any(), "no window starts inside the fade"
    assert (w0 == 1.0).any()


def test_library_without_a_cosine(ctx):
    """every duration below deltat / 2: the source-time function is [1], and the whole reference is numpy's"""
    responses, tmins, arrivals = _case(2, 3, 37, seed=7)
    durations = np.array([0.0, 0.1])
    gfs = sl.construct_seismic_library(responses, tmins, DELTAT, arrivals, durations, STARTTIMES, TAPER, FILTERS["stepwise"],
                                       ctx=ctx)
    table = ref.stf_table(durations, DELTAT)
    assert table[0].tolist() == [1, 1]
    twin = _reference(gfs, ctx, responses, tmins, arrivals, durations, STARTTIMES, _stages("stepwise"), table=table)
    np.testing.assert_array_equal(gfs._device_tensor.cpu().numpy(), twin._gfmatrix)


def test_seventeen_taps(ctx):
    """an order-8 bandpass: 17 taps, the cascade's limit"""
    filt = sl.Filter(0.1, 0.8, order=8, stepwise=False)
    stages = sl.filter_stages(filt, DELTAT)
    assert stages[0][0].size == 17
    responses, tmins, arrivals = _case(2, 3, 37, seed=3)
    gfs = sl.construct_seismic_library(responses, tmins, DELTAT, arrivals, DURATIONS, STARTTIMES, TAPER, filt, ctx=ctx)
    twin = _reference(gfs, ctx, responses, tmins, arrivals, DURATIONS, STARTTIMES, stages)
    got = gfs._device_tensor.cpu().numpy()
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got, twin._gfmatrix)


def test_library_does_not_depend_on_the_blocking(ctx):
    responses, tmins, arrivals = _case(2, 5, 37, seed=1)
    libs = [sl.construct_seismic_library(responses, tmins, DELTAT, arrivals, DURATIONS, STARTTIMES, TAPER, FILTERS["stepwise"],
                                         patch_block=pb, ctx=ctx)._device_tensor.cpu().numpy() for pb in (None, 1, 2)]
    np.testing.assert_array_equal(libs[0], libs[1])
    np.testing.assert_array_equal(libs[0], libs[2])
    import torch
    dev = sl.construct_seismic_library(torch.from_numpy(responses).to("cuda:%d" % ctx.device), tmins, DELTAT, arrivals,
                                       DURATIONS, STARTTIMES, TAPER, FILTERS["stepwise"], patch_block=3, ctx=ctx)
    np.testing.assert_array_equal(libs[0], dev._device_tensor.cpu().numpy())       # device input, a block with a tail
    odd = sl.ArrivalTaper(-1.5, -1.0, 2.75, 3.5)                                    # 15 samples: the 8-byte store path
    a = sl.construct_seismic_library(responses, tmins, DELTAT, arrivals, DURATIONS, STARTTIMES, odd, None, ctx=ctx)
    assert a.nsamples == 15
    np.testing.assert_array_equal(a._device_tensor.cpu().numpy(),
                                  sl.construct_seismic_library(responses, tmins, DELTAT, arrivals, DURATIONS, STARTTIMES, TAPER,
                                                               None, ctx=ctx)._device_tensor.cpu().numpy()[..., :15])


# ------------------------------------------------------------------------------------------------ observed traces
@pytest.mark.parametrize("side", ["numpy", "torch"])
@pytest.mark.parametrize("R", [1, 64, 65])
def test_taper_filter_traces_is_the_restatement(ctx, R, side):
    rng = np.random.default_rng(R)
    traces = rng.standard_normal((R, 41))
    tmins = 3.0 + rng.integers(-6, 7, R) * DELTAT
    tmins[0] += 0.1
    arrivals = 6.0 + rng.integers(0, 3, R) * DELTAT
    X = traces
    if side == "torch":
        import torch
        X = torch.from_numpy(traces).to("cuda:%d" % ctx.device)
    for filt in ("none", "stepwise"):
        got = sl.taper_filter_traces(X, tmins, DELTAT, TAPER, FILTERS[filt], arrivals, ctx=ctx)
        assert (side == "numpy") == isinstance(got, np.ndarray) and tuple(got.shape) == (R, 16)
        np.testing.assert_array_equal(_np(got), ref.taper_filter_traces(traces, tmins, DELTAT, TAPER4, _stages(filt), arrivals))


# ------------------------------------------------------------------------------------------------ end to end
def test_built_library_stacks_and_round_trips(ctx, tmp_path):
    T, P, L = 2, 5, 37
    responses, tmins, arrivals = _case(T, P, L, seed=11)
    cfg = SeismicGFLibraryConfig(component="uperp", mapnumber=2, wavename="any_P", starttime_sampling=0.5,
                                 duration_sampling=0.7)
    gfs = sl.construct_seismic_library(responses, tmins, DELTAT, arrivals, DURATIONS, STARTTIMES, TAPER, FILTERS["stepwise"],
                                       config=cfg, ctx=ctx)
    assert gfs.config is cfg and cfg.component == "uperp" and gfs.filename == "seismic_uperp_any_P_2_0"
    twin = _reference(gfs, ctx, responses, tmins, arrivals, DURATIONS, STARTTIMES, _stages("stepwise"))
    rng = np.random.default_rng(2)
    slips = rng.uniform(0.0, 2.0, P)
    for interpolation, durs, sts in (
            ("nearest_neighbor", DURATIONS[rng.integers(0, 2, P)], STARTTIMES[rng.integers(0, 3, (T, P))]),
            ("multilinear", rng.uniform(0.15, 0.75, P), rng.uniform(-0.4, 0.4, (T, P)))):
        a = gfs.stack_all(durs, sts, slips, targetidxs=np.arange(T), interpolation=interpolation)
        b = twin.stack_all(durs, sts, slips, targetidxs=np.arange(T), interpolation=interpolation)
        assert a.shape == (T, 16) and np.abs(a).max() > 0.0
        np.testing.assert_array_equal(a, b)
    gfs.save(outdir=str(tmp_path))
    back = load_gf_library(directory=str(tmp_path), filename=gfs.filename)
    np.testing.assert_array_equal(np.asarray(back._gfmatrix), gfs._device_tensor.cpu().numpy())
    np.testing.assert_array_equal(np.asarray(back._gfmatrix), twin._gfmatrix)
    np.testing.assert_array_equal(np.asarray(back._tmins), arrivals)
    assert back.dimensions == gfs.dimensions and back.config.component == "uperp" and back.config.mapnumber == 2
    assert (back.duration_min, back.duration_sampling, back.starttime_min, back.starttime_sampling) == (0.1, 0.7, -0.5, 0.5)


class _Engine(object):
    def __init__(self, T, L):
        self.T, self.L, self.calls = T, L, 0

    def elementary_seismograms(self, patches, targets):
        self.calls += 1
        responses, tmins, arrivals = _case(self.T, len(patches), self.L, seed=len(patches))
        return responses, tmins, arrivals


class _Prior(object):
    def __init__(self, lower, upper):
        self.lower, self.upper = np.atleast_1d(np.asarray(lower, dtype=float)), np.atleast_1d(np.asarray(upper, dtype=float))

    def get_lower(self, sizes):
        return np.repeat(self.lower, sizes) if self.lower.size == len(sizes) else self.lower

    def get_upper(self, sizes):
        return np.repeat(self.upper, sizes) if self.upper.size == len(sizes) else self.upper


class _Fault(object):
    """one subfault of 4 patches whose sweep onsets are 0 ... 0.9 s"""
    subfault_npatches, npatches = [4], 4

    def iter_subfaults(self):
        return iter([object()])

    def vector2subfault(self, idx, vector):
        return vector

    def get_subfault_starttimes(self, index, rupture_velocities, nuc_dip_idx, nuc_strike_idx):
        return np.array([0.0, 0.3, 0.6, 0.9])

    def get_all_patches(self, datatype, component=None):
        return [component] * 4


def test_driver_builds_one_library_per_component_and_keeps_files(ctx, tmp_path):
    wavemap = type("wm", (), {})()
    wavemap.config = type("cfg", (), dict(domain="time", name="any_P", arrival_taper=TAPER, filterer=[FILTERS["stepwise"]]))()
    wavemap.targets, wavemap.mapnumber = [0, 1], 1
    engine = _Engine(2, 37)
    args = (engine, _Fault(), _Prior(0.5, 1.5), _Prior(2.0, 4.0), _Prior(-0.6, 0.4), ["uparr", "uperp"], wavemap, None)
    kw = dict(starttime_sampling=0.5, duration_sampling=0.5, sample_rate=1.0 / DELTAT, outdirectory=str(tmp_path), ctx=ctx)
    built = sl.seis_construct_gf_linear(*args, **kw)
    starttimes, durations = sl.seismic_library_grid(0.0, 0.9, -0.6, 0.4, 0.5, 1.5, 0.5, 0.5)
    assert [g.config.component for g in built] == ["uparr", "uperp"] and engine.calls == 2
    for g in built:
        assert g.dimensions == (2, 4, durations.size, starttimes.size, 16)
        back = load_gf_library(directory=str(tmp_path), filename=g.filename)
        np.testing.assert_array_equal(np.asarray(back._gfmatrix), g._device_tensor.cpu().numpy())
    responses, tmins, arrivals = _case(2, 4, 37, seed=4)
    twin = _reference(built[0], ctx, responses, tmins, arrivals, durations, starttimes, _stages("stepwise"))
    np.testing.assert_array_equal(built[0]._device_tensor.cpu().numpy(), twin._gfmatrix)
    assert sl.seis_construct_gf_linear(*args, **kw) == [] and engine.calls == 2            # the files exist: kept
    assert len(sl.seis_construct_gf_linear(*args, force=True, **kw)) == 2 and engine.calls == 4
