"""The kernels that walk whole traces along the sample axis, at real trace lengths and at every launch shape
(csrc/seislib.hip: k_stf_convolve, k_trace_filter<3 ... 17>, k_library_windows<VEC>; csrc/spectrum.hip is covered by
tests/test_gpu_spectrum.py): bit for bit against tests/seislib_ref.py, the device's own source-time functions fed to the
reference as in tests/test_gpu_seislib.py.

What each case is there for
  convolution   (3, 5): nt = 14 and 81 exceed L, the lower and the upper clamp of the sum act on the same sample;
                (3, 176): Lc = 176, 189, 256, the last trace ends on the 256-thread stride; (2, 300): Lc up to 380, a second
                trip of the sample loop; (2, 700): Lc up to 780, a third
  filter        every tap count 3 ... 17 as one stage, with and without demean, on 65 traces a duration (Q = 195: a
                workgroup of three traces) of 70, 83, 150 samples (tiles of 64: remainders 6, 19, 22); four stages of 4, 7,
                6, 5 taps; (130, 300): Q = 390 is no multiple of 64, tile remainders 44, 57, 60 in the fifth and sixth tile;
                (1, 48): Lc = 48, 61, 128, a trace that ends on a tile edge
  windows       N = 514 (16-byte stores, 257 pairs: a second trip with one lane), 512 (one trip exactly), 257 (8-byte
                stores, a second trip with one lane) out of traces of 700 ... 780 samples; windows before sample 0, past Lc,
                wholly past Lcmax and wholly before -N (the two clamps of i0), odd and even i0

The corner frequencies are those of tests/test_gpu_seislib.py (0.1 and 0.8 Hz; 0.05 and 0.4 of Nyquist).  Every section
used here keeps the reference cascade finite and below 10^3 max|x| at these corners (asserted per case; measured on the
host: at most 1.11 max|x|.  The rounded denominator of the order-15 high-pass has a root of modulus 1.03, which 150 samples
do not bring out), so no tap count needed another corner."""
import numpy as np
import pytest

import seislib_ref as ref
from beat_amd import seislib as sl, seislib_binding as sb
from beat_amd.ffi import SeismicGFLibrary, SeismicGFLibraryConfig

pytestmark = pytest.mark.gpu

DELTAT = 0.25
DURATIONS = np.array([0.1, 3.3, 20.0])                   # nt = 1, 14, 81
NT = [1, 14, 81]
STARTTIMES = np.array([-0.5, 0.0, 0.5])
STEPWISE = sl.Filter(0.1, 0.8, order=4, stepwise=True)
TAP_FILTERS = ref.tap_count_filters(0.1 * 2.0 * DELTAT, 0.8 * 2.0 * DELTAT)


def _taper(N):
    """[b, c] of N samples from one second before the arrival, fades of half a second"""
    return sl.ArrivalTaper(-1.5, -1.0, -1.0 + N * DELTAT, -0.5 + N * DELTAT)


def _taper4(t):
    return (t.a, t.b, t.c, t.d)


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.fixture(scope="module")
def table(ctx):
    """the device's source-time functions of DURATIONS, on the host, read-only"""
    nt, A = sb.stf_table(ctx, DURATIONS, DELTAT)
    assert nt.tolist() == NT and A.shape == (3, 81)
    rnt, rA = ref.stf_table(DURATIONS, DELTAT)
    assert (np.abs(A - rA) <= ref.stf_bound(rA, rnt)).all()
    nt.setflags(write=False)
    A.setflags(write=False)
    return nt, A


def _check_batch(ctx, table, traces, stages):
    """trace_filter_batch against the restatement; -> the largest |reference| / max|x| (the input condition)"""
    nt, A = table
    R, L = traces.shape
    Y = sb.trace_filter_batch(ctx, traces, nt, A, stages)
    want = ref.filtered_traces(traces, nt, A, stages)
    assert Y.shape == (R, 3, L + 80)
    growth = 0.0
    for d in range(3):
        Lc = L + NT[d] - 1
        assert want[d].shape == (R, Lc) and np.isfinite(want[d]).all()
        growth = max(growth, float(np.abs(want[d]).max() / np.abs(traces).max()))
        np.testing.assert_array_equal(Y[:, d, :Lc], want[d], err_msg="duration %d" % d)
        assert (Y[:, d, Lc:] == 0.0).all(), "duration %d: not zero beyond Lc" % d
    assert growth < 1.0e3, "the reference cascade grows to %g max|x|" % growth
    return growth


# ------------------------------------------------------------------------------------------------ 1 convolution
@pytest.mark.parametrize("R,L", [(3, 5), (3, 176), (2, 300), (2, 700)])
def test_1_convolution_is_the_restatement(ctx, table, R, L):
    traces = np.random.default_rng(R + L).standard_normal((R, L))
    if L == 5:
        assert NT[1] > L and NT[2] > L          # samples L - 1 <= n <= nt - 1: both clamps of the sum
    assert _check_batch(ctx, table, traces, []) <= 1.0 + 100 * ref.EPS      # the amplitudes are positive and add up to 1


# ------------------------------------------------------------------------------------------------ 2 filter cascade
@pytest.mark.parametrize("ntaps,order,wn,btype", TAP_FILTERS, ids=["%s%d" % (c[3], c[1]) for c in TAP_FILTERS])
def test_2_every_tap_count(ctx, table, ntaps, order, wn, btype):
    traces = np.random.default_rng(65 + 70 + ntaps).standard_normal((65, 70))
    b, a = sl.butter_coefficients(order, wn, btype)
    assert b.size == a.size == ntaps
    for demean in (True, False):
        print("%s order %d, %d taps, demean %s: reference up to %.3g max|x|"
              % (btype, order, ntaps, demean, _check_batch(ctx, table, traces, [(b, a, demean)])))


def test_2_every_tap_count_is_there():
    assert sorted(set(c[0] for c in TAP_FILTERS)) == list(range(sb.MIN_TAPS, sb.MAX_TAPS + 1))


def test_2_four_stages_of_even_and_odd_tap_counts(ctx, table):
    lo, hi = 0.1 * 2.0 * DELTAT, 0.8 * 2.0 * DELTAT
    stages = [sl.butter_coefficients(3, lo, "high") + (True,), sl.butter_coefficients(3, [lo, hi], "band") + (True,),
              sl.butter_coefficients(5, hi, "low") + (False,),
              sl.butter_coefficients(2, [0.3 * 2.0 * DELTAT, 0.5 * 2.0 * DELTAT], "bandstop") + (False,)]
    assert [s[0].size for s in stages] == [4, 7, 6, 5] and len(stages) == sb.MAX_STAGES
    traces = np.random.default_rng(4).standard_normal((65, 70))
    _check_batch(ctx, table, traces, stages)


@pytest.mark.parametrize("R,L", [(130, 300), (1, 48)])
def test_2_tile_edges(ctx, table, R, L):
    stages = sl.filter_stages(STEPWISE, DELTAT)
    assert [s[0].size for s in stages] == [5, 5]
    assert [(L + n - 1) % 64 for n in NT] == ([44, 57, 60] if L == 300 else [48, 61, 0])
    assert (R * 3) % 64 == (6 if R == 130 else 3)
    traces = np.random.default_rng(R + L).standard_normal((R, L))
    _check_batch(ctx, table, traces, stages)


# ------------------------------------------------------------------------------------------------ 3 windows
T, P, L = 2, 6, 700
LCMAX = L + 80


def _case(N):
    """responses, tmins, arrivals: the first ten (target, patch) pairs hold the window edge cases.  With target 0's arrival at
    6 s and the taper's b = -1, the window of starttime 0 begins at sample (5 - tmin) / deltat"""
    rng = np.random.default_rng(N)
    responses = rng.standard_normal((T, P, L))
    arrivals = 6.0 + 0.5 * np.arange(T)
    tmins = 3.0 + rng.integers(-4, 5, (T, P)) * DELTAT
    tmins.flat[:10] = [3.0, 3.25,                           # inside: i0 = 8 (even), 7 (odd)
                       5.75,                                # before sample 0: i0 = -3 (odd)
                       5.0 - (L - 9) * DELTAT,              # past Lc of every duration: i0 = L - 9
                       3.1, 3.0 - 0.07,                     # off the sample grid: floor snapping, a start inside the fade
                       5.0 - (LCMAX + 50) * DELTAT,         # wholly past Lcmax
                       5.0 + (N + 40) * DELTAT,             # wholly before -N
                       5.0 - LCMAX * DELTAT,                # i0 = Lcmax at starttime 0
                       5.0 + N * DELTAT]                    # i0 = -N at starttime 0
    return responses, tmins, arrivals


def _host_twin(N, duration_min, duration_sampling):
    twin = SeismicGFLibrary(SeismicGFLibraryConfig(dimensions=(T, P, 3, 3, N), starttime_sampling=0.5, starttime_min=-0.5,
                                                   duration_sampling=duration_sampling, duration_min=duration_min))
    twin.setup(T, P, 3, 3, N, allocate=True)
    return twin


WINDOW_CASES = dict(argnames="N,filt", argvalues=[(514, None), (512, None), (257, None), (514, STEPWISE)],
                    ids=["514", "512", "257", "514-stepwise"])


@pytest.mark.parametrize(**WINDOW_CASES)
def test_3_library_is_the_reference_loop(ctx, table, N, filt):
    """the source-time functions of DURATIONS (nt = 1, 14, 81).  construct_seismic_library refuses them -- a library
    addresses its durations by round((x - min) / sampling) and wants an evenly spaced grid -- so the three kernels run
    through the call it makes, seis_library_fill, and the host twin files the rows under the duration indices 0, 1, 2;
    test_3_construct_seismic_library_at_real_length runs the public entry on an even grid"""
    nt, A = table
    taper = _taper(N)
    assert taper.nsamples(1.0 / DELTAT) == N
    with pytest.raises(ValueError, match="evenly spaced"):
        sl.construct_seismic_library(np.zeros((T, P, L)), np.zeros((T, P)), DELTAT, np.zeros(T), DURATIONS, STARTTIMES, taper,
                                     None, ctx=ctx)
    responses, tmins, arrivals = _case(N)
    i0, w0 = sl.window_tables(tmins, arrivals, STARTTIMES, DELTAT, taper)
    ri0, rw0 = ref.window_tables(tmins, arrivals, STARTTIMES, DELTAT, _taper4(taper))
    np.testing.assert_array_equal(i0, ri0)
    np.testing.assert_array_equal(w0, rw0)
    stages = sl.filter_stages(filt, DELTAT)
    got = sb.seis_library_fill(ctx, responses, nt, A, stages, i0, w0, N)
    assert got.shape == (T, P, 3, 3, N)
    twin = ref.build_library(_host_twin(N, 0.0, 1.0), responses, tmins, DELTAT, arrivals, np.arange(3.0), STARTTIMES,
                             _taper4(taper), stages, nt, A)
    np.testing.assert_array_equal(got, twin._gfmatrix)
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    # the edge cases are in the inputs: assert that they occur
    lcs = [L + n - 1 for n in NT]
    assert ((i0 < 0) & (i0 + N > 0)).any(), "no window starts before sample 0"
    for Lc in lcs:
        assert ((i0 >= 0) & (i0 < Lc) & (i0 + N > Lc)).any(), "no window runs past Lc = %d" % Lc
    past, before = i0 > LCMAX, i0 < -N
    assert past.any(), "no window wholly past Lcmax"
    assert before.any(), "no window wholly before -N"
    assert (i0 == LCMAX).any() and (i0 == -N).any(), "no window on the clamps' edges"
    outside = (i0 >= LCMAX) | (i0 <= -N)
    assert (got.transpose(0, 1, 3, 2, 4)[outside] == 0.0).all()
    overlap = (i0 + N > 0) & (i0 < LCMAX)
    assert (i0[overlap] % 2 == 1).any() and (i0[overlap] % 2 == 0).any(), "no odd or no even i0"
    assert (i0[overlap & (i0 < 0)] % 2 == 1).any(), "no odd i0 before sample 0"
    raw = ((arrivals[:, None, None] - STARTTIMES[None, None, :]) + taper.b - tmins[:, :, None]) / DELTAT
    assert (np.floor(raw) != raw).any(), "no floor snapping"
    assert ((w0 > 0.0) & (w0 < 1.0)).any(), "no window starts inside the fade"
    assert (w0 == 1.0).any()


@pytest.mark.parametrize(**WINDOW_CASES)
def test_3_construct_seismic_library_at_real_length(ctx, N, filt):
    """the public entry with the same inputs on an evenly spaced duration grid (nt = 1, 41, 81; Lc = 700, 740, 780)"""
    taper = _taper(N)
    durations = np.array([0.1, 10.05, 20.0])
    responses, tmins, arrivals = _case(N)
    gfs = sl.construct_seismic_library(responses, tmins, DELTAT, arrivals, durations, STARTTIMES, taper, filt, ctx=ctx)
    assert gfs.dimensions == (T, P, 3, 3, N) and (gfs.duration_min, gfs.starttime_min, gfs.starttime_sampling) == (0.1, -0.5, 0.5)
    np.testing.assert_array_equal(gfs._tmins, arrivals)
    nt, A = (np.asarray(a) for a in sb.stf_table(ctx, durations, DELTAT))
    assert nt.tolist() == [1, 41, 81]
    twin = ref.build_library(_host_twin(N, gfs.duration_min, gfs.duration_sampling), responses, tmins, DELTAT, arrivals,
                             durations, STARTTIMES, _taper4(taper), sl.filter_stages(filt, DELTAT), nt, A)
    got = gfs._device_tensor.cpu().numpy()
    np.testing.assert_array_equal(got, twin._gfmatrix)
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0


def test_3_taper_filter_traces_at_real_length(ctx):
    R, N = 65, 514
    taper = _taper(N)
    rng = np.random.default_rng(R + N)
    traces = rng.standard_normal((R, L))
    arrivals = 6.0 + rng.integers(0, 3, R) * DELTAT
    tmins = 3.0 + rng.integers(-6, 7, R) * DELTAT
    tmins[:6] = [3.1, 5.75, 5.0 - (L - 9) * DELTAT, 5.0 - (L + 50) * DELTAT, 8.0 + (N + 40) * DELTAT, 3.25]
    i0, w0 = ref.window_tables(tmins[:, None], arrivals, np.zeros(1), DELTAT, _taper4(taper))
    i0 = i0[:, 0, 0]
    assert ((i0 < 0) & (i0 + N > 0)).any() and ((i0 < L) & (i0 + N > L)).any() and (i0 > L).any() and (i0 < -N).any()
    assert (i0 % 2 == 1).any() and (i0 % 2 == 0).any() and ((w0 > 0.0) & (w0 < 1.0)).any()
    for filt in (None, STEPWISE):
        got = sl.taper_filter_traces(traces, tmins, DELTAT, taper, filt, arrivals, ctx=ctx)
        assert got.shape == (R, N)
        want = ref.taper_filter_traces(traces, tmins, DELTAT, _taper4(taper), sl.filter_stages(filt, DELTAT), arrivals)
        np.testing.assert_array_equal(got, want)
        assert np.isfinite(got).all() and np.abs(got).max() > 0.0
