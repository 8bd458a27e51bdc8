"""CPU tests of the seismic library producer (beat_amd/seislib.py, csrc/seislib.hip): the numpy restatement
(tests/seislib_ref.py) against scipy, the Butterworth restatement, the taper / grid arithmetic against the reference's
expressions, the argument rules ahead of any device call, the ABI and the kernels' resources."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import seislib_ref as ref
from beat_amd import seislib as sl, seislib_binding as sb
from conftest import ROOT

FILTER_SETS = (("high", 0.013), ("low", 0.31), ("band", [0.02, 0.4]), ("bandstop", [0.12, 0.25]))
ORDERS = range(2, 9)


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


# ------------------------------------------------------------------------------------------------ the filter arithmetic
def test_filter_recurrence_is_scipys_lfilter_bit_for_bit():
    ss = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(1).standard_normal((3, 517))
    for order in ORDERS:
        for btype, wn in FILTER_SETS:
            b, a = ss.butter(order, wn, btype)
            np.testing.assert_array_equal(ref.lfilter(b, a, x), ss.lfilter(b, a, x, axis=1), err_msg="%d %s" % (order, btype))


def test_filter_recurrence_is_scipys_lfilter_for_every_tap_count():
    """the sections tests/test_gpu_trace_lengths.py runs on the device, 3 ... 17 taps: the odd-order low- and high-passes
    (even tap counts) are not among the orders above"""
    ss = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(2).standard_normal((3, 150))
    seen = set()
    for ntaps, order, wn, btype in ref.tap_count_filters():
        b, a = sl.butter_coefficients(order, wn, btype)
        assert b.size == a.size == ntaps
        np.testing.assert_array_equal(ref.lfilter(b, a, x), ss.lfilter(b, a, x, axis=1), err_msg="%d %s" % (order, btype))
        seen.add(ntaps)
    assert seen == set(range(sb.MIN_TAPS, sb.MAX_TAPS + 1))


@pytest.mark.parametrize("L,duration", [(5, 3.3), (5, 20.0), (500, 3.3), (700, 20.0)])
def test_convolution_is_numpys_within_the_summation_order(L, duration):
    """a source-time function longer than the response (nt = 14, 81 > L = 5) and Lc = 513, 780 > 512.  Both sides add the
    products a_i g[n - i], in different orders: a sum of at most nt terms in any order is within (nt - 1) 2^-53
    sum_i |a_i g[n - i]| of the exact one to first order.  The bound held here, nt 2^-53 sum_i |a_i g[n - i]| per sample,
    is about half of the two worst cases added: a wrong index or a dropped term misses it by thirteen orders of magnitude"""
    nt, A = ref.stf_table([duration], 0.25)
    a = A[0, :nt[0]]
    assert (a.size > L) == (L == 5) and (L + a.size - 1 > 512) == (L > 5)
    g = np.random.default_rng(L + a.size).standard_normal((3, L))
    got = ref.convolve(g, a)
    assert got.shape == (3, L + a.size - 1)
    for r in range(3):
        want, mag = np.convolve(g[r], a), np.convolve(np.abs(g[r]), np.abs(a))
        ratio = float((np.abs(got[r] - want) / (a.size * 2.0 ** -53 * mag)).max())
        print("L %d nt %d row %d: largest |diff| / bound %.3g" % (L, a.size, r, ratio))
        assert ratio <= 1.0


def test_butter_coefficients_are_scipys_bit_for_bit():
    """measured where this was written: the largest |delta| / max|coef| over the sets below is 0 -- the restatement is
    bit-equal, so array_equal is asserted"""
    ss = pytest.importorskip("scipy.signal")
    sets = FILTER_SETS + (("low", 0.9), ("high", 0.5), ("band", [0.001, 0.1]), ("lowpass", 0.31), ("highpass", 0.013),
                          ("bandpass", [0.02, 0.4]))
    for order in ORDERS:
        for btype, wn in sets:
            b, a = sl.butter_coefficients(order, wn, btype)
            bs, as_ = ss.butter(order, wn, btype)
            np.testing.assert_array_equal(b, bs, err_msg="b %d %s" % (order, btype))
            np.testing.assert_array_equal(a, as_, err_msg="a %d %s" % (order, btype))
            assert a[0] == 1.0 and b.size == a.size == (order if btype in ("low", "high", "lowpass", "highpass") else 2 * order) + 1
    for bad in ((4, 1.2, "low"), (4, [0.3, 0.2], "band"), (4, 0.3, "band"), (0, 0.3, "low"), (4, 0.3, "notch")):
        with pytest.raises(ValueError):
            sl.butter_coefficients(*bad)


def test_filter_stages_follow_the_reference_filter_classes():
    deltat = 0.5
    f = sl.Filter(lower_corner=0.01, upper_corner=0.2, order=4, stepwise=True)
    assert (f.lower_corner, f.upper_corner, f.order, f.stepwise, f.ffactor) == (0.01, 0.2, 4, True, 1.5)
    assert (sl.Filter().lower_corner, sl.Filter().upper_corner, sl.Filter().order, sl.Filter().stepwise) == (0.001, 0.1, 4, True)
    bs = sl.BandstopFilter()
    assert (bs.lower_corner, bs.upper_corner, bs.order) == (0.12, 0.25, 4)
    assert f.get_freqlimits() == (0.01 / 1.5, 0.01, 0.2, 0.2 * 1.5)
    st = sl.filter_stages([f], deltat)                          # heart.py:382-385
    assert [s[2] for s in st] == [True, False]
    for (b, a, _), (btype, wn) in zip(st, (("high", 0.01 * 2.0 * deltat), ("low", 0.2 * 2.0 * deltat))):
        bb, aa = sl.butter_coefficients(4, wn, btype)
        np.testing.assert_array_equal(b, bb)
        np.testing.assert_array_equal(a, aa)
    st = sl.filter_stages(sl.Filter(0.01, 0.2, 3, stepwise=False), deltat)       # heart.py:386-392
    assert len(st) == 1 and st[0][2] is True and st[0][0].size == 7
    np.testing.assert_array_equal(st[0][1], sl.butter_coefficients(3, [0.01, 0.2], "band")[1])
    st = sl.filter_stages([sl.Filter(0.01, 0.2, 2, stepwise=False), bs], deltat)  # heart.py:405-412
    assert [s[2] for s in st] == [True, False] and st[1][0].size == 9
    np.testing.assert_array_equal(st[1][0], sl.butter_coefficients(4, [0.12, 0.25], "bandstop")[0])
    assert sl.filter_stages(None, deltat) == [] and sl.filter_stages([], deltat) == []
    assert len(sl.filter_stages(sl.Filter(0.01, 0.2, 8, stepwise=False), deltat)[0][0]) == 17     # the tap limit itself


# ------------------------------------------------------------------------------------------------ taper and grids
def test_arrival_taper_is_the_references():
    t = sl.ArrivalTaper()
    assert (t.a, t.b, t.c, t.d) == (-15.0, -10.0, 50.0, 55.0)
    assert t.duration() == 60.0 and t.duration(["a", "d"]) == 70.0 and t.fadein == 5.0 and t.fadeout == 5.0
    for taper, rate in ((t, 2.0), (sl.ArrivalTaper(-3.1, -1.3, 7.45, 9.0), 4.0), (t, 1.0 / 0.3)):
        for bounds in (["b", "c"], ["a", "d"]):
            want = int(np.ceil(rate * (getattr(taper, bounds[1]) - getattr(taper, bounds[0]))))      # heart.py:304
            assert taper.nsamples(rate, bounds) == want
    assert sl.ArrivalTaper(-3.1, -1.3, 7.45, 9.0).nsamples(4.0) == ref.nsamples((-3.1, -1.3, 7.45, 9.0), 0.25)
    t.check()
    t.check_sample_rate_consistency(0.5)
    with pytest.raises(ValueError, match="is not a whole number"):
        t.check_sample_rate_consistency(0.7)
    with pytest.raises(ValueError, match="is not a whole number"):
        sl.ArrivalTaper(-15.0, -10.0, 50.0, 55.25).check_sample_rate_consistency(0.5)       # [a, d] alone is off
    for bad in ((-10.0, -15.0, 50.0, 55.0), (-15.0, -10.0, 50.0, 50.0), (-15.0, 60.0, 50.0, 55.0)):
        with pytest.raises(ValueError, match="a < b < c < d"):
            sl.ArrivalTaper(*bad).check()


def test_library_grid_keeps_the_references_expressions():
    cases = [(0.0, 12.3, 0.0, 4.0, 0.5, 10.5, 1.0, 0.5), (0.7, 30.2, -3.5, 6.0, 1.0, 4.0, 2.0, 1.0),
             (0.0, 9.0, -5.0, 5.0, 0.0, 3.0, 2.0, 0.25), (0.0, 9.0, -2.6, 5.0, 0.0, 3.0, 4.0, 0.75)]
    differs = False
    for st_min, st_max, nl, nu, dmin, dmax, ss_, ds in cases:
        starttimes, durations = sl.seismic_library_grid(st_min, st_max, nl, nu, dmin, dmax, ss_, ds)
        idx = np.arange(int(np.floor(st_min + nl) / ss_), int(np.ceil(st_max + nu) / ss_) + 1)      # base.py:1151-1161
        np.testing.assert_array_equal(starttimes, idx * ss_)
        n = (dmax - dmin) / ds
        assert float(n).is_integer()
        np.testing.assert_array_equal(durations, np.linspace(dmin, dmax, int(n) + 1))                # base.py:1166-1173
        differs |= int(np.floor(st_min + nl) / ss_) != int(np.floor((st_min + nl) / ss_))
    assert differs      # a negative lower bound: int(floor(x) / sampling) is not floor(x / sampling), and the quirk is kept
    assert sl.seismic_library_grid(0.0, 9.0, -5.0, 5.0, 0.0, 3.0, 2.0, 0.25)[0][0] == -4.0         # int(-5 / 2) = -2
    with pytest.raises(ValueError, match="ndurations"):
        sl.seismic_library_grid(0.0, 9.0, 0.0, 5.0, 0.0, 3.1, 1.0, 0.5)


def test_window_tables_are_the_restatements():
    rng = np.random.default_rng(5)
    T, P, deltat = 3, 7, 0.25
    taper = sl.ArrivalTaper(-3.0, -1.5, 7.0, 9.0)
    arrivals, starttimes = 20.0 + rng.integers(0, 20, T) * deltat, np.arange(-2, 4) * 0.5
    tmins = np.floor(rng.uniform(5.0, 30.0, (T, P)) / deltat) * deltat
    tmins[0, 1] += 0.1          # off the sample grid: floor snapping, w0 < 1
    tmins[1, 2] -= 0.07
    i0, w0 = sl.window_tables(tmins, arrivals, starttimes, deltat, taper)
    ri0, rw0 = ref.window_tables(tmins, arrivals, starttimes, deltat, (taper.a, taper.b, taper.c, taper.d))
    assert i0.dtype == np.int64 and i0.shape == w0.shape == (T, P, starttimes.size)
    np.testing.assert_array_equal(i0, ri0)
    np.testing.assert_array_equal(w0, rw0)
    assert (w0[0, 1] < 1.0).all() and (w0[0, 1] > 0.0).all() and (w0[0, 0] == 1.0).all()
    with pytest.raises(ValueError, match="2\\^40"):
        sl.window_tables(tmins, arrivals + 1e15, starttimes, deltat, taper)


def test_reference_cut_fills_zeros_outside_the_trace():
    y = np.arange(1.0, 7.0)
    np.testing.assert_array_equal(ref.cut(y, -2, 0.5, 5), [0.0, 0.0, 1.0, 2.0, 3.0])
    np.testing.assert_array_equal(ref.cut(y, 4, 0.5, 5), [2.5, 6.0, 0.0, 0.0, 0.0])
    np.testing.assert_array_equal(ref.cut(y, 6, 0.5, 3), np.zeros(3))
    np.testing.assert_array_equal(ref.cut(y, -3, 0.5, 3), np.zeros(3))
    np.testing.assert_array_equal(ref.convolve(np.array([[1.0, 2.0, 3.0]]), np.array([0.5, 0.25])), [[0.5, 1.25, 2.0, 0.75]])
    nt, A = ref.stf_table([0.1, 0.75, 0.0], 0.25)       # below deltat / 2 -> nt == 1; 0.75 / 0.25 -> nt = 4
    assert nt.tolist() == [1, 4, 1] and A[0].tolist() == [1.0, 0.0, 0.0, 0.0] and abs(A[1].sum() - 1.0) < 4 * ref.EPS


# ------------------------------------------------------------------------------------------------ refusals, no device
def _inputs(T=2, P=3, L=20, D=2, S=3, deltat=0.5):
    rng = np.random.default_rng(3)
    return dict(responses=rng.standard_normal((T, P, L)), tmins=np.full((T, P), 10.0), deltat=deltat,
                arrival_times=np.full(T, 14.0), durations=np.arange(D) * 1.0, starttimes=np.arange(S) * 0.5,
                arrival_taper=sl.ArrivalTaper(-2.0, -1.0, 3.0, 4.0), filterer=sl.Filter(0.05, 0.4, 2))


class _NoContext(object):
    """a context that fails the test if anything reaches the binding's device calls"""
    device = 0

    def __getattr__(self, name):
        raise AssertionError("the binding was reached (%s)" % name)


def test_every_refusal_comes_before_the_binding():
    ctx = _NoContext()

    def build(**kw):
        a = _inputs()
        a.update(kw)
        return sl.construct_seismic_library(ctx=ctx, **a)

    a = _inputs()
    with pytest.raises(ValueError, match="tmins must be"):
        build(tmins=np.zeros((2, 4)))
    with pytest.raises(ValueError, match="arrival_times must be"):
        build(arrival_times=np.zeros(3))
    with pytest.raises(ValueError, match="3-d"):
        build(responses=np.zeros((2, 20)))
    for name in ("responses", "tmins", "arrival_times", "durations", "starttimes"):
        bad = np.array(a[name], dtype=np.float64)
        bad.flat[-1] = np.nan
        with pytest.raises(ValueError, match="finite"):
            build(**{name: bad})
        bad.flat[-1] = np.inf
        with pytest.raises(ValueError, match="finite"):
            build(**{name: bad})
    with pytest.raises(ValueError, match="int16"):
        build(starttimes=np.arange(32768) * 0.5)
    with pytest.raises(ValueError, match="int16"):
        build(durations=np.arange(32768) * 1e-6)
    with pytest.raises(ValueError, match="negative"):
        build(durations=np.array([-1.0, 0.0]))
    with pytest.raises(ValueError, match="evenly spaced"):
        build(starttimes=np.array([0.0, 0.5, 1.5]))
    with pytest.raises(ValueError, match="at most 4"):
        build(filterer=[sl.Filter(0.05, 0.4, 2)] * 3)                     # 6 stages
    with pytest.raises(ValueError, match="17 taps"):
        build(filterer=sl.Filter(0.05, 0.4, 9, stepwise=False))           # 19 taps
    with pytest.raises(ValueError, match="17 taps"):
        build(filterer=sl.Filter(0.05, 0.4, 17))
    with pytest.raises(ValueError, match="is not a whole number"):
        build(arrival_taper=sl.ArrivalTaper(-2.0, -1.0, 3.2, 4.0))
    with pytest.raises(ValueError, match="a < b < c < d"):
        build(arrival_taper=sl.ArrivalTaper(-1.0, -2.0, 3.0, 4.0))
    with pytest.raises(NotImplementedError, match="FrequencyFilter"):
        build(filterer=[sl.FrequencyFilter()])
    with pytest.raises(ValueError, match="deltat"):
        build(deltat=0.0)
    with pytest.raises(ValueError, match="patch_block"):
        sb.seis_library_fill(ctx, a["responses"], np.ones(1, np.int32), np.ones((1, 1)), [], np.zeros((2, 3, 1), np.int64),
                             np.ones((2, 3, 1)), 4, patch_block=0)

    def cut(**kw):
        b = dict(traces=a["responses"][0], tmins=np.full(3, 10.0), deltat=0.5, arrival_taper=a["arrival_taper"],
                 filterer=a["filterer"], arrival_times=np.full(3, 14.0))
        b.update(kw)
        return sl.taper_filter_traces(ctx=ctx, **b)

    with pytest.raises(ValueError, match="tmins must be"):
        cut(tmins=np.zeros(4))
    with pytest.raises(ValueError, match="finite"):
        cut(traces=np.full((3, 20), np.nan))
    with pytest.raises(NotImplementedError, match="FrequencyFilter"):
        cut(filterer=sl.FrequencyFilter())
    with pytest.raises(ValueError, match="is not a whole number"):
        cut(deltat=0.3)
    with pytest.raises(ValueError, match="2-d"):
        cut(traces=a["responses"])
    # the stage rules of the binding itself
    with pytest.raises(ValueError, match="normalised"):
        sb.check_stages([([1.0, 0.0, 0.0], [2.0, 0.0, 0.0], False)])
    with pytest.raises(ValueError, match="taps"):
        sb.check_stages([([1.0, 0.0], [1.0, 0.0], False)])
    with pytest.raises(ValueError, match="b has"):
        sb.check_stages([([1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], False)])
    n, ntaps, demean, coef = sb.check_stages([([0.5, 0.25, 0.125], [1.0, -0.5, 0.25], True)])
    assert (n, ntaps.tolist(), demean.tolist(), coef.shape) == (1, [3], [1], (1, 2, 17))
    assert coef[0, 0, :4].tolist() == [0.5, 0.25, 0.125, 0.0] and coef[0, 1, :3].tolist() == [1.0, -0.5, 0.25]


class _Wavemap(object):
    class config(object):
        domain = "spectrum"


def test_driver_refuses_the_spectrum_domain_and_a_missing_engine():
    with pytest.raises(TypeError, match="only supported for time-domain"):          # base.py:1119-1120
        sl.seis_construct_gf_linear(object(), None, None, None, None, ["uparr"], _Wavemap(), None)
    wm = _Wavemap()
    wm.config = type("cfg", (), {"domain": "time"})
    with pytest.raises(NotImplementedError, match="waveform engine"):
        sl.seis_construct_gf_linear(object(), None, None, None, None, ["uparr"], wm, None)


@pytest.mark.skipif(_gpu_present(), reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    from beat_amd import BeatAmdError
    a = _inputs()
    with pytest.raises(BeatAmdError):
        sl.construct_seismic_library(**a)
    with pytest.raises(BeatAmdError):
        sl.taper_filter_traces(a["responses"][0], np.full(3, 10.0), 0.5, a["arrival_taper"], None, np.full(3, 14.0))


# ------------------------------------------------------------------------------------------------ ABI, resources
NEW_ENTRIES = {"beatamd_stf_table": 7, "beatamd_trace_filter_batch": 13, "beatamd_seis_library_fill": 19}


def test_seislib_entries_are_declared_and_bound():
    from beat_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "beat_amd.h")).read()
    lib = _lib.load()
    for name, arity in NEW_ENTRIES.items():
        m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr)
        assert m, "%s is not declared" % name
        assert len(m.group(1).split(",")) == arity == len(_lib._PROTOS[name]), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for cite in ("beat/ffi/base.py:1005-1254", "beat/heart.py:3466-3525, 4242-4323", "beat/heart.py:366-412",
                 "beat/heart.py:295-304", "base.py:1013"):
        assert cite in hdr
    assert lib.beatamd_version() == 120
    hpp = open(os.path.join(ROOT, "beat_amd", "csrc", "kernels.hpp")).read()
    assert "SL_MAX_STAGES = 4, SL_MIN_TAPS = 3, SL_MAX_TAPS = 17" in hpp and "SL_NT_MAX = 65536" in hpp
    assert (sb.MAX_STAGES, sb.MIN_TAPS, sb.MAX_TAPS, sb.NT_MAX) == (4, 3, 17, 65536)
    # the source-time function's sample is one device function, shared with the moment-rate kernel
    csrc = os.path.join(ROOT, "beat_amd", "csrc")
    sources = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".cpp"))]
    defs = [f for f in sources if re.search(r"double mr_amplitude\(", open(os.path.join(csrc, f)).read())]
    assert defs == ["stf.hpp"]
    for f in ("momentrate.hip", "seislib.hip"):
        txt = open(os.path.join(csrc, f)).read()
        assert '#include "stf.hpp"' in txt and "mr_amplitude(" in txt


KERNELS = ("k_stf_table", "k_stf_convolve", "k_trace_filter", "k_library_windows")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_seislib_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "beat_amd", "csrc", "seislib.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "seislib.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    scratch, vgprs, lds, name = {}, {}, {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for key, table in ((r"ScratchSize \[bytes/lane\]: (\d+)", scratch), (r" VGPRs: (\d+)", vgprs),
                           (r"LDS Size \[bytes/block\]: (\d+)", lds)):
            m = re.search(key, line)
            if m and name:
                table[name] = int(m.group(1))
    # one k_trace_filter per tap count 3 ... 17, two window writers (16-byte stores or not)
    assert len(scratch) == 2 + 15 + 2, sorted(scratch)
    for kern in KERNELS:
        hits = [v for k, v in scratch.items() if kern in k]
        assert hits and hits == [0] * len(hits), "%s uses scratch: %s" % (kern, hits)
    filt = [k for k in scratch if "k_trace_filter" in k]
    assert max(vgprs[k] for k in filt) <= 128                 # the recurrence state stays in registers at full occupancy
    assert {lds[k] for k in filt} == {64 * 65 * 8}            # the padded 64 x 64 tile
