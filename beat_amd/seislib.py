"""
Build seismic FFI Green's-function libraries on the device -- the counterpart of ``seis_construct_gf_linear`` /
``_process_patch_seismic`` (reference beat/ffi/base.py:1005-1254) and of ``heart.taper_filter_traces`` /
``post_process_trace`` (beat/heart.py:3466-3525, 4242-4323).

The reference builds the 5-D library (ntargets, npatches, ndurations, nstarttimes, nsamples) with one process per patch
and a Python loop over targets x durations x starttimes.  Here the elementary responses of all (target, patch) pairs go to
the GPU once; the convolution with the source-time function of every duration, the Butterworth filters and the cut of one
window per starttime run there (csrc/seislib.hip, which states the arithmetic contract), and the library is written
straight into a torch tensor in HBM that ``SeismicGFLibrary.adopt_device_tensor`` takes without a host copy.

What is NOT here: the elementary waveforms themselves.  In the reference they come from pyrocko's ``engine.process`` on a
GF store (heart.seis_synthetics, beat/heart.py:3564-3762); the package ships no waveform engine (see
``beat_amd.heart.seis_synthetics``).  The caller provides them: ``responses[t, p, :]`` is the unit-slip response of patch
``p`` at target ``t`` for an impulsive source-time function, sampled at ``deltat``; ``tmins[t, p]`` is the time of its
sample 0 relative to the event's origin time, which lies on the sample grid (the reference's ``patch.time = event.time``,
base.py:1010); ``arrival_times[t]`` is the event's phase arrival at the target, which becomes the library's ``_tmins``
(base.py:1044).

Recalled, UNVERIFIED against pyrocko (it is not installed where this was written): ``HalfSinusoidSTF.discretize_t``
(the source-time function, as in csrc/momentrate.hip), ``Trace.lowpass / highpass / bandpass / bandstop`` (a Butterworth
``scipy.signal.butter(order, corner * 2 * deltat)`` run through ``lfilter``, preceded by a demean where asked),
``Trace.extend(fillmethod="zeros")``, ``Trace.taper`` with a ``CosTaper`` and ``Trace.chop(snap=(floor, floor))``.
Deviations: a demean divides the sum taken in sample order (numpy's mean is pairwise); the source-time function is
normalised in the fixed order of the moment-rate kernel.  Out of scope: downsampling (``deltat=`` of
post_process_trace), ``transfer_function``, chop bounds other than ["b", "c"], ``FrequencyFilter``.
"""
import os

import numpy as np

from . import seislib_binding as sb
from ._marshal import is_dev, upload
from .engine import get_context
from .ffi import SeismicGFLibrary, SeismicGFLibraryConfig, _time2idx

__all__ = ["ArrivalTaper", "Filter", "BandstopFilter", "FrequencyFilter", "butter_coefficients", "filter_stages",
           "seismic_library_grid", "window_tables", "taper_filter_traces", "construct_seismic_library",
           "seis_construct_gf_linear", "error_not_whole"]


def error_not_whole(f, errstr=""):
    """beat/utility.py:1374-1381"""
    f = float(f)
    if f.is_integer():
        return int(f)
    raise ValueError("%s : %f is not a whole number!" % (errstr, f))


class ArrivalTaper(object):
    """Cosine arrival taper, times [s] relative to the phase arrival (beat/heart.py:266-335)."""

    def __init__(self, a=-15.0, b=-10.0, c=50.0, d=55.0):
        self.a, self.b, self.c, self.d = float(a), float(b), float(c), float(d)

    def check(self):
        """heart.py:327-328"""
        if not self.a < self.b < self.c < self.d:
            raise ValueError("Taper values violate: a < b < c < d")

    def duration(self, chop_bounds=("b", "c")):
        return getattr(self, chop_bounds[1]) - getattr(self, chop_bounds[0])

    def nsamples(self, sample_rate, chop_bounds=("b", "c")):
        """heart.py:295-304"""
        return int(np.ceil(sample_rate * self.duration(chop_bounds)))

    def check_sample_rate_consistency(self, deltat):
        """heart.py:276-288"""
        for chop_b in (["b", "c"], ["a", "d"]):
            duration = self.duration(chop_b)
            error_not_whole(duration / deltat,
                            errstr="Taper duration %g of %s is inconsistent with sampling rate of %g! Please adjust Taper "
                                   "values!" % (duration, ", ".join(chop_b), deltat))

    fadein = property(lambda self: self.b - self.a)
    fadeout = property(lambda self: self.d - self.c)


class _FilterBase(object):
    def __init__(self, lower_corner, upper_corner, ffactor=1.5):
        self.lower_corner, self.upper_corner, self.ffactor = float(lower_corner), float(upper_corner), ffactor

    def get_lower_corner(self):
        return self.lower_corner

    def get_upper_corner(self):
        return self.upper_corner

    def get_freqlimits(self):
        return (self.lower_corner / self.ffactor, self.lower_corner, self.upper_corner, self.upper_corner * self.ffactor)


class Filter(_FilterBase):
    """Time-domain band limitation (heart.py:366-392): ``stepwise`` runs a highpass (with demean) and then a lowpass
    (without), otherwise one bandpass (with demean)."""

    def __init__(self, lower_corner=0.001, upper_corner=0.1, order=4, stepwise=True, ffactor=1.5):
        super(Filter, self).__init__(lower_corner, upper_corner, ffactor)
        self.order, self.stepwise = int(order), bool(stepwise)


class BandstopFilter(_FilterBase):
    """Suppressed frequency band (heart.py:395-412): one bandstop without demean."""

    def __init__(self, lower_corner=0.12, upper_corner=0.25, order=4, ffactor=1.5):
        super(BandstopFilter, self).__init__(lower_corner, upper_corner, ffactor)
        self.order = int(order)


class FrequencyFilter(_FilterBase):
    """The spectral filter of heart.py:415-437 (pyrocko ``Trace.transfer``): kept so that a configuration holding one is
    refused with a message by ``filter_stages``; it has no device counterpart."""

    def __init__(self, lower_corner=0.001, upper_corner=0.1, tfade=20.0, ffactor=1.5):
        super(FrequencyFilter, self).__init__(lower_corner, upper_corner, ffactor)
        self.tfade = float(tfade)


def butter_coefficients(order, wn, btype):
    """(b, a) of the digital Butterworth filter ``scipy.signal.butter(order, wn, btype)``: wn in units of the Nyquist
    frequency, a scalar for "low" / "high", a pair for "band" / "bandstop".  A numpy restatement of scipy's path: analog
    prototype poles, frequency transform of the poles and zeros, bilinear transform, polynomials (numpy.poly)."""
    order = int(order)
    if order < 1:
        raise ValueError("filter order must be at least 1, got %d" % order)
    wn = np.atleast_1d(np.asarray(wn, dtype=np.float64))
    kinds = {"low": "low", "lowpass": "low", "high": "high", "highpass": "high", "band": "band", "bandpass": "band",
             "bandstop": "stop", "stop": "stop"}
    if btype not in kinds:
        raise ValueError("unknown filter type %r" % (btype,))
    kind = kinds[btype]
    if wn.size != (1 if kind in ("low", "high") else 2):
        raise ValueError("%s needs %d corner frequencies, got %d" % (btype, 1 if kind in ("low", "high") else 2, wn.size))
    if not np.all((wn > 0.0) & (wn < 1.0)) or (wn.size == 2 and not wn[0] < wn[1]):
        raise ValueError("corner frequencies must satisfy 0 < wn < 1 (Nyquist) and increase, got %s" % wn.tolist())
    # buttap
    z = np.array([])
    p = -np.exp(1j * np.pi * np.arange(-order + 1, order, 2) / (2 * order))
    k = 1.0
    fs = 2.0
    warped = 2 * fs * np.tan(np.pi * wn / fs)
    degree = p.size - z.size
    if kind == "low":
        wo = float(warped[0])
        z, p, k = wo * z, wo * p, k * wo ** degree
    elif kind == "high":
        wo = float(warped[0])
        k = k * np.real(np.prod(-z) / np.prod(-p))
        z, p = np.append(wo / z, np.zeros(degree)), wo / p
    else:
        bw, wo = float(warped[1] - warped[0]), float(np.sqrt(warped[0] * warped[1]))
        if kind == "band":
            z_lp, p_lp = (z * bw / 2).astype(complex), (p * bw / 2).astype(complex)
            k = k * bw ** degree
            z = np.concatenate((z_lp + np.sqrt(z_lp ** 2 - wo ** 2), z_lp - np.sqrt(z_lp ** 2 - wo ** 2)))
            p = np.concatenate((p_lp + np.sqrt(p_lp ** 2 - wo ** 2), p_lp - np.sqrt(p_lp ** 2 - wo ** 2)))
            z = np.append(z, np.zeros(degree))
        else:
            k = k * np.real(np.prod(-z) / np.prod(-p))
            z_hp, p_hp = ((bw / 2) / z).astype(complex), ((bw / 2) / p).astype(complex)
            z = np.concatenate((z_hp + np.sqrt(z_hp ** 2 - wo ** 2), z_hp - np.sqrt(z_hp ** 2 - wo ** 2)))
            p = np.concatenate((p_hp + np.sqrt(p_hp ** 2 - wo ** 2), p_hp - np.sqrt(p_hp ** 2 - wo ** 2)))
            z = np.append(z, np.full(degree, +1j * wo))
            z = np.append(z, np.full(degree, -1j * wo))
    # bilinear_zpk
    degree = p.size - z.size
    fs2 = 2.0 * fs
    k = k * np.real(np.prod(fs2 - z) / np.prod(fs2 - p))
    z, p = np.append((fs2 + z) / (fs2 - z), -np.ones(degree)), (fs2 + p) / (fs2 - p)
    # zpk2tf: the roots come in conjugate pairs, the polynomials are real
    b, a = k * np.poly(z), np.poly(p)
    return np.ascontiguousarray(np.real(b), dtype=np.float64), np.ascontiguousarray(np.real(a), dtype=np.float64)


def filter_stages(filterer, deltat):
    """The filter cascade of a ``filterer`` (None, one filter object or a list of them, applied in order as
    post_process_trace does, heart.py:3504-3507) at the sampling interval ``deltat``: a list of (b, a, demean).

      Filter(stepwise=True)    highpass at lower_corner with demean, then lowpass at upper_corner without
      Filter(stepwise=False)   one bandpass with demean (pyrocko's default, as recalled)
      BandstopFilter           one bandstop without demean
      FrequencyFilter          refused: the spectral ``transfer`` has no device counterpart"""
    deltat = sb.check_deltat(deltat)
    if filterer is None:
        return []
    filters = list(filterer) if isinstance(filterer, (list, tuple)) else [filterer]
    stages = []
    for f in filters:
        if isinstance(f, FrequencyFilter) or type(f).__name__ == "FrequencyFilter":
            raise NotImplementedError("FrequencyFilter (spectral transfer, beat/heart.py:415-437) is not supported by the "
                                      "device library producer: use Filter or BandstopFilter")
        lo, hi = f.lower_corner * 2.0 * deltat, f.upper_corner * 2.0 * deltat
        if isinstance(f, BandstopFilter) or type(f).__name__ == "BandstopFilter":
            stages.append(butter_coefficients(f.order, [lo, hi], "bandstop") + (False,))
        elif isinstance(f, Filter) or type(f).__name__ == "Filter":
            if f.stepwise:
                stages.append(butter_coefficients(f.order, lo, "high") + (True,))
                stages.append(butter_coefficients(f.order, hi, "low") + (False,))
            else:
                stages.append(butter_coefficients(f.order, [lo, hi], "band") + (True,))
        else:
            raise TypeError("unknown filter %r (Filter, BandstopFilter)" % (f,))
    sb.check_stages(stages)
    return stages


def seismic_library_grid(st_min, st_max, nucleation_lower_min, nucleation_upper_max, durations_min, durations_max,
                         starttime_sampling=1.0, duration_sampling=1.0):
    """The starttime and duration grids of a library (base.py:1151-1173) from the smallest / largest rupture onset of the
    sweep (hypocentre at the fault's corner, time shifts included: ``min(st_mins)``, ``max(st_maxs)``) and the bounds of
    the nucleation-time and duration priors -> (starttimes, durations).  The reference's expressions are kept as they
    are: ``int(floor(x) / sampling)`` truncates toward zero after the division, and a duration range that is no whole
    multiple of the sampling is an error."""
    starttimeidxs = np.arange(
        int(np.floor(st_min + nucleation_lower_min) / starttime_sampling),
        int(np.ceil(st_max + nucleation_upper_max) / starttime_sampling) + 1)
    starttimes = starttimeidxs * starttime_sampling
    ndurations = error_not_whole((durations_max - durations_min) / duration_sampling, errstr="ndurations") + 1
    durations = np.linspace(durations_min, durations_max, ndurations)
    return starttimes, durations


def window_tables(tmins, arrival_times, starttimes, deltat, arrival_taper):
    """The two tables the window kernel reads, for tmins (T, P), arrival_times (T,), starttimes (S,):

      i0 int64 (T, P, S)  the first sample of the cut: with lower = (arrival - starttime) + b,
                          floor((lower - tmin) / deltat) -- chop's snap=(floor, floor), heart.py:3522
      w0 (T, P, S)        the taper's value at that sample's time t0 = tmin + i0 deltat: the cosine fade-in
                          0.5 (1 - cos(pi (t0 - a') / (b' - a'))) where t0 < b' (0 at or below a'), 1 otherwise; a', b' are
                          the taper edges shifted by the arrival.  Only sample 0 of a [b, c] cut can lie in the fade."""
    tm = np.asarray(tmins, dtype=np.float64)[:, :, None]
    shifted = np.asarray(arrival_times, dtype=np.float64)[:, None, None] - np.asarray(starttimes, dtype=np.float64)[None, None, :]
    lower, fade_start = shifted + arrival_taper.b, shifted + arrival_taper.a
    idx = np.floor((lower - tm) / deltat)
    if not np.all(np.abs(idx) < 2.0 ** 40):
        raise ValueError("a window starts more than 2^40 samples from its trace: check tmins, arrival_times and starttimes")
    t0 = tm + idx * deltat
    fade = 0.5 * (1.0 - np.cos(np.pi * (t0 - fade_start) / (lower - fade_start)))
    w0 = np.where(t0 < lower, np.where(t0 <= fade_start, 0.0, fade), 1.0)
    return np.ascontiguousarray(idx.astype(np.int64)), np.ascontiguousarray(w0)


def _window_inputs(deltat, arrival_taper):
    deltat = sb.check_deltat(deltat)
    arrival_taper.check()
    arrival_taper.check_sample_rate_consistency(deltat)
    return deltat, arrival_taper.nsamples(1.0 / deltat)


def _host_vector(a, n, what):
    a = np.asarray(sb._host(a), dtype=np.float64)
    if a.shape != (n,):
        raise ValueError("%s must be (%d,), got %s" % (what, n, a.shape))
    sb._finite(a, what)
    return a


def taper_filter_traces(traces, tmins, deltat, arrival_taper, filterer, arrival_times, ctx=None):
    """``heart.taper_filter_traces(outmode="array")`` (heart.py:4242-4323) for a batch of observed or synthetic traces:
    traces (R, L) sampled at ``deltat`` with sample 0 at tmins (R,), filtered by ``filterer``, zero-extended, tapered and
    cut to [b, c] of ``arrival_taper`` around arrival_times (R,) -> (R, nsamples), on the side of ``traces``.  The kernels
    are the library producer's, with no source-time function and one window a trace."""
    deltat, N = _window_inputs(deltat, arrival_taper)
    stages = filter_stages(filterer, deltat)
    X = sb.check_traces(traces, 2, "traces")
    R, L = int(X.shape[0]), int(X.shape[1])
    tm, arr = _host_vector(tmins, R, "tmins"), _host_vector(arrival_times, R, "arrival_times")
    i0, w0 = window_tables(tm[:, None], arr, np.zeros(1), deltat, arrival_taper)
    ctx = ctx or get_context()
    nt, A = sb.unit_stf(X)
    lib = sb.seis_library_fill(ctx, X.reshape(R, 1, L), nt, A, stages, i0, w0, N)
    return lib.reshape(R, N)


def construct_seismic_library(responses, tmins, deltat, arrival_times, durations, starttimes, arrival_taper, filterer,
                              config=None, patch_block=None, ctx=None):
    """Fill a seismic FFI library on the device: what ``_process_patch_seismic`` (base.py:1005-1064) does for every patch.

    responses (T, P, L), numpy or a torch CUDA tensor (see the module text); tmins (T, P); arrival_times (T,);
    durations (D,), starttimes (S,): ascending, evenly spaced grids (the library addresses them by
    ``round((x - min) / sampling)``); arrival_taper, filterer: as in the wavemap's configuration.  ``config``: a
    ``SeismicGFLibraryConfig`` whose component / wave name / map number are kept (its dimensions, samplings and minima
    are set here); ``patch_block``: the patches filtered at a time (None: all), which bounds the intermediate buffer of
    T * patch_block * D * (L + ntmax - 1) doubles and does not change the result.

    -> a ``SeismicGFLibrary`` holding the library as a torch tensor in HBM (``adopt_device_tensor``), ``_tmins`` set to
    the arrival times; ``save()`` writes the reference's files."""
    deltat, N = _window_inputs(deltat, arrival_taper)
    stages = filter_stages(filterer, deltat)
    X = sb.check_traces(responses, 3, "responses")
    T, P, L = (int(v) for v in X.shape)
    tm = np.asarray(sb._host(tmins), dtype=np.float64)
    if tm.shape != (T, P):
        raise ValueError("tmins must be (%d, %d), got %s" % (T, P, tm.shape))
    sb._finite(tm, "tmins")
    arr = _host_vector(arrival_times, T, "arrival_times")
    dur, _ = sb.check_durations(durations, deltat)
    st = sb.check_grid(starttimes, "starttimes")
    cfg = config or SeismicGFLibraryConfig()
    cfg.dimensions = (T, P, dur.size, st.size, N)
    for name, grid in (("duration", dur), ("starttime", st)):
        if config is None and grid.size > 1:     # (a given config states its samplings)
            setattr(cfg, name + "_sampling", float((grid[-1] - grid[0]) / (grid.size - 1)))
        setattr(cfg, name + "_min", float(grid.min()))
        lo, step = getattr(cfg, name + "_min"), getattr(cfg, name + "_sampling")
        idx, _ = _time2idx(grid, lo, step, "nearest_neighbor")
        if step <= 0.0 or not np.array_equal(idx, np.arange(grid.size)) or \
                np.abs(grid - (lo + np.arange(grid.size) * step)).max() > 1e-6 * step:
            raise ValueError("%ss must form an ascending, evenly spaced grid, got %s" % (name, grid.tolist()))
    i0, w0 = window_tables(tm, arr, st, deltat, arrival_taper)
    ctx = ctx or get_context()
    if not is_dev(X):
        X = upload(X, "cuda:%d" % ctx.device, np.float64)
    nt, A = sb.stf_table(ctx, dur, deltat, like=X)
    tensor = sb.seis_library_fill(ctx, X, nt, A, stages, i0, w0, N, patch_block=patch_block)
    gfs = SeismicGFLibrary(config=cfg)
    gfs.adopt_device_tensor(tensor)
    gfs._tmins = arr.copy()
    return gfs


def seis_construct_gf_linear(engine, fault, durations_prior, velocities_prior, nucleation_time_prior, varnames, wavemap, event,
                             nworkers=1, time_shift=None, starttime_sampling=1.0, duration_sampling=1.0, sample_rate=1.0,
                             outdirectory="./", force=False, patch_block=None, ctx=None):
    """The reference's driver (base.py:1067-1254) with its control flow: the starttime and duration grids from the priors
    and a rupture sweep from the fault's corner, then one library per slip component in ``varnames``, saved under
    ``outdirectory``; an existing file is kept unless ``force``.  ``nworkers`` is accepted and unused (one GPU call
    replaces the process pool).

    ``engine`` is anything offering ``elementary_seismograms(patches, targets) -> (responses (T, P, L), tmins (T, P),
    arrival_times (T,))`` -- the unit-slip responses for an impulsive source-time function at ``sample_rate``.  The
    package ships no waveform engine (in the reference: pyrocko GF stores, heart.seis_synthetics); INTEGRATION.md shows
    one built on pyrocko.  -> the list of libraries built (not the ones kept)."""
    if wavemap.config.domain == "spectrum":
        raise TypeError("FFI is currently only supported for time-domain!")
    if not hasattr(engine, "elementary_seismograms"):
        raise NotImplementedError(
            "seis_construct_gf_linear needs a waveform engine offering elementary_seismograms(patches, targets) (pyrocko "
            "GF stores in the reference); none is part of this package")
    st_mins, st_maxs = [], []
    for idx, sf in enumerate(fault.iter_subfaults()):
        try:
            rupture_velocities = fault.vector2subfault(idx, velocities_prior.get_lower(fault.subfault_npatches))
        except IndexError:
            raise ValueError("Velocities need to be of size either npatches or number of fault segments")
        start_times = fault.get_subfault_starttimes(index=idx, rupture_velocities=rupture_velocities, nuc_dip_idx=0,
                                                    nuc_strike_idx=0)
        if time_shift is not None:
            shift_times_min, shift_times_max = time_shift.lower.min(), time_shift.upper.max()
        else:
            shift_times_min = shift_times_max = 0.0
        st_mins.append(start_times.min() + shift_times_min)
        st_maxs.append(start_times.max() + shift_times_max)
    starttimes, durations = seismic_library_grid(
        min(st_mins), max(st_maxs), nucleation_time_prior.lower.min(), nucleation_time_prior.upper.max(),
        durations_prior.get_lower(fault.subfault_npatches).min(), durations_prior.get_upper(fault.subfault_npatches).max(),
        starttime_sampling, duration_sampling)
    wc = wavemap.config
    built = []
    for var in varnames:
        cfg = SeismicGFLibraryConfig(component=var, datatype="seismic", duration_sampling=duration_sampling,
                                     starttime_sampling=starttime_sampling, starttime_min=float(starttimes.min()),
                                     duration_min=float(durations.min()), mapnumber=wavemap.mapnumber, wavename=wc.name)
        probe = SeismicGFLibrary(config=cfg)
        if os.path.exists(os.path.join(outdirectory, probe.filename + ".traces.npy")) and not force:
            continue      # base.py:1208-1211: "Library exists ... Please use --force to override!"
        patches = fault.get_all_patches("seismic", component=var)
        responses, tmins, arrival_times = engine.elementary_seismograms(patches, wavemap.targets)
        gfs = construct_seismic_library(responses, tmins, 1.0 / sample_rate, arrival_times, durations, starttimes,
                                        wc.arrival_taper, wc.filterer, config=cfg, patch_block=patch_block, ctx=ctx)
        gfs.save(outdir=outdirectory)
        built.append(gfs)
    return built
