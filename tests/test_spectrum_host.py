"""CPU tests of the spectrum domain of a seismic wavemap: the numpy restatement (tests/spectrum_ref.py) against the
reference's numbers (tests/golden/spectrum.npz, tools/gen_golden_spectrum.py) bit for bit, the valid-spectrum indices, the
validation of ``SeismicWavemap(domain="spectrum")``, the refusals on the host and the C ABI table."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spectrum_ref  # noqa: E402

NEW_ENTRIES = ("beatamd_amp_spectrum_batch", "beatamd_ffi_model_add_wavemap_spectrum")
MODEL_CASES = ("t3", "t2s")


def _kernel_cases(g):
    for i in range(int(g["kernel_cases"])):
        yield i, spectrum_ref.load_case(g, "k%d" % i)


# ------------------------------------------------------------------------------------------------- restatement == fixture
def test_restated_spectra_equal_the_reference(golden):
    g = golden("spectrum")
    seen = set()
    for i, c in _kernel_cases(g):
        N = c["traces"].shape[1]
        ntrans, (lo, hi) = spectrum_ref.valid_spectrum_indices(N, float(c["deltat"]), c["band"])
        assert ntrans == int(c["ntrans"]) and [lo, hi] == list(c["lohi"]), i
        assert np.array_equal(spectrum_ref.spec(c["traces"], ntrans, lo, hi), c["spectra"]), i
        seen.add((N, ntrans))
        if lo == 0:
            seen.add("dc")
        if hi == ntrans // 2 + 1:
            seen.add("nyquist")
    assert {(2, 2), (3, 4), (8, 8), (10, 16), (120, 128), (127, 128), (129, 256), "dc", "nyquist"} <= seen


def test_restated_model_cases_equal_the_reference(golden):
    g = golden("spectrum")
    assert tuple(str(n) for n in g["model_cases"]) == MODEL_CASES
    for name in MODEL_CASES:
        c = spectrum_ref.load_case(g, name)
        T, N = c["data"].shape
        ntrans, (lo, hi) = spectrum_ref.valid_spectrum_indices(N, float(c["deltat"]), c["band"])
        assert ntrans == int(c["ntrans"]) and [lo, hi] == list(c["lohi"])
        assert np.array_equal(spectrum_ref.spec(c["data"], ntrans, lo, hi), c["data_spec"])
        h0 = int(np.cumsum([int(s) for s in c["sizes"]])[-1]) - T        # h_any_P_T is the last variable
        assert str(c["names"][-1]) == "h_any_P_T"
        for key in ("nn", "ml"):
            for ch in range(c["Q"].shape[0]):
                sp = spectrum_ref.spec(c["syn_" + key][ch], ntrans, lo, hi)
                assert np.array_equal(sp, c["spec_" + key][ch]), (name, key, ch)
                res = spectrum_ref.residual(c["data_spec"], c["syn_" + key][ch], ntrans, lo, hi)
                for wk in ("scalar", "bidiag", "dense"):
                    for hps in (0, 1):
                        h = c["Q"][ch, h0:h0 + T]
                        hp = h if hps else np.full(T, h[0])
                        lp = spectrum_ref.logpt(spectrum_ref.case_weights(c, wk), c["slog"], hp, res)
                        assert np.array_equal(lp, c["logpt_%s_%s_hp%d" % (key, wk, hps)][ch]), (name, key, wk, hps, ch)
    # the cases the GPU test needs: T=3 N=10 (ntrans 16), T=2 N=120 with station shifts and a banded-size M
    t3, t2 = spectrum_ref.load_case(g, "t3"), spectrum_ref.load_case(g, "t2s")
    assert t3["data"].shape == (3, 10) and int(t3["ntrans"]) == 16 and not int(t3["has_shift"])
    assert t2["data"].shape == (2, 120) and int(t2["has_shift"]) and t2["w_bidiag"].shape[1] > 32
    assert np.count_nonzero(np.triu(t2["w_bidiag"][0], 2)) == 0 and np.count_nonzero(np.diag(t2["w_bidiag"][0], 1)) > 0


def test_get_valid_spectrum_data_equals_the_fixture(golden):
    """bands that land exactly on a bin and between bins"""
    from beat_amd import utility
    g = golden("spectrum")
    on_bin = between = 0
    for i, c in _kernel_cases(g):
        ntrans = utility.nextpow2(c["traces"].shape[1])
        assert ntrans == int(c["ntrans"])
        deltaf = 1.0 / (ntrans * float(c["deltat"]))
        assert list(utility.get_valid_spectrum_data(deltaf, list(c["band"]))) == list(c["lohi"]), i
        exact = [float(f / deltaf).is_integer() for f in c["band"]]
        on_bin += all(exact)
        between += not any(exact)
    assert on_bin >= 2 and between >= 2
    assert utility.get_valid_spectrum_data(0.125, [0.125, 0.75]) == (1, 6)
    assert utility.get_valid_spectrum_data(0.125, [0.2, 0.7]) == (1, 6)
    assert [utility.nextpow2(n) for n in (2, 3, 5, 8, 120, 128, 129, 4096, 4097)] == [2, 4, 8, 8, 128, 128, 256, 4096, 8192]


# ------------------------------------------------------------------------------------------------- validation on the host
def _wavemap(N=10, T=3, weights=None, **kw):
    from beat_amd.models import SeismicWavemap
    data = np.arange(T * N, dtype=np.float64).reshape(T, N)
    args = dict(domain="spectrum", deltat=0.5, taper_frequencies=(0.125, 0.75))
    args.update(kw)
    return SeismicWavemap({}, data, np.ones(T) if weights is None else weights, np.zeros(T), [("h", 0)] * T, **args)


def test_spectrum_wavemap_attributes():
    wm = _wavemap()
    assert wm.domain == "spectrum" and wm.ntrans == 16 and wm.valid_spectrum_indices == (1, 6)
    assert wm.nsamples_spectrum == 5 and wm.nsamples == 5 and wm.n_t == 3
    assert np.array_equal(wm.data_spec, np.abs(np.fft.rfft(wm.data, 16, axis=1))[:, 1:6])
    assert _wavemap(weights=np.zeros((3, 5, 5))).nsamples_spectrum == 5
    tm = _wavemap(domain="time", deltat=None, taper_frequencies=None)
    assert tm.domain == "time" and tm.nsamples == 10 and tm.nsamples_spectrum is None and tm.data_spec is None
    # the Nyquist bin may be the last one: hi == ntrans/2 + 1
    assert _wavemap(taper_frequencies=(0.0, 1.01)).valid_spectrum_indices == (0, 9)


@pytest.mark.parametrize("kw, text", [
    (dict(deltat=None), "deltat"),
    (dict(taper_frequencies=None), "taper_frequencies"),
    (dict(taper_frequencies=(0.0, 1.2)), "outside the 9 bins"),        # hi = 10 > ntrans/2 + 1 = 9
    (dict(taper_frequencies=(0.5, 0.4)), "spectrum indices [4, 4)"),   # lo >= hi
    (dict(taper_frequencies=(-0.2, 0.4)), "spectrum indices [-2"),
    (dict(weights=np.zeros((3, 10, 10))), "M = hi - lo spectrum samples"),   # N-sized operators instead of M-sized
    (dict(domain="frequency"), "domain must be"),
], ids=["no_deltat", "no_band", "hi_beyond_nyquist", "lo_ge_hi", "lo_negative", "weights_of_size_N", "unknown_domain"])
def test_spectrum_wavemap_validation(kw, text):
    with pytest.raises(ValueError) as e:
        _wavemap(**kw)
    assert text in str(e.value)
    if kw.get("domain") != "frequency":
        assert "spectrum" in str(e.value)


def test_transform_length_limit():
    with pytest.raises(ValueError) as e:
        _wavemap(N=8193, T=1, taper_frequencies=(0.0, 0.5))
    assert "16384" in str(e.value) and "spectrum" in str(e.value)


# ------------------------------------------------------------------------------------------------- refusals on the host
def _stub_func(wavemaps):
    """a LogpForwFunc over a problem description alone: no context, no device model -- a refusal has to come first"""
    from types import SimpleNamespace

    from beat_amd.models.problem import LogpForwFunc
    f = LogpForwFunc.__new__(LogpForwFunc)
    f.ctx, f.model_id, f._dirty = None, 0, None
    f.problem = SimpleNamespace(wavemaps=list(wavemaps), laplacian=(np.eye(2), 0.0), geodetic=None, slip_varnames=["uparr"],
                                layout=SimpleNamespace(size=4))
    f.nparams = 4
    return f


def test_refusals_name_the_spectrum_domain():
    from beat_amd.covariance import NoiseCovarianceUpdate
    from beat_amd.models.sharded import TargetShardedLogp
    wm = _wavemap()
    with pytest.raises(ValueError, match="spectrum domain"):
        wm.prewhitened()
    with pytest.raises(ValueError, match="spectrum domain"):
        _wavemap(weights=np.zeros((3, 5, 5))).prewhitened()
    f = _stub_func([_wavemap(domain="time", deltat=None, taper_frequencies=None), wm])
    Q = np.zeros((1, 4))
    for call in (lambda: f.lsq_normal_equations(Q), lambda: f.lsq_solution(Q),
                 lambda: f.standardized_residuals(Q, [1.0] * 3, wavemap_index=1), lambda: NoiseCovarianceUpdate(f),
                 lambda: TargetShardedLogp(f.problem)):
        with pytest.raises(NotImplementedError, match="spectrum domain"):
            call()


def test_lsq_start_population_refuses_a_spectrum_wavemap():
    from beat_amd.models import lsq
    f = _stub_func([_wavemap()])
    with pytest.raises(NotImplementedError, match="spectrum domain"):
        lsq.lsq_start_population(f, 2, 1, lower=np.zeros(4), upper=np.ones(4))


def test_fft_transforms_signature_and_outmodes():
    import inspect

    from beat_amd import heart
    sig = inspect.signature(heart.fft_transforms)
    assert list(sig.parameters)[:4] == ["time_domain_signals", "valid_spectrum_indices", "outmode", "pad_to_pow2"]
    assert sig.parameters["outmode"].default == "array" and sig.parameters["pad_to_pow2"].default is True
    with pytest.raises(TypeError, match="not supported"):
        heart.fft_transforms(np.zeros((1, 8)), (0, 2), outmode="data")
    with pytest.raises(NotImplementedError, match="power-of-two"):
        heart.fft_transforms(np.zeros((1, 10)), (0, 2), pad_to_pow2=False)


# ------------------------------------------------------------------------------------------------- C ABI
def test_new_entry_points_are_declared_bound_and_exported():
    from beat_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "beat_amd.h")).read()
    declared = set(re.findall(r"\b(beatamd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib._PROTOS and hasattr(lib, name), name
    # the argument counts of the prototypes are the header's
    for name in NEW_ENTRIES:
        args = re.search(name + r"\s*\(([^;]*)\);", hdr).group(1)
        assert len(_lib._PROTOS[name]) == args.count(",") + 1, name
    for cite in ("heart.py:4091-4155", "heart.py:3086-3095", "pytensorf.py:199-206", "utility.py:1604-1610",
                 "seismic.py:1277-1278", "seismic.py:932-941", "covariance.py:133-135"):
        assert cite in hdr, cite
    src = open(os.path.join(ROOT, "beat_amd", "csrc", "Makefile")).read()
    assert "spectrum.hip" in src


def test_no_gpu_means_an_error_not_a_fallback():
    try:
        import torch
        if torch.cuda.is_available():
            return      # (with a GPU the call below is tests/test_gpu_spectrum.py's)
    except ImportError:
        pass
    from beat_amd import heart
    with pytest.raises(Exception):
        heart.fft_transforms(np.zeros((2, 8)), (0, 5))
