"""CPU tests of the density grids (fuzzy waveforms): the numpy restatement (tests/density_ref.py) against grids of the
reference's own ``draw_line_on_array`` (tests/golden/trace_density.npz, tools/gen_golden_density.py) bit for bit, the
default extent, the C ABI table, no CPU fallback, and the compiler's resource report of the new kernels."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_ref as dref  # noqa: E402

ENTRY = "beatamd_trace_density_update"
SHAPES = {(2, 5, 6, 1), (16, 12, 10, 1), (16, 12, 10, 7), (65, 40, 24, 3), (130, 33, 47, 7), (40, 64, 64, 2), (300, 20, 16, 7)}


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def case_shape(key):
    N, ny, nx, lw = (int(v) for v in key.split("_")[:4])
    return N, ny, nx, lw


# ------------------------------------------------------------------------------------------------- D1 twin vs the reference
def test_d1_fixture_holds_the_cases():
    g = np.load(os.path.join(ROOT, "tests", "golden", "trace_density.npz"), allow_pickle=False)
    keys = [str(k) for k in g["keys"]]
    assert {case_shape(k) for k in keys if not k.endswith("transposed")} == SHAPES
    for shape in SHAPES:
        assert {k.rsplit("_", 1)[1] for k in keys if case_shape(k) == shape} == {"unit", "small", "narrow"}
    tr = [k for k in keys if k.endswith("transposed")]
    assert len(tr) == 1 and case_shape(tr[0])[0] >= 200 and case_shape(tr[0])[2] == 8
    for k in keys:
        assert g[k + "_Y"].shape[0] == 5 and g[k + "_grid"].shape[1:] == case_shape(k)[1:3]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "trace_density.npz")) <= 200000


def test_d1_restatement_equals_the_reference_bit_for_bit(golden):
    g = golden("trace_density")
    for key in g["keys"]:
        key = str(key)
        N, ny, nx, lw = case_shape(key)
        got = dref.trace_density(g[key + "_Y"], g[key + "_tmin"], float(g[key + "_deltat"]), g[key + "_extent"], (ny, nx), lw)
        assert got.dtype == np.float64 and np.array_equal(got, g[key + "_grid"]), key
        assert g[key + "_grid"].any()
        # the last row and the last column are never written
        assert not got[:, -1, :].any() and not got[:, :, -1].any(), key
        if key.endswith("narrow"):          # the extent leaves data out: negative indices were clipped, not refused
            ext = g[key + "_extent"]
            assert g[key + "_Y"][:, 0].min() < ext[0, 2] and g[key + "_tmin"][0] < ext[0, 0]


def test_d1_restatement_adds_to_a_given_grid_in_any_split(golden):
    g = golden("trace_density")
    key = "65_40_24_3_unit"
    args = (g[key + "_tmin"], float(g[key + "_deltat"]), g[key + "_extent"], (40, 24), 3)
    Y = g[key + "_Y"]
    grid = dref.trace_density(Y[:1], *args)
    grid = dref.trace_density(Y[1:4], *args, grid=grid)
    grid = dref.trace_density(Y[4:], *args, grid=grid)
    assert np.array_equal(grid, g[key + "_grid"])


def test_d1_errors(golden):
    g = golden("trace_density")
    N, ny, nx, lw = (int(v) for v in g["err_shape"])
    args = (g["err_tmin"], float(g["err_deltat"]), g["err_extent"], (ny, nx), lw)
    with pytest.raises(TypeError, match="outside of given grid"):
        dref.trace_density(g["err_above_Y"], *args)
    with pytest.raises(ValueError):
        dref.trace_density(g["err_nan_Y"], *args)
    with pytest.raises(TypeError):                      # far below the grid: the reference's int32 products overflow
        ext = g["err_extent"].copy()
        ext[:, 2] = ext[:, 3] - 1e-6 * (ext[:, 3] - ext[:, 2])
        dref.trace_density(g["err_above_Y"] * 0.0 - 1.0, g["err_tmin"], float(g["err_deltat"]), ext, (ny, nx), lw)


# ------------------------------------------------------------------------------------------------- D2 default extent
def test_d2_density_extent_matches_the_fixture(golden):
    from beat_amd.summary import density_extent
    g = golden("trace_density")
    n = 0
    for key in g["keys"]:
        key = str(key)
        if key.endswith("narrow"):
            continue
        Y = g[key + "_Y"]
        for fn in (density_extent, dref.density_extent):
            ext = fn(Y.min(axis=0), Y.max(axis=0), g[key + "_tmin"], float(g[key + "_deltat"]))
            assert ext.shape == (Y.shape[1], 4) and np.array_equal(ext, g[key + "_extent"]), key
        n += 1
    assert n == 15
    ext = density_extent(np.array([[-3.0, 1.0], [0.5, 0.25]]), np.array([[2.0, 1.5], [0.5, 4.0]]), 2.0, 0.5)
    assert np.array_equal(ext, [[2.0, 2.5, -3.0, 3.0], [2.0, 2.5, -4.0, 4.0]])


# ------------------------------------------------------------------------------------------------- D3 ABI
def test_d3_header_entry_is_bound_with_matching_arity():
    from beat_amd import _lib
    with open(os.path.join(ROOT, "include", "beat_amd.h")) as fh:
        raw = fh.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % ENTRY, text)
    assert m, "%s is not declared in include/beat_amd.h" % ENTRY
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert nargs == 12
    assert ENTRY in _lib._PROTOS and ENTRY in _lib.EXPORTS
    assert len(_lib._PROTOS[ENTRY]) == nargs
    assert "plotting/common.py:619-801" in raw and "plotting/seismic.py:255-316" in raw
    assert _lib.EOUTSIDE == -8 and re.search(r"#define\s+BEATAMD_EOUTSIDE\s+\(-8\)", raw)
    lib = os.path.join(ROOT, "beat_amd", "libbeat_amd.so")
    if os.path.exists(lib):
        assert hasattr(_lib.load(), ENTRY)


def test_d3_context_and_summary_offer_the_calls():
    import inspect

    from beat_amd import summary
    from beat_amd.engine import Context
    sig = inspect.signature(Context.trace_density_update)
    assert list(sig.parameters)[1:] == ["Y", "tmin", "deltat", "extent", "grid_size", "linewidth", "grid"]
    assert sig.parameters["grid_size"].default == (500, 500) and sig.parameters["linewidth"].default == 7
    assert callable(summary.trace_density) and callable(summary.density_extent)
    sig = inspect.signature(summary.result_ensemble)
    assert sig.parameters["density"].default is None and sig.parameters["linewidth"].default == 7
    assert sig.parameters["tmin"].default == 0.0 and sig.parameters["deltat"].default == 1.0


# ------------------------------------------------------------------------------------------------- D4 no CPU fallback
@pytest.mark.skipif(_gpu_present(), reason="GPU present")
def test_d4_no_cpu_fallback_without_gpu(golden):
    import beat_amd
    from beat_amd import summary
    g = golden("trace_density")
    key = "16_12_10_1_unit"
    with pytest.raises(beat_amd.BeatAmdError):
        summary.trace_density(g[key + "_Y"], g[key + "_tmin"], float(g[key + "_deltat"]), g[key + "_extent"], (12, 10), 1)

    class _F(object):
        ndata = 2

        def variance_reductions(self, Q, out=None):
            raise AssertionError("reached the model without a device")

        synthetics = variance_reductions

    pop = np.zeros((5, 3))
    with pytest.raises(beat_amd.BeatAmdError):
        summary.result_ensemble(_F(), pop, pop[0], 2, density=(12, 10))


# ------------------------------------------------------------------------------------------------- D5 resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_d5_density_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "beat_amd", "csrc", "summary.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "summary.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    seen, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    for kern in ("k_trace_density_check", "k_trace_densityE"):
        hits = [v for k, v in seen.items() if kern in k]
        assert hits, "no resource report for %s:\n%s" % (kern, r.stdout[-2000:])
        assert hits == [0] * len(hits), "%s uses scratch: %s" % (kern, hits)
