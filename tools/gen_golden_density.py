"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/trace_density.npz by running the REFERENCE's own ``draw_line_on_array`` on seeded inputs.  Needs the
reference tree (oracle/ref_import.py finds it) and matplotlib, so it runs where that tree is mounted; the fixture it
writes is data (inputs and expected outputs, none of the reference's text).

    python tools/gen_golden_density.py

Reference entry points exercised:
  beat/plotting/common.py:700-801    draw_line_on_array(X, Y, grid, extent, grid_resolution, linewidth), called once per
                                     trace on one grid, as fuzzy_waveforms does (beat/plotting/seismic.py:293-303)
  beat/plotting/common.py:619-697    _weighted_line (through draw_line_on_array)
  beat/utility.py:1556               positions2idxs (through draw_line_on_array)

The default extent of fuzzy_waveforms (seismic.py:282-291) needs pyrocko traces; its arithmetic -- time span of the
traces, amplitudes symmetric about zero -- is applied here to the arrays.

Cases: key "<N>_<ny>_<nx>_<lw>_<kind>", each with Y (E, T, N), tmin (T,), deltat (), extent (T, 4), grid (T, ny, nx);
kinds unit / small (two amplitudes, default extent) and narrow (an extent that leaves data out on the low side of both
axes: negative indices, clipped).  "transposed": many samples per column.  err_above / err_nan: inputs the reference
raises TypeError on / that hold a NaN (no grid).
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

ref_import.install()
# beat/plotting/__init__ imports every plotting module (and with them the compiled sweep extension): an empty package
# with the directory as its path lets the one module be imported on its own
_pkg = types.ModuleType("beat.plotting")
_pkg.__path__ = [os.path.join(ref_import.REFERENCE_ROOT, "beat", "plotting")]
sys.modules["beat.plotting"] = _pkg
common = importlib.import_module("beat.plotting.common")

GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = ((2, 5, 6, 1), (16, 12, 10, 1), (16, 12, 10, 7), (65, 40, 24, 3), (130, 33, 47, 7), (40, 64, 64, 2),
          (300, 20, 16, 7))
TRANSPOSED = (256, 64, 8, 3)
E, T = 5, 1


def _traces(rng, N, amp):
    """(E, T, N): a few sinusoids and noise -- flat stretches, steep flanks, both signs"""
    j = np.arange(N)
    Y = np.empty((E, T, N))
    for e in range(E):
        for t in range(T):
            f = rng.uniform(0.5, 6.0, 3) / max(N, 2)
            ph = rng.uniform(0, 2 * np.pi, 3)
            a = rng.uniform(0.2, 1.0, 3)
            Y[e, t] = (a[:, None] * np.sin(2 * np.pi * f[:, None] * j[None, :] + ph[:, None])).sum(0) \
                + 0.15 * rng.standard_normal(N)
    # float32-representable values: the low mantissa bits are zero and the fixture compresses to within 200 kB
    return (amp * Y).astype(np.float32).astype(np.float64)


def _default_extent(Y, tmin, deltat):
    N = Y.shape[2]
    ext = np.empty((T, 4))
    for t in range(T):
        X = tmin[t] + np.arange(N, dtype=np.float64) * deltat
        ymin, ymax = Y[:, t].min(), Y[:, t].max()
        ymax = max(abs(ymin), abs(ymax))
        ext[t] = [X.min(), X.max(), -ymax, ymax]
    return ext


def _reference_grid(Y, tmin, deltat, extent, ny, nx, lw):
    grids = np.zeros((T, ny, nx))
    for t in range(T):
        X = tmin[t] + np.arange(Y.shape[2], dtype=np.float64) * deltat
        for e in range(Y.shape[0]):
            common.draw_line_on_array(X, Y[e, t], grid=grids[t], extent=list(extent[t]), grid_resolution=(ny, nx),
                                      linewidth=lw)
    return grids


def _case(out, key, rng, N, ny, nx, lw, kind):
    amp = {"unit": 1.0, "small": 3.7e-6, "narrow": 1.0}[kind]
    deltat = float(rng.choice([0.5, 0.1, 2.0]))
    tmin = rng.uniform(-50.0, 50.0, T)
    Y = _traces(rng, N, amp)
    extent = _default_extent(Y, tmin, deltat)
    if kind == "narrow":
        span = extent[:, 1] - extent[:, 0]
        extent[:, 0] += 0.3 * span                      # the first third of every trace lies left of the grid
        extent[:, 2] *= 0.4                             # and what is below -0.4 a lies under it
    out[key + "_Y"], out[key + "_tmin"], out[key + "_deltat"], out[key + "_extent"] = Y, tmin, np.float64(deltat), extent
    out[key + "_grid"] = _reference_grid(Y, tmin, deltat, extent, ny, nx, lw)


def main():
    rng = np.random.default_rng(20261017)
    out, keys = {}, []
    for (N, ny, nx, lw) in SHAPES:
        for kind in ("unit", "small", "narrow"):
            key = "%d_%d_%d_%d_%s" % (N, ny, nx, lw, kind)
            _case(out, key, rng, N, ny, nx, lw, kind)
            keys.append(key)
    N, ny, nx, lw = TRANSPOSED
    key = "%d_%d_%d_%d_transposed" % TRANSPOSED
    _case(out, key, rng, N, ny, nx, lw, "unit")
    keys.append(key)
    out["keys"] = np.array(keys)

    # the two error inputs, on the (65, 40, 24, 3) shape
    N, ny, nx, lw = 65, 40, 24, 3
    Y = _traces(rng, N, 1.0)
    tmin, deltat = rng.uniform(-5.0, 5.0, T), 0.5
    extent = _default_extent(Y, tmin, deltat)
    above = Y.copy()
    above[3, 0, 17] = 1.5 * extent[0, 3]
    raised = False
    try:
        _reference_grid(above, tmin, deltat, extent, ny, nx, lw)
    except TypeError:
        raised = True
    assert raised, "the reference did not raise on a sample above ymax"
    nan = Y.copy()
    nan[2, 0, 40] = np.nan
    out["err_shape"] = np.array([N, ny, nx, lw])
    out["err_tmin"], out["err_deltat"], out["err_extent"] = tmin, np.float64(deltat), extent
    out["err_above_Y"], out["err_nan_Y"] = above, nan

    path = os.path.join(GOLDEN, "trace_density.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(keys), os.path.getsize(path)))


if __name__ == "__main__":
    main()
