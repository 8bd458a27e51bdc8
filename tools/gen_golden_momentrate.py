"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/moment_rate.npz by running the REFERENCE's own moment and moment-rate methods on seeded points.  Needs
the reference tree (oracle/ref_import.py finds it), so it runs where that tree is mounted; the fixture it writes is data
(inputs and expected outputs, none of the reference's text).

    python tools/gen_golden_momentrate.py

Reference entry points exercised (beat/ffi/fault.py):
  :445-474  FaultGeometry.get_moment_rate_function(index=[0 .. nsub - 1], point, target, store)     -> the total
  :410-443  get_subfault_moment_rate_function(index, point, target, store)                           -> every subfault
  :361-408  get_subfault_patch_stfs (through the above, and once more for every patch's times)
  :317-329  get_moment(point, store, target, datatype="seismic")
  :343-359  get_total_slip (through the above)
and beat/plotting/common.py:700-801 draw_line_on_array, looped as fuzzy_moment_rate does (beat/plotting/ffi.py:62-77;
that module itself needs matplotlib's pyplot and the whole plotting package).

pyrocko is not installed: the patches are stand-ins with what the methods above touch --
  .stf.discretize_t   pyrocko's HalfSinusoidSTF.discretize_t (exponent 1, anchor -1) AS RECALLED, with numpy's own sum
  .get_moment         k_p * slip (RectangularSource.get_moment is linear in the slip)
  .update(slip=)
-- ``point2starttimes`` returns stored onsets plus the subfault's ``time`` (the sweep is not what is tested here), the
store carries ``config.deltat``, and the magnitude is pyrocko's moment_to_magnitude as recalled, applied to the
reference's moment.  deltat is a power of two so that the reference's float slices are exact.

Every case: ndip, nstrike (nsub,), deltat, k (P,), comps (names), uparr / uperp [/ utens] / durations / onsets (C, P),
time (C, nsub); expected: M0, Mw (C,), spans (C, nsub + 1, 2), kbase, rates (C, nsub + 1, NT) zero-padded onto the common
grid, patch_k0 / patch_nt (C, P).  The case "two" also has the density grids of its total curves.
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
try:
    import fast_sweep_ext  # noqa: F401  (oracle/_ref)
except ImportError:
    # fault.py imports the compiled sweep at module level; nothing on this path calls it
    sys.modules["fast_sweep_ext"] = types.ModuleType("fast_sweep_ext")
    sys.modules["beat.fast_sweeping.fast_sweep_ext"] = sys.modules["fast_sweep_ext"]
fault_mod = importlib.import_module("beat.ffi.fault")
_pkg = types.ModuleType("beat.plotting")
_pkg.__path__ = [os.path.join(ref_import.REFERENCE_ROOT, "beat", "plotting")]
sys.modules["beat.plotting"] = _pkg
common = importlib.import_module("beat.plotting.common")

GOLDEN = os.path.join(ROOT, "tests", "golden")
DENSITY = (60, 90, 7)     # ny, nx, linewidth of the fixture's grids


class _Stf(object):
    duration = 0.0
    anchor = -1.0

    def discretize_t(self, deltat, tref):
        tmin_stf = tref - self.duration * (self.anchor + 1.0) * 0.5
        tmax_stf = tref + self.duration * (1.0 - self.anchor) * 0.5
        tmin = round(tmin_stf / deltat) * deltat
        tmax = round(tmax_stf / deltat) * deltat
        nt = int(round((tmax - tmin) / deltat)) + 1
        if nt > 1:
            t_edges = np.maximum(tmin_stf, np.minimum(tmax_stf, tmin + (np.arange(nt + 1) - 0.5) * deltat))
            fint = -np.cos((t_edges - tmin_stf) * (np.pi / self.duration))
            amplitudes = fint[1:] - fint[:-1]
            amplitudes /= np.sum(amplitudes)
        else:
            amplitudes = np.ones(1)
        return np.linspace(tmin, tmax, nt), amplitudes


class _Patch(object):
    def __init__(self, k):
        self.k, self.slip, self.stf = float(k), 0.0, _Stf()

    def update(self, slip=None):
        self.slip = slip

    def get_moment(self, target=None, store=None):
        return self.k * self.slip


class _Fault(fault_mod.FaultGeometry):
    def point2starttimes(self, point, index=0):
        return self.vector2subfault(index, point["_onsets"]) + point["time"][index]


def _fault(ndip, nstrike, k, comps):
    ordering = fault_mod.FaultOrdering(list(nstrike), list(ndip), [1.0] * len(ndip), [1.0] * len(ndip))
    fault = _Fault(["seismic"], list(comps), ordering)
    o = 0
    for s, (d, n) in enumerate(zip(ndip, nstrike)):
        fault.set_subfault_patches(s, [_Patch(v) for v in k[o:o + d * n]], "seismic", comps[0])
        o += d * n
    return fault


def _run(ndip, nstrike, deltat, k, comps, vars_, time):
    """the reference's answers for the C points of a case"""
    nsub, P = len(ndip), int(k.size)
    C = vars_["durations"].shape[0]
    fault = _fault(ndip, nstrike, k, comps)
    store = types.SimpleNamespace(config=types.SimpleNamespace(deltat=deltat))
    M0, per_draw, k0s, nts = [], [], np.zeros((C, P), np.int64), np.zeros((C, P), np.int64)
    for c in range(C):
        point = dict((v, vars_[v][c]) for v in comps)
        point.update(durations=vars_["durations"][c], time=time[c], _onsets=vars_["onsets"][c])
        M0.append(fault.get_moment(point=point, store=store, target=None, datatype="seismic"))
        curves = [fault.get_subfault_moment_rate_function(s, point, None, store) for s in range(nsub)]
        curves.append(fault.get_moment_rate_function(list(range(nsub)), point, None, store))
        per_draw.append(curves)
        o = 0
        for s in range(nsub):
            n = ndip[s] * nstrike[s]
            starts = fault.point2starttimes(point, index=s).ravel()
            pts, _ = fault.get_subfault_patch_stfs(s, fault.vector2subfault(s, point["durations"]), starts, store=store)
            for i, pt in enumerate(pts):
                k0s[c, o + i], nts[c, o + i] = int(round(pt[0] / deltat)), pt.size
            o += n
    spans = np.zeros((C, nsub + 1, 2), np.int64)
    for c in range(C):
        for r, (rates, times) in enumerate(per_draw[c]):
            assert rates.size == times.size
            first = int(round(times[0] / deltat))
            assert first * deltat == times[0] and np.all(times == (first + np.arange(times.size)) * deltat)
            spans[c, r] = first, times.size
    kbase = int(spans[:, nsub, 0].min())
    NT = int((spans[:, nsub, 0] + spans[:, nsub, 1]).max()) - kbase
    out = np.zeros((C, nsub + 1, NT))
    for c in range(C):
        for r, (rates, _) in enumerate(per_draw[c]):
            a = spans[c, r, 0] - kbase
            out[c, r, a:a + rates.size] = rates
    M0 = np.array(M0, dtype=np.float64)
    Mw = np.where(M0 == 0.0, 0.0, np.log10(np.where(M0 == 0.0, 1.0, M0) * 1.0e7) / 1.5 - 10.7)
    return dict(M0=M0, Mw=Mw, spans=spans, kbase=np.int64(kbase), rates=out, patch_k0=k0s, patch_nt=nts), per_draw


def _density(per_draw, nsub):
    """plotting/ffi.py:62-77 on the total curves"""
    ny, nx, lw = DENSITY
    rates = [d[nsub][0] for d in per_draw]
    times = [d[nsub][1] for d in per_draw]
    extent = (min(map(np.min, times)), max(map(np.max, times)), min(map(np.min, rates)), max(map(np.max, rates)))
    grid = np.zeros((ny, nx), dtype="float64")
    for mr, time in zip(rates, times):
        common.draw_line_on_array(time, mr, grid=grid, extent=extent, grid_resolution=grid.shape, linewidth=lw)
    raw = grid.copy()
    truncate = len(rates) / 2
    grid[grid > truncate] = truncate
    return dict(density_raw=raw, density=grid, density_extent=np.array(extent), density_shape=np.array(DENSITY))


def _points(rng, C, P, nsub, comps, dur=(0.3, 6.0)):
    v = dict((name, rng.uniform(-1.0, 2.0, (C, P))) for name in comps)
    v["durations"] = rng.uniform(dur[0], dur[1], (C, P))
    v["onsets"] = rng.uniform(0.0, 20.0, (C, P))
    return v, rng.uniform(-3.0, 3.0, (C, nsub))


def main():
    rng = np.random.default_rng(20261019)
    cases = {}

    def add(name, ndip, nstrike, deltat, comps, vars_, time, k, density=False):
        res, per_draw = _run(ndip, nstrike, deltat, k, comps, vars_, time)
        res.update(ndip=np.array(ndip), nstrike=np.array(nstrike), deltat=np.float64(deltat), k=k, comps=np.array(comps),
                   time=time)
        res.update(vars_)
        if density:
            res.update(_density(per_draw, len(ndip)))
        cases[name] = res

    two = ("uparr", "uperp")
    # one subfault of 3 x 2 patches
    v, t = _points(rng, 8, 6, 1, two)
    add("single", [3], [2], 0.5, two, v, t, rng.uniform(1.0e16, 5.0e17, 6))
    # two subfaults (6 + 4) with different times; utens takes part in the magnitude only
    three = ("uparr", "uperp", "utens")
    v, t = _points(rng, 24, 10, 2, three)
    v["uparr"][3, :] = 0.0                                   # a draw without slip: M0 = Mw = 0
    v["uperp"][3, :] = 0.0
    v["utens"][3, :] = 0.0
    v["uparr"][5, 2] = v["uperp"][5, 2] = 0.0                # patches without uparr / uperp (utens alone moves them)
    add("two", [3, 2], [2, 2], 0.5, three, v, t, rng.uniform(1.0e16, 5.0e17, 10), density=True)
    # half-to-even ties of k0 and k1, patches with nt == 1 (duration < deltat / 2), patches without slip
    v, t = _points(rng, 6, 6, 1, two)
    t[:] = 0.0
    v["onsets"][:, 0], v["durations"][:, 0] = 1.25, 2.0      # 2.5 -> 2, 6.5 -> 6
    v["onsets"][:, 1], v["durations"][:, 1] = 0.75, 1.5      # 1.5 -> 2, 4.5 -> 4
    v["onsets"][:, 2], v["durations"][:, 2] = 2.25, 0.5      # 4.5 -> 4, 5.5 -> 6
    v["onsets"][:, 3], v["durations"][:, 3] = 3.1, 0.1       # nt == 1
    v["onsets"][:, 4], v["durations"][:, 4] = 2.75, 0.125    # 5.5 -> 6, 5.75 -> 6: nt == 1 on a tie
    v["uparr"][:, 5] = v["uperp"][:, 5] = 0.0                # no slip
    v["uparr"][2, 0] = v["uperp"][2, 0] = 0.0
    t[4:] = 0.25                                             # the same ties moved by half a sample
    add("ties", [3], [2], 0.5, two, v, t, rng.uniform(1.0e16, 5.0e17, 6))
    # one patch with nt = 130: twice across the 64-lane loop
    v, t = _points(rng, 4, 4, 1, two)
    v["durations"][:, 1] = 129 * 0.25
    v["onsets"][:, 1] = [1.0, 1.3, 2.125, 0.05]
    add("long", [2], [2], 0.25, two, v, t, rng.uniform(1.0e16, 5.0e17, 4))
    # one subfault of 70 patches
    v, t = _points(rng, 5, 70, 1, two)
    add("wide", [7], [10], 0.5, two, v, t, rng.uniform(1.0e16, 5.0e17, 70))
    assert cases["long"]["patch_nt"][:, 1].max() == 130

    out = {"cases": np.array(sorted(cases))}
    for name, res in cases.items():
        for key, val in res.items():
            out["%s_%s" % (name, key)] = val
    path = os.path.join(GOLDEN, "moment_rate.npz")
    np.savez_compressed(path, **out)
    print("%s: %d cases, %d bytes" % (path, len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
