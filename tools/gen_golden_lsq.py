"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/lsq.npz by running the REFERENCE's own code on seeded inputs: the linear problem that
DistributionOptimizer.lsq_solution (beat/models/problems.py:753-873) assembles for a point and scipy's solution of it.
Needs the reference tree (oracle/ref_import.py finds it) and its sweep extension built into oracle/_ref (`make -C oracle`),
so it runs where that tree is mounted; the fixture it writes is data (inputs and expected outputs, none of the reference's
text).

    python tools/gen_golden_lsq.py

Reference entry points exercised:
  beat/utility.py:1542-1558            positions2idxs (nucleation point -> patch index)
  beat/fast_sweeping/fast_sweep_ext.c  fast_sweep (rupture onset times of a subfault); + time, - station shift as
                                       beat/ffi/fault.py:614-632 and beat/models/seismic.py:1283-1296 combine them
  beat/ffi/base.py:607-709             SeismicGFLibrary.stack_all(patchidxs=[p], slips=[1.]) in numpy mode, nearest
                                       neighbour and multilinear: one column of A per call, as problems.py:822-835
  beat/ffi/base.py (GeodeticGFLibrary) _gfmatrix.T, the geodetic rows (problems.py:810)
  beat/models/corrections.py:46-87     RampCorrection.get_displacements(point=...), subtracted from the displacements
                                       (problems.py:812-820, geodetic.py:411-427)
  beat/models/laplacian.py:209-258     get_smoothing_operator_nearest_neighbor, times h_laplacian ** 2 (problems.py:845-848)
  scipy.optimize.nnls                  (problems.py:854)

Per case (prefix "<name>_"): the libraries, data, layout (names / sizes of the flat parameter vector, prior box), points Q
[C, nparams], start times st0 [C, P], station shifts per wavemap [C, T], durations [C, P], ramp displacements geo_corr
[C, Nobs], h [C]; and per chain A, d, m_ref, scipy's residual norm.  Library values are small integers / 256 (they
compress); three cases add a component shared by all patches, so that their columns correlate, and search a seeded sequence
of data draws for one with which the active set removes a variable.  The generator asserts what the tests rely on: every
entry of m_ref and of the dual A^T (d - A m_ref) on the zero set is further than 1e-6 (relative) from zero, cond_2(A_P)^2 2^-52 10^3 <= 1e-8, the
residual norm is above 1e-3 |d| (a consistent system has no objective to compare), and at least two cases make the restated active set (tests/lsq_ref.py) remove a variable.
"""
import os
import sys

import numpy as np
from scipy.optimize import nnls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402

ref_import.install()

import fast_sweep_ext  # noqa: E402  (oracle/_ref, the reference's C built in place)
import lsq_ref  # noqa: E402
from beat import utility  # noqa: E402
from beat.config import GeodeticGFLibraryConfig, RampConfig, SeismicGFLibraryConfig  # noqa: E402
from beat.ffi import base as ffibase  # noqa: E402
from beat.models import laplacian as rlap  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
VEL = (2.5, 4.0)
TIME = (0.5, 1.0)
SHIFT = (-0.5, 0.5)

# name: subfault grids (n dip, n strike, patch size), wavemaps (T, N, interpolation, station shifts), geodetic dataset
# sizes, ramp on the first dataset, h range, chains, data recipe
CASES = [
    dict(name="s2x3", grids=[(2, 3, 1.0)], wms=[(1, 1, "nearest_neighbor", False)], geo=(), h=(0.5, 0.6), C=2),
    dict(name="joint3x4", grids=[(3, 4, 1.0)], wms=[(3, 5, "nearest_neighbor", True)], geo=(20,), ramp=True, h=(0.4, 0.9),
         C=3),
    dict(name="ml5x7", grids=[(5, 7, 1.0)], wms=[(4, 16, "multilinear", True)], geo=(), h=(0.8, 1.2), C=2, common=True),
    dict(name="s1x17", grids=[(1, 17, 0.5)], wms=[(3, 24, "nearest_neighbor", False)], geo=(), h=(1.5, 2.0), C=2, common=True),
    dict(name="two_sub", grids=[(2, 3, 1.0), (3, 2, 1.0)], wms=[(3, 5, "nearest_neighbor", True), (1, 16, "multilinear", False)],
         geo=(), h=(0.6, 0.8), C=2),
    dict(name="geo40", grids=[(3, 4, 1.0)], wms=[], geo=(20, 20), ramp=True, h=(0.2, 0.4), C=3, common=True),
    dict(name="zero", grids=[(2, 3, 1.0)], wms=[], geo=(20,), h=(0.1, 0.1), C=1, recipe="zero"),
    dict(name="positive", grids=[(2, 3, 1.0)], wms=[], geo=(20,), h=(0.1, 0.1), C=1, recipe="positive"),
]


def ints64(rng, shape, scale=1.0):
    return rng.integers(-127, 128, shape).astype(np.float64) / 64.0 * scale


def start_times(grids, velocities, nuc_dip, nuc_strike, time):
    """fault.py:614-632 per subfault, concatenated in patch order"""
    out, o = [], 0
    for s, (nd, ns, psz) in enumerate(grids):
        n = nd * ns
        hd = int(utility.positions2idxs(nuc_dip[s], psz))
        hs = int(utility.positions2idxs(nuc_strike[s], psz))
        slow = np.ascontiguousarray(1.0 / velocities[o:o + n])
        out.append(fast_sweep_ext.fast_sweep(slow, psz, hd, hs, nd, ns) + time[s])
        o += n
    return np.concatenate(out)


def seismic_columns(G, grid, st, dur, interp):
    """problems.py:822-835: one whole-library stacking call per patch"""
    T, P, D, S, N = G.shape
    cfg = SeismicGFLibraryConfig(dimensions=(T, P, D, S, N), starttime_sampling=grid[1], duration_sampling=grid[3],
                                 starttime_min=grid[0], duration_min=grid[2])
    gfs = ffibase.SeismicGFLibrary(config=cfg)
    gfs.setup(T, P, D, S, N, allocate=True)
    gfs._gfmatrix[:] = G
    gfs._stack_switch = {"numpy": gfs._gfmatrix}
    tidx = np.atleast_2d(np.arange(T)).T
    cols = []
    for p in range(P):
        syn = gfs.stack_all(durations=dur[[p]], starttimes=st[:, [p]], slips=np.array([1.0]), targetidxs=tidx,
                            patchidxs=np.array([p], dtype="int"), interpolation=interp)
        cols.append(np.asarray(syn).reshape(T * N))
    return np.stack(cols, axis=1)


def smoothing_operator(grids):
    """block diagonal of the subfaults' nearest-neighbour operators"""
    P = sum(nd * ns for nd, ns, _ in grids)
    L, o = np.zeros((P, P)), 0
    for nd, ns, psz in grids:
        n = nd * ns
        L[o:o + n, o:o + n] = rlap.get_smoothing_operator_nearest_neighbor(ns, nd, psz, psz)
        o += n
    return L


def gen_case(spec, rng, out):
    name, grids, C = spec["name"], spec["grids"], spec["C"]
    nsub = len(grids)
    P = sum(nd * ns for nd, ns, _ in grids)
    seismic = len(spec["wms"]) > 0
    geo = tuple(spec["geo"])
    D, du_min, du_dt, st_min, st_dt = 3, 0.5, 0.5, 0.0, 0.5
    reach = max((nd + ns) * psz for nd, ns, psz in grids) / VEL[0] + TIME[1] + SHIFT[1]
    S = int(np.ceil(reach / st_dt)) + 2
    grid = np.array([st_min, st_dt, du_min, du_dt])

    names, sizes, lower, upper = [], [], [], []

    def add(n, size, lo, up):
        names.append(n)
        sizes.append(size)
        lower.append(np.broadcast_to(np.asarray(lo, dtype=np.float64), (size,)))
        upper.append(np.broadcast_to(np.asarray(up, dtype=np.float64), (size,)))

    add("uparr", P, 0.0, 5.0)
    add("uperp", P, -1.0, 1.0)
    nshift = 0
    if seismic:
        add("durations", P, du_min, du_min + (D - 1) * du_dt)
        add("velocities", P, VEL[0], VEL[1])
        add("nucleation_strike", nsub, 0.0, [ns * psz - 0.51 * psz for nd, ns, psz in grids])
        add("nucleation_dip", nsub, 0.0, [nd * psz - 0.51 * psz for nd, ns, psz in grids])
        add("time", nsub, TIME[0], TIME[1])
        if any(w[3] for w in spec["wms"]):
            nshift = 2
            add("time_shifts", nshift, SHIFT[0], SHIFT[1])
        add("h_seis", 1, -1.0, 1.0)
    ramp_names = ["scene_0_%s" % s for s in ("azimuth_ramp", "range_ramp", "offset")]
    if geo:
        if spec.get("ramp"):
            add(ramp_names[0], 1, -0.01, 0.01)
            add(ramp_names[1], 1, -0.01, 0.01)
            add(ramp_names[2], 1, -0.05, 0.05)
        add("h_geo", 1, -1.0, 1.0)
    add("h_laplacian", 1, spec["h"][0], spec["h"][1])
    lower, upper = np.concatenate(lower), np.concatenate(upper)
    offs = dict(zip(names, np.concatenate([[0], np.cumsum(sizes)[:-1]])))
    Q = lower + (upper - lower) * rng.random((C, lower.size))

    def var(c, n):
        return Q[c, offs[n]:offs[n] + sizes[names.index(n)]]

    L = smoothing_operator(grids)
    pre = name + "_"
    out.update({pre + "P": np.array(P), pre + "grids": np.array(grids, dtype=np.float64), pre + "nwm": np.array(len(spec["wms"])),
                pre + "names": np.array(names), pre + "sizes": np.array(sizes), pre + "lower": lower, pre + "upper": upper,
                pre + "Q": Q, pre + "L": L, pre + "has_geo": np.array(int(bool(geo))), pre + "geo_sizes": np.array(geo, dtype=np.int64),
                pre + "has_ramp": np.array(int(bool(spec.get("ramp")))), pre + "h": Q[:, offs["h_laplacian"]].copy()})

    wms = []
    for w, (T, N, interp, shifts) in enumerate(spec["wms"]):
        G = ints64(rng, (T, P, D, S, N))
        if spec.get("common"):
            # a component shared by all patches: correlated columns, so that variables enter and leave the passive set
            G = ints64(rng, (T, 1, D, S, N)) + 0.25 * G
        sidx = (np.arange(T) % nshift) if shifts else np.zeros(T, dtype=np.int64)
        data = 3.0 * ints64(rng, (T, N))
        wms.append((G, interp, sidx, shifts, data))
        out.update({pre + "wm%d_G" % w: G, pre + "wm%d_grid" % w: grid, pre + "wm%d_ml" % w: np.array(int(interp == "multilinear")),
                    pre + "wm%d_data" % w: data, pre + "wm%d_sidx" % w: sidx, pre + "wm%d_has_shift" % w: np.array(int(shifts))})
    if geo:
        nobs = sum(geo)
        gcfg = GeodeticGFLibraryConfig(dimensions=(P, nobs))
        ggf = ffibase.GeodeticGFLibrary(config=gcfg)
        ggf.setup(P, nobs, allocate=True)
        ggf._gfmatrix[:] = ints64(rng, (P, nobs), 0.25)
        if spec.get("common"):
            ggf._gfmatrix[:] = ints64(rng, (1, nobs), 0.25) + 0.25 * ggf._gfmatrix
        Ggeo = ggf._gfmatrix
        east, north = rng.uniform(-30.0, 30.0, geo[0]), rng.uniform(-30.0, 30.0, geo[0])
        recipe = spec.get("recipe")
        if recipe == "zero":
            # A^T d = -1 on every component: the solution is zero throughout
            gdata = -Ggeo.T @ np.linalg.solve(Ggeo @ Ggeo.T, np.ones(P))
        elif recipe == "positive":
            gdata = Ggeo.T @ rng.uniform(1.0, 2.0, P)
        else:
            gdata = Ggeo.T @ np.where(rng.random(P) < 0.5, rng.uniform(0.5, 3.0, P), -rng.uniform(0.5, 3.0, P)) \
                + 0.05 * rng.standard_normal(nobs)
        out.update({pre + "geo_G": np.array(Ggeo), pre + "geo_data": gdata, pre + "geo_odw": 0.5 + rng.random(nobs),
                    pre + "geo_east": east, pre + "geo_north": north})
        corr = None
        if spec.get("ramp"):
            corr = RampConfig(dataset_names=["scene_0"], enabled=True).init_correction()
            corr.setup_correction(locy=north, locx=east, los_vector=None, data_mask=None, dataset_name="scene_0")
            assert list(corr.correction_names) == ramp_names

    # phase 1: everything that does not depend on the data
    st0 = np.zeros((C, P))
    dur = np.zeros((C, P))
    shift = [np.zeros((C, wm[0].shape[0])) for wm in wms]
    gcorr = np.zeros((C, sum(geo))) if geo else None
    seis_rows = []
    for c in range(C):
        seis_rows.append([])
        if seismic:
            st0[c] = start_times(grids, var(c, "velocities"), var(c, "nucleation_dip"), var(c, "nucleation_strike"), var(c, "time"))
            dur[c] = var(c, "durations")
            for w, (G, interp, sidx, shifts, data) in enumerate(wms):
                if shifts:
                    shift[w][c] = var(c, "time_shifts")[sidx]
                # seismic.py:1283-1296: tile(starttimes0, T) - repeat(time_shifts[station_idx], P)
                st = st0[c][None, :] - shift[w][c][:, None]
                seis_rows[c].append(seismic_columns(G, grid, st, dur[c], interp))
        if geo and corr is not None:
            point = dict((n, float(var(c, n)[0])) for n in ramp_names)
            gcorr[c, :geo[0]] = corr.get_displacements({}, point=point)

    def solve(datas, gdata):
        """phase 2: A, d, scipy's solution and the asserted conditions for every chain"""
        As, ds, ms, rn, removed, log = [], [], [], [], 0, []
        for c in range(C):
            rows, rhs = list(seis_rows[c]), [dd.ravel() for dd in datas]
            if geo:
                rows.append(Ggeo.T)
                rhs.append(gdata - gcorr[c])        # apply_corrections(displacements, point=point, operation="-")
            h = float(Q[c, offs["h_laplacian"]])
            rows.append(L * h ** 2.0)
            rhs.append(np.zeros(P))
            A, d = np.vstack(rows), np.hstack(rhs)
            m, res = nnls(A, d)
            dual = A.T @ (d - A @ m)
            zero = m == 0
            if (~zero).any():
                assert np.abs(m[~zero]).min() > 1e-6 * np.abs(m).max(), (name, c, "primal entry near zero")
            if zero.any():
                assert np.abs(dual[zero]).min() > 1e-6 * np.abs(A.T @ d).max(), (name, c, "dual entry near zero")
            # (an objective that is zero to rounding could not be compared with scipy's to 1e-12)
            assert res > 1e-3 * np.linalg.norm(d), (name, c, "the system is consistent")
            cond = lsq_ref.passive_cond(A, m)
            assert cond ** 2 * lsq_ref.EPS * 1e3 <= 1e-8, (name, c, "cond", cond)
            xr, it, status, rem = lsq_ref.nnls_normal(A.T @ A, A.T @ d)
            assert status == 0 and np.array_equal(xr != 0, m != 0), (name, c, "restatement support")
            removed += rem
            As.append(A); ds.append(d); ms.append(m); rn.append(res)
            log.append("%-10s chain %d: rows %d, P %d, support %d, cond %.1f, iters %d, removed %d, rnorm %.4g"
                       % (name, c, A.shape[0], P, int((m != 0).sum()), cond, it, rem, res))
        return As, ds, ms, rn, removed, log

    datas = [wm[4] for wm in wms]
    if spec.get("common"):
        # data that make the active set remove a variable: slip of mixed sign through chain 0's rows plus noise, the first
        # of a seeded sequence of draws with which the restated active set removes one (and every assert above holds)
        for attempt in range(400):
            mt = np.where(rng.random(P) < 0.6, rng.uniform(0.5, 3.0, P), -rng.uniform(0.5, 3.0, P))
            datas = [(rows0 @ mt).reshape(wm[4].shape) + 0.05 * rng.standard_normal(wm[4].shape)
                     for rows0, wm in zip(seis_rows[0], wms)]
            if geo:
                gdata = Ggeo.T @ mt + 0.05 * rng.standard_normal(sum(geo))
            try:
                res = solve(datas, gdata if geo else None)
            except AssertionError:
                continue
            if res[4] > 0:
                break
        else:
            raise AssertionError("%s: no draw of the data makes the active set remove a variable" % name)
        for w, dd in enumerate(datas):
            out[pre + "wm%d_data" % w] = dd
        if geo:
            out[pre + "geo_data"] = gdata
    else:
        res = solve(datas, gdata if geo else None)
    As, ds, ms, rn, removed, log = res
    print("\n".join(log))
    if spec.get("recipe") == "zero":
        assert not np.any(ms[0])
    if spec.get("recipe") == "positive":
        assert np.all(ms[0] > 0)
    out.update({pre + "st0": st0, pre + "durations": dur, pre + "A": np.stack(As), pre + "d": np.stack(ds),
                pre + "m_ref": np.stack(ms), pre + "rnorm": np.array(rn)})
    for w in range(len(wms)):
        out[pre + "wm%d_shift" % w] = shift[w]
    if geo:
        out[pre + "geo_corr"] = gcorr
    return removed > 0


def main():
    rng = np.random.default_rng(20261019)
    out = {"note": np.array(
        "A, d = the rows DistributionOptimizer.lsq_solution stacks for a point (seismic per wavemap / target / sample from "
        "the reference's SeismicGFLibrary.stack_all(patchidxs=[p], slips=[1.]) in numpy mode, geodetic G.T and displacements "
        "minus RampCorrection.get_displacements, laplacian L * h ** 2 and zeros); m_ref, rnorm = scipy.optimize.nnls(A, d); "
        "st0 = the reference's fast_sweep of the point's velocities and nucleation point + time."),
        "cases": np.array([c["name"] for c in CASES])}
    with_removal = 0
    for spec in CASES:
        for attempt in range(20):      # the first draw of the case's points and data that meets the asserted conditions
            part = {}
            try:
                with_removal += bool(gen_case(spec, rng, part))
            except AssertionError as exc:
                print("%s: draw %d refused (%s)" % (spec["name"], attempt, exc))
                continue
            out.update(part)
            break
        else:
            raise AssertionError("%s: no draw meets the conditions" % spec["name"])
    assert with_removal >= 2, "only %d case(s) exercise the removal loop" % with_removal
    path = os.path.join(GOLDEN, "lsq.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f kB); %d cases remove a variable" % (path, os.path.getsize(path) / 1e3, with_removal))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
