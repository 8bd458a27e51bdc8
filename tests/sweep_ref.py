"""What tests/test_gpu_sweep_exact.py expects of the rupture-time sweep (csrc/sweep.hip), and the inputs it is given.

* host_sweep: fast_sweep_ext.c:120-206 restated in numpy with sqrt(x) for pow(x, 0.5) and d*d for pow(d, 2.0), the second
  writing of the expressions of oracle.fast_sweep_exact (tests/test_sweep_ref_host.py holds the two to equal bits).  It can
  also sum err in the kernel's order, with or without the kernel's fallback to the sequential sum: the CPU model of the
  kernel's stop decision, used to choose inputs and to show that the stop-rule cases catch a missing fallback.
* the case builders: grids, fields and hypocentres of the explicit mode, the four-wave workgroup batches, the stop-rule
  cases (a seeded field and a patch size, as a hex float, at which the sequential and the kernel-order err lie on
  opposite sides of 0.1) and the model-path populations with nucleation positions on and beside the rounding ties.

Nothing here is imported by the product."""
import functools
import math

import numpy as np

H = 1.3
PLAIN_MIN = 2.0 ** -767          # sweep.hip SWEEP_PLAIN: a cell passes when S2 - S*S >= 0x1p-767
ERR_STOP = 0.1                   # fast_sweep_ext.c:139 while (err > 0.1)
ERR_WINDOW = 1e-9                # sweep.hip sweep_wave: |err - 0.1| <= 1e-9 repeats the sum in the reference's order


# ------------------------------------------------------------------------------------------------- the two err orders
def sequential_err(t, told):
    """fast_sweep_ext.c:199-202: err += (t[k] - told[k])^2 over k = 0, 1, ...; t, told [C, n] -> [C]"""
    with np.errstate(all="ignore"):
        d = t - told
        return np.cumsum(d * d, axis=1)[:, -1]


def kernel_err(t, told):
    """sweep.hip sweep_wave: lane l sums its cells l, l + 64, ... in that order from 0.0, then the butterfly over xor 32,
    16, ..., 1 (wave.hpp wave_butterfly<OpAdd>: v = v + v[lane ^ off], every lane the same bits); t, told [C, n] -> [C]"""
    C, n = t.shape
    with np.errstate(all="ignore"):
        d = t - told
        sq = np.zeros((C, -(-n // 64) * 64))      # (a lane without a cell in the last round: e + 0.0 is e)
        sq[:, :n] = d * d
        e = np.zeros((C, 64))
        for r in sq.reshape(C, -1, 64).transpose(1, 0, 2):
            e = e + r
        lane = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            e = e + e[:, lane ^ off]
    assert (e == e[:, :1]).all() or np.isnan(e).any()
    return e[:, 0]


def host_sweep(slow, h, hi, hj, ni, nj, err_order="sequential", fallback=True, max_iter=None):
    """fast_sweep_ext.c:120-206 restated for a batch (cells in the reference's order, the chains side by side):
    -> times [C, ni*nj], outer iterations of every grid.  h: one patch size or one per chain.

    err_order "sequential": the reference's sum.  "kernel": the kernel's sum (kernel_err) and, with fallback, its repeat
    in the reference's order inside the window around 0.1 -- sweep.hip's stop rule as written; fallback=False is the
    kernel with that repeat taken out."""
    C = slow.shape[0]
    f = slow.reshape(C, ni, nj)
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (C,))
    t = np.full((C, ni, nj), np.inf)
    t[np.arange(C), hi, hj] = 0.0
    iters = np.zeros(C, dtype=int)
    running = np.ones(C, dtype=bool)
    orders = ((range(ni), range(nj)), (range(ni - 1, -1, -1), range(nj)),
              (range(ni - 1, -1, -1), range(nj - 1, -1, -1)), (range(ni), range(nj - 1, -1, -1)))
    with np.errstate(all="ignore"):
        while running.any() and (max_iter is None or iters.max() < max_iter):
            told = t.copy()
            for ri, rj in orders:
                for i in ri:
                    for j in rj:
                        a1, a2 = t[:, max(i - 1, 0), j], t[:, min(i + 1, ni - 1), j]
                        b1, b2 = t[:, i, max(j - 1, 0)], t[:, i, min(j + 1, nj - 1)]
                        a, b = np.where(a1 < a2, a1, a2), np.where(b1 < b2, b1, b2)
                        fij = f[:, i, j]
                        fh = fij * h
                        dab = a - b
                        v = np.where(np.abs(dab) >= fh, np.where(a < b, a, b) + fh,
                                     (a + b + np.sqrt(2.0 * fij * fij * h * h - dab * dab)) / 2.0)
                        t[:, i, j] = np.where(v < t[:, i, j], v, t[:, i, j])
            # a grid that has converged keeps its times: the reference would have stopped
            t[~running] = told[~running]
            tf, of = t.reshape(C, -1), told.reshape(C, -1)
            if err_order == "sequential":
                err = sequential_err(tf, of)
            else:
                err = kernel_err(tf, of)
                if fallback:
                    near = np.abs(err - ERR_STOP) <= ERR_WINDOW
                    err = np.where(near, sequential_err(tf, of), err)
            iters += running
            running &= err > ERR_STOP   # (NaN, from inf - inf of a cell that was not reached, ends the loop as in C)
    return t.reshape(C, -1), iters


def ulp_distance(a, b):
    """|a - b| in units in the last place for finite doubles of one sign pattern set; elementwise int64"""
    ia = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    ib = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 63) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2 ** 63) - ib, ib)
    return np.abs(ia - ib)


def plain_cells(slow, h):
    """SWEEP_PLAIN cell by cell, in put_terms' expression order"""
    with np.errstate(all="ignore"):
        S = slow * h
        S2 = 2.0 * slow * slow * h * h
        return S2 - S * S >= PLAIN_MIN


def overflow_cells(slow, h):
    """the exception the SWEEP_PLAIN comment names: S2 = 2*f*f*h*h overflowed, S*S = (f*h)*(f*h) did not"""
    with np.errstate(all="ignore"):
        S = slow * h
        S2 = 2.0 * slow * slow * h * h
        return np.isinf(S2) & np.isfinite(S * S)


# ---------------------------------------------------------------------------------------------------- explicit mode
# no interior; one cell short of / at the four-wave limit (512 cells) and the first one-wave grid; all 64 lanes live; the
# last grid with slowness terms in LDS (5120 cells); three LDS arrays: the first version although 64 rows; more than 64
# rows; the largest grid (LDS opted in above 64 KiB)
GRIDS = [(1, 1), (1, 7), (7, 1), (3, 5), (20, 20), (16, 32), (19, 27), (64, 64), (64, 80), (64, 81), (65, 3), (80, 80)]
LARGE = {(64, 80), (64, 81), (80, 80)}        # a handful of chains each


def hypocentres(ni, nj):
    """the four corners, an edge midpoint and the centre"""
    return [(0, 0), (0, nj - 1), (ni - 1, 0), (ni - 1, nj - 1), (0, nj // 2), (ni // 2, nj // 2)]


def fields(ni, nj, rng, h=H):
    n = ni * nj
    uniform = np.full(n, 1.0 / 3.0)
    random = rng.uniform(1.0 / 4.0, 1.0 / 2.5, n)
    holes = random.copy().reshape(ni, nj)
    if n > 4:
        holes.ravel()[rng.choice(n, 3, replace=False)] = np.inf       # isolated infinitely slow patches
    if ni >= 3:
        holes[ni // 2, :] = np.inf                                    # a row that cuts the grid
    elif nj >= 3:
        holes[:, nj // 2] = np.inf
    ii, jj = np.meshgrid(np.arange(ni), np.arange(nj), indexing="ij")
    checker = np.where((ii + jj) % 2 == 0, 0.25, 1e3).ravel()
    # f*h near 1.2e154: 2*f*f*h*h is +inf while (f*h)*(f*h) is finite, the sqrt argument of these cells is +inf; the
    # other half of the cells a decade below, where every term is finite
    window = rng.uniform(0.97, 1.03, n) * (1.2e154 / h)
    inside = rng.random(n) < 0.5
    inside[0] = True
    window = np.where(inside, window, 0.1 * window)
    # one cell that fails SWEEP_PLAIN (its S2 underflows to 0) in an otherwise plain grid
    onefail = random.copy()
    onefail[n // 2] = 1e-200
    # slow walls (not infinite: every cell is reached) on every other one of the first rows, open at alternating ends:
    # the front turns once per wall, more turns than one outer iteration's four sweeps follow (ten walls at the most:
    # the outer iterations grow with the walls, and the numpy restatement pays for every one of them)
    maze = np.full((ni, nj), 0.3)
    for r, i in enumerate(range(1, min(ni, 20), 2)):
        maze[i, :] = 1e3
        maze[i, nj - 1 if r % 2 == 0 else 0] = 0.3
    # (1e-200: 2*f*f*h*h underflows to 0, the sqrt argument is -(a-b)^2 or 0; 1e+150: arguments near 1e299)
    return [("uniform", uniform), ("random", random), ("inf", holes.ravel()), ("tiny", random * 1e-200),
            ("huge", random * 1e150), ("window", window), ("checker", checker), ("onefail", onefail),
            ("maze", maze.ravel())]


@functools.lru_cache(maxsize=None)
def explicit_case(ni, nj):
    """-> slow [C, n], hi [C], hj [C], names: every field x every hypocentre of one grid as one batch; of the three
    largest grids one hypocentre per field, in turn"""
    rng = np.random.default_rng(100 * ni + nj)
    slow, hi, hj, names = [], [], [], []
    for k, (fname, f) in enumerate(fields(ni, nj, rng)):
        hyp = hypocentres(ni, nj)
        for (a, b) in ([hyp[k % len(hyp)]] if (ni, nj) in LARGE else hyp):
            slow.append(f)
            hi.append(a)
            hj.append(b)
            names.append("%s@%d,%d" % (fname, a, b))
    return np.array(slow), np.array(hi, dtype=np.int32), np.array(hj, dtype=np.int32), names


@functools.lru_cache(maxsize=None)
def explicit_reference(ni, nj, h=H):
    """-> times [C, n], outer iterations [C], last err [C] of explicit_case(ni, nj) by oracle.fast_sweep_exact"""
    from oracle import oracle as orc
    slow, hi, hj, _ = explicit_case(ni, nj)
    out = [orc.fast_sweep_exact(slow[c], h, int(hi[c]), int(hj[c]), ni, nj, with_err=True) for c in range(len(hi))]
    times = np.array([o[0] for o in out])
    times.setflags(write=False)
    return times, np.array([o[1] for o in out]), np.array([o[2][-1] for o in out])


def pow_cases(count=1200, seed=20240607):
    """the seeded list the exact expressions are measured against the reference's pow arithmetic on:
    yields (slow, h, hi, hj, ni, nj), grids of 2..20 by 2..20 patches, velocities U(0.5, 6), patch sizes U(0.5, 3)"""
    rng = np.random.default_rng(seed)
    for _ in range(count):
        ni, nj = int(rng.integers(2, 21)), int(rng.integers(2, 21))
        slow = 1.0 / rng.uniform(0.5, 6.0, ni * nj)
        h = float(rng.uniform(0.5, 3.0))
        yield slow, h, int(rng.integers(0, ni)), int(rng.integers(0, nj)), ni, nj


# ---------------------------------------------------------------------------------------------- four-wave workgroups
WG_GRID = (20, 20)
# the order of the chains of a four-wave batch: (field, hypocentre number).  Neighbouring waves of workgroup 0: plain
# (uniform, maze) beside non-plain (tiny, inf), and grids of 2, at least 6 and 1 outer iterations
WG_ORDER = [("uniform", 5), ("tiny", 0), ("maze", 0), ("inf", 1), ("onefail", 3), ("random", 1), ("tiny", 4), ("checker", 5),
            ("maze", 3)]
WG_COUNTS = [1, 4, 5, 9]


def workgroup_case(C):
    """-> slow [C, 400], hi, hj, names: the first C chains of WG_ORDER, picked from explicit_case(20, 20)"""
    ni, nj = WG_GRID
    slow, hi, hj, names = explicit_case(ni, nj)
    hyp = hypocentres(ni, nj)
    sel = [names.index("%s@%d,%d" % ((f,) + hyp[k])) for f, k in WG_ORDER[:C]]
    return slow[sel], hi[sel], hj[sel], [names[s] for s in sel], sel


# ---------------------------------------------------------------------------------------------------- the stop rule
def stop_field(ni, nj, seed):
    """the seeded slowness field and hypocentre of a stop-rule case"""
    rng = np.random.default_rng(seed)
    slow = rng.uniform(0.2, 1.0, ni * nj)
    return slow, int(rng.integers(0, ni)), int(rng.integers(0, nj))


def stop_probe(slow, h, hi, hj, ni, nj, k):
    """-> (sequential err, kernel-order err) of outer iteration k >= 2 at patch size h, whatever the loop decided before"""
    from oracle import oracle as orc
    _, _, errs, tk = orc.fast_sweep_exact(slow, h, hi, hj, ni, nj, snap_iter=k)
    tkm = orc.fast_sweep_exact(slow, h, hi, hj, ni, nj, snap_iter=k - 1)[3]
    seq = sequential_err(tk[None], tkm[None])[0]
    assert seq == errs[k - 1]
    return float(seq), float(kernel_err(tk[None], tkm[None])[0])


def find_stop_case(ni, nj, seed, steps=400):
    """The search the committed STOP_CASES came from: times are proportional to the patch size, err to its square, so
    scale h until the err of the iteration the loop stops at lands on 0.1, then walk the neighbouring doubles of h for one
    where the two summation orders decide differently.  -> (h.hex(), iteration, direction) or None"""
    from oracle import oracle as orc
    slow, hi, hj = stop_field(ni, nj, seed)
    h = 1.0
    _, k, errs = orc.fast_sweep_exact(slow, h, hi, hj, ni, nj, with_err=True)
    if k < 2 or not errs[k - 1] > 0.0:
        return None
    for _ in range(4):
        e = stop_probe(slow, h, hi, hj, ni, nj, k)[0]
        if not (e > 0.0 and math.isfinite(e)):
            return None
        h *= math.sqrt(ERR_STOP / e)
    bits = np.array([h]).view(np.int64)[0]
    for s in sorted(range(-steps, steps + 1), key=abs):
        hh = float(np.array([bits + s], dtype=np.int64).view(np.float64)[0])
        seq, ker = stop_probe(slow, hh, hi, hj, ni, nj, k)
        if (seq > ERR_STOP) != (ker > ERR_STOP):
            errs = orc.fast_sweep_exact(slow, hh, hi, hj, ni, nj, snap_iter=k)[2]
            direction = "kernel_stops_early" if seq > ERR_STOP else "kernel_runs_on"
            c = stop_case((ni, nj, seed, hh.hex(), k, direction))
            # the iterations before are far from the decision, and the other decision changes a time
            if (errs[:k - 1] > 1.0).all() and not np.array_equal(c["wrong"], c["times"]):
                return hh.hex(), k, direction
    return None


# (ni, nj, seed, patch size, the iteration whose err straddles 0.1, what the kernel's own sum would decide there)
#   kernel_stops_early: sequential err > 0.1 >= kernel-order err: the reference sweeps on, the bare kernel sum stops
#   kernel_runs_on:     sequential err <= 0.1 < kernel-order err: the reference stops, the bare kernel sum sweeps on
STOP_CASES = [
    # 400 cells: lanes sum six or seven cells each
    (20, 20, 1, "0x1.2fcad2a0dc371p+2", 3, "kernel_stops_early"),
    (20, 20, 9, "0x1.5c9d5a85b9acdp+1", 2, "kernel_stops_early"),
    (20, 20, 13, "0x1.6792eb04c08d7p+5", 3, "kernel_runs_on"),
    (20, 20, 47, "0x1.ec6575bcd5af1p+1", 2, "kernel_runs_on"),
    # 64 cells: one cell per lane, the butterfly alone against the sequential sum
    (4, 16, 137, "0x1.182a7ea477f2bp+0", 2, "kernel_stops_early"),
    (4, 16, 166, "0x1.0baca60f26477p+1", 2, "kernel_stops_early"),
    (4, 16, 14, "0x1.b32dd5e93297dp+3", 2, "kernel_runs_on"),
    (4, 16, 25, "0x1.4feae8329a25dp+1", 2, "kernel_runs_on"),
    # 512 cells: the largest grid of the four-wave workgroup
    (16, 32, 17, "0x1.a5124215608efp+1", 3, "kernel_stops_early"),
    (16, 32, 2, "0x1.5bff026ec9f2fp+1", 3, "kernel_runs_on"),
]


def stop_case(case):
    """-> dict of a STOP_CASES entry: inputs, the reference's times and iterations, the times of the other decision"""
    from oracle import oracle as orc
    ni, nj, seed, hhex, k, direction = case
    h = float.fromhex(hhex)
    slow, hi, hj = stop_field(ni, nj, seed)
    seq, ker = stop_probe(slow, h, hi, hj, ni, nj, k)
    # the other decision: stop after iteration k where the reference goes on; go on to k + 1 where it stops
    other = k if direction == "kernel_stops_early" else k + 1
    times, iters, errs, wrong = orc.fast_sweep_exact(slow, h, hi, hj, ni, nj, snap_iter=other)
    return dict(ni=ni, nj=nj, h=h, slow=slow, hi=hi, hj=hj, k=k, direction=direction, seq=seq, ker=ker, times=times,
                iters=iters, errs=errs, wrong=wrong)


# ---------------------------------------------------------------------------------------------------- the model path
# (subfault grids, patch sizes): lean loop twice; the first version (65 rows) and the lean loop in one launch; three LDS
# arrays, which the small grid inherits
MODEL_SETS = [(((20, 20), (3, 5)), (1.0, 0.7)), (((65, 3), (20, 20)), (0.5, 1.0)), (((64, 81), (4, 4)), (0.7, 0.5))]
MODEL_CHAINS = 13


def tie_positions(n, h):
    """nucleation positions pd of a subfault axis of n patches of size h whose (pd - h/2)/h is exactly k + 0.5 in float64
    with k and k + 1 both on the axis (the tie and its two neighbouring doubles stay on the grid) -> [(pd, k)]"""
    out = []
    for k in range(0, n - 1):
        pd = (k + 1) * h
        if (pd - 0.0 - (h / 2.0)) / h == k + 0.5:
            out.append((pd, k))
    return out


def model_spec(grids, sizes):
    from beat_amd.synthetic import SyntheticSpec
    # the smallest library the spec allows (one target, one duration, two start times wide enough for any rupture): only
    # the rupture times are computed.  time > 0: the + time store.
    return SyntheticSpec(tuple(g[0] for g in grids), tuple(g[1] for g in grids), tuple(sizes), T=1, N=32, D=1, S=2,
                         st_dt=500.0, time_bounds=(0.25, 1.0))


@functools.lru_cache(maxsize=None)
def model_population(which):
    """-> spec, layout, Q [MODEL_CHAINS, nparams] of MODEL_SETS[which]: the seeded draw, then chain by chain the nucleation
    positions of every subfault set on a tie (even and odd k in turn), one double below it, one above it, or left as
    drawn; ties -> per subfault and axis the list of (chain, k, step)"""
    from beat_amd.synthetic import _layout_and_bounds, draw_population
    grids, sizes = MODEL_SETS[which]
    spec = model_spec(grids, sizes)
    layout, lower, upper = _layout_and_bounds(spec)
    Q = draw_population(spec, layout, lower, upper, MODEL_CHAINS, seed_offset=7000 + 100 * which)
    ties = {}
    for sf, ((nd, ns), h) in enumerate(zip(grids, sizes)):
        for axis, n in (("nucleation_dip", nd), ("nucleation_strike", ns)):
            tp = tie_positions(n, h)
            even, odd = [p for p in tp if p[1] % 2 == 0], [p for p in tp if p[1] % 2 == 1]
            col = layout.offset(axis, sf)
            rec = ties.setdefault((sf, axis), [])
            for c in range(MODEL_CHAINS - 1):           # the last chain stays as drawn
                pool = (even, odd)[(c // 3 + (axis == "nucleation_strike")) % 2] or even or odd
                pd, k = pool[(c * 7 + sf) % len(pool)]
                step = (0, -1, 1)[c % 3]
                Q[c, col] = pd if step == 0 else np.nextafter(pd, -np.inf if step < 0 else np.inf)
                rec.append((c, k, step))
    return spec, layout, Q, ties


def model_reference(which):
    """-> [C, P]: every subfault fast_sweep_exact(1 / velocities, h_sf, hi, hj) + time_sf with the indices of
    oracle.positions2idxs (seismic.py:1253-1272)"""
    from oracle import oracle as orc
    grids, sizes = MODEL_SETS[which]
    spec, layout, Q, _ = model_population(which)
    out = np.empty((Q.shape[0], spec.P))
    at = 0
    for sf, ((nd, ns), h) in enumerate(zip(grids, sizes)):
        n = nd * ns
        v0 = layout.offset("velocities") + at
        hi = orc.positions2idxs(Q[:, layout.offset("nucleation_dip", sf)], h)
        hj = orc.positions2idxs(Q[:, layout.offset("nucleation_strike", sf)], h)
        for c in range(Q.shape[0]):
            out[c, at:at + n] = orc.fast_sweep_exact(1.0 / Q[c, v0:v0 + n], h, int(hi[c]), int(hj[c]), nd, ns) \
                + Q[c, layout.offset("time", sf)]
        at += n
    return out
