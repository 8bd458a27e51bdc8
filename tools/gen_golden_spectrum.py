"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/spectrum.npz by running the REFERENCE's own code on seeded inputs: the amplitude spectra of the
spectrum domain of a seismic wavemap (WaveformFitConfig.domain = "spectrum") as the reference's geometry mode computes
them, applied to traces and to the synthetics its FFI library stacks.  Needs the reference tree (oracle/ref_import.py finds
it) and its sweep extension built into oracle/_ref (`make -C oracle`), so it runs where that tree is mounted; the fixture it
writes is data (inputs and expected outputs, none of the reference's text).

    python tools/gen_golden_spectrum.py

Reference entry points exercised:
  beat/utility.py:1604-1610            get_valid_spectrum_data(deltaf, taper_frequencies)
  beat/heart.py:4091-4155              fft_transforms(signals, (lo, hi), outmode="array", pad_to_pow2=True)
  beat/utility.py:1542-1558, beat/fast_sweeping/fast_sweep_ext.c, beat/ffi/fault.py:614-632
                                       rupture onset times of a point, + time, - station shift (seismic.py:1283-1296)
  beat/ffi/base.py:607-709             SeismicGFLibrary.stack_all in numpy mode, nearest neighbour and multilinear, one call
                                       per slip variable, summed (seismic.py:1317-1330)

ONE LINE IS RESTATED FROM MEMORY: the import harness's stub of pyrocko.trace has no nextpow2 (pyrocko is not installed), so
this generator assigns   heart.trace.nextpow2 = lambda n: 2 ** int(ceil(log2(n)))   before it calls fft_transforms.  With it
the reference's call returns bit for bit numpy.abs(numpy.fft.rfft(y, ntrans, axis=1))[:, lo:hi] (asserted below).
multivariate_normal_chol (beat/models/distributions.py:108-140) is a pytensor graph and cannot run here: logpt comes from its
numpy restatement tests/spectrum_ref.py, applied to the reference's spectra.

"k<i>_" cases (the transform alone): traces, deltat, band, lohi, ntrans, spectra.
"<name>_" model cases: the libraries of the two slip variables, data, layout (names / sizes / prior box), points Q [C, nparams],
start times st0 [C, P], station shifts [C, T], durations [C, P], and per interpolation ("nn", "ml") the stacked synthetics
syn [C, T, N] and their spectra spec [C, T, M]; data_spec [T, M]; the weights w_scalar [T], w_bidiag, w_dense [T, M, M], slog
[T]; logpt_<interp>_<weights>_hp<0|1> [C, T] (hp1: one hyper-parameter per dataset, hp0: the first one shared).  Library values
are small integers / 64 (they compress).
"""
import os
import sys
from math import ceil, log2

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402

ref_import.install()

import fast_sweep_ext  # noqa: E402  (oracle/_ref, the reference's C built in place)
import spectrum_ref  # noqa: E402
from beat import heart, utility  # noqa: E402
from beat.config import SeismicGFLibraryConfig  # noqa: E402
from beat.ffi import base as ffibase  # noqa: E402

heart.trace.nextpow2 = lambda n: 2 ** int(ceil(log2(n)))   # restated from memory (see the docstring)

GOLDEN = os.path.join(ROOT, "tests", "golden")
VEL = (2.5, 4.0)
TIME = (0.5, 1.0)
SHIFT = (-0.5, 0.5)

# the transform alone: (N, rows, deltat, band); bands that land exactly on bins and between bins
KERNEL_CASES = [
    (10, 3, 0.5, (0.125, 0.75)),      # ntrans 16, deltaf 1/8: on bins -> [1, 6)
    (10, 3, 0.5, (0.2, 0.7)),         # between bins -> [1, 6)
    (8, 2, 1.0, (0.0, 0.55)),         # N == ntrans, DC up to and including the Nyquist bin -> [0, 5)
    (120, 3, 0.25, (0.0625, 1.0)),    # ntrans 128, deltaf 1/32: on bins -> [2, 32)
    (120, 3, 0.25, (0.05, 0.99)),     # between bins -> [1, 32)
    (127, 2, 0.25, (0.0, 2.01)),      # every bin, Nyquist included -> [0, 65)
    (129, 2, 0.25, (0.3, 0.9)),       # ntrans 256
    (2, 2, 1.0, (0.0, 0.6)),          # ntrans 2: DC and Nyquist alone -> [0, 2)
    (3, 2, 1.0, (0.25, 0.5)),         # ntrans 4
]
# name, grid (n dip, n strike, patch size), T, N, station shifts, deltat, band
MODEL_CASES = [
    dict(name="t3", grid=(2, 3, 1.0), T=3, N=10, shifts=False, deltat=0.5, band=(0.125, 0.75), C=3),
    dict(name="t2s", grid=(2, 3, 1.0), T=2, N=120, shifts=True, deltat=0.25, band=(0.0625, 1.25), C=3),
]


def ints64(rng, shape, scale=1.0):
    return rng.integers(-127, 128, shape).astype(np.float64) / 64.0 * scale


def ref_spectra(traces, deltat, band):
    """the reference's functions, and what the issue says they return"""
    n = traces.shape[1]
    ntrans = heart.trace.nextpow2(n)
    deltaf = 1.0 / (ntrans * deltat)            # heart.py:3122-3124
    lo, hi = utility.get_valid_spectrum_data(deltaf, list(band))
    assert 0 <= lo < hi <= ntrans // 2 + 1, (n, band, lo, hi)
    s = heart.fft_transforms(traces, (lo, hi), outmode="array", pad_to_pow2=True)
    assert np.array_equal(s, np.abs(np.fft.rfft(traces, ntrans, axis=1))[:, lo:hi])
    return ntrans, (lo, hi), np.asarray(s, dtype=np.float64)


def start_times(grid, velocities, nuc_dip, nuc_strike, time):
    """fault.py:614-632 for the one subfault"""
    nd, ns, psz = grid
    hd = int(utility.positions2idxs(nuc_dip, psz))
    hs = int(utility.positions2idxs(nuc_strike, psz))
    slow = np.ascontiguousarray(1.0 / velocities)
    return fast_sweep_ext.fast_sweep(slow, psz, hd, hs, nd, ns) + time


def make_library(G, grid):
    T, P, D, S, N = G.shape
    cfg = SeismicGFLibraryConfig(dimensions=(T, P, D, S, N), starttime_sampling=grid[1], duration_sampling=grid[3],
                                 starttime_min=grid[0], duration_min=grid[2])
    gfs = ffibase.SeismicGFLibrary(config=cfg)
    gfs.setup(T, P, D, S, N, allocate=True)
    gfs._gfmatrix[:] = G
    gfs._stack_switch = {"numpy": gfs._gfmatrix}
    return gfs


def exponential_bidiagonal(M, dt, tzero, scale):
    """chol(inv(C)).T of C_ij = scale exp(-|i - j| dt / tzero) (covariance.py:24-51): bidiagonal up to rounding residue,
    which is cut so that every consumer sees the same operator"""
    i = np.arange(M)
    C = scale * np.exp(-np.abs(i[:, None] - i[None, :]) * (dt / tzero))
    W = np.linalg.cholesky(np.linalg.inv(C)).T
    assert np.abs(np.triu(W, 2)).max() < 1e-12 * np.abs(W).max()
    return np.triu(np.tril(W, 1))


def gen_model(spec, rng, out):
    name, grid, T, N, C = spec["name"], spec["grid"], spec["T"], spec["N"], spec["C"]
    nd, ns, psz = grid
    P = nd * ns
    D, du_min, du_dt, st_min, st_dt = 3, 0.5, 0.5, 0.0, 0.5
    reach = (nd + ns) * psz / VEL[0] + TIME[1] + SHIFT[1]
    S = int(np.ceil(reach / st_dt)) + 2
    lgrid = np.array([st_min, st_dt, du_min, du_dt])
    nshift = 2 if spec["shifts"] else 0

    names, sizes, lower, upper = [], [], [], []

    def add(n, size, lo, up):
        names.append(n)
        sizes.append(size)
        lower.append(np.broadcast_to(np.asarray(lo, dtype=np.float64), (size,)))
        upper.append(np.broadcast_to(np.asarray(up, dtype=np.float64), (size,)))

    add("uparr", P, 0.0, 5.0)
    add("uperp", P, -1.0, 1.0)
    add("durations", P, du_min + 0.01, du_min + (D - 1) * du_dt)
    add("velocities", P, VEL[0], VEL[1])
    add("nucleation_strike", 1, 0.0, ns * psz - 0.51 * psz)
    add("nucleation_dip", 1, 0.0, nd * psz - 0.51 * psz)
    add("time", 1, TIME[0], TIME[1])
    if nshift:
        add("time_shifts", nshift, SHIFT[0], SHIFT[1])
    add("h_any_P_T", T, -1.0, 1.0)
    lower, upper = np.concatenate(lower), np.concatenate(upper)
    offs = dict(zip(names, np.concatenate([[0], np.cumsum(sizes)[:-1]])))
    Q = lower + (upper - lower) * rng.random((C, lower.size))

    def var(c, n):
        return Q[c, offs[n]:offs[n] + sizes[names.index(n)]]

    G = {v: ints64(rng, (T, P, D, S, N)) for v in ("uparr", "uperp")}
    libs = {v: make_library(G[v], lgrid) for v in G}
    sidx = (np.arange(T) % nshift) if nshift else np.zeros(T, dtype=np.int64)
    tidx = np.atleast_2d(np.arange(T)).T
    pidx = np.arange(P, dtype="int")

    st0, dur, shift = np.zeros((C, P)), np.zeros((C, P)), np.zeros((C, T))
    syn = {"nn": np.zeros((C, T, N)), "ml": np.zeros((C, T, N))}
    for c in range(C):
        st0[c] = start_times(grid, var(c, "velocities"), var(c, "nucleation_dip")[0], var(c, "nucleation_strike")[0],
                             var(c, "time")[0])
        dur[c] = var(c, "durations")
        if nshift:
            shift[c] = var(c, "time_shifts")[sidx]
        st = st0[c][None, :] - shift[c][:, None]          # seismic.py:1283-1296
        for key, interp in (("nn", "nearest_neighbor"), ("ml", "multilinear")):
            s = np.zeros((T, N))
            for v in ("uparr", "uperp"):                   # seismic.py:1317-1330
                s += np.asarray(libs[v].stack_all(durations=dur[c], starttimes=st, slips=var(c, v), targetidxs=tidx,
                                                  patchidxs=pidx, interpolation=interp)).reshape(T, N)
            syn[key][c] = s

    # observed traces: chain 0's nearest-neighbour synthetics, disturbed -- spectra of the size of the synthetics'
    data = syn["nn"][0] + 0.5 * ints64(rng, (T, N))
    ntrans, (lo, hi), data_spec = ref_spectra(data, spec["deltat"], spec["band"])
    M = hi - lo
    w_scalar = 0.5 + rng.random(T)
    w_bidiag = np.stack([exponential_bidiagonal(M, 1.0, 2.0 + t, 0.5 + 0.25 * t) for t in range(T)])
    w_dense = np.stack([np.triu(ints64(rng, (M, M), 0.25)) + np.diag(1.0 + rng.random(M)) for _ in range(T)])
    slog = rng.uniform(-3.0, 3.0, T)
    pre = name + "_"
    out.update({pre + "grid": np.array(grid, dtype=np.float64), pre + "names": np.array(names), pre + "sizes": np.array(sizes),
                pre + "lower": lower, pre + "upper": upper, pre + "Q": Q, pre + "G_uparr": G["uparr"], pre + "G_uperp": G["uperp"],
                pre + "lgrid": lgrid, pre + "data": data, pre + "sidx": sidx, pre + "has_shift": np.array(int(bool(nshift))),
                pre + "deltat": np.array(spec["deltat"]), pre + "band": np.array(spec["band"]), pre + "lohi": np.array([lo, hi]),
                pre + "ntrans": np.array(ntrans), pre + "st0": st0, pre + "shift": shift, pre + "durations": dur,
                pre + "data_spec": data_spec, pre + "w_scalar": w_scalar, pre + "w_bidiag": w_bidiag, pre + "w_dense": w_dense,
                pre + "slog": slog})
    for key in ("nn", "ml"):
        sp = np.stack([ref_spectra(syn[key][c], spec["deltat"], spec["band"])[2] for c in range(C)])
        out[pre + "syn_" + key] = syn[key]
        out[pre + "spec_" + key] = sp
        for wname, w in (("scalar", w_scalar), ("bidiag", w_bidiag), ("dense", w_dense)):
            for hps in (0, 1):
                lp = np.zeros((C, T))
                for c in range(C):
                    h = var(c, "h_any_P_T")
                    hp = h if hps else np.full(T, h[0])
                    lp[c] = spectrum_ref.logpt(w, slog, hp, data_spec - sp[c])
                out[pre + "logpt_%s_%s_hp%d" % (key, wname, hps)] = lp
    print("%-4s T %d P %d N %d ntrans %d band [%d, %d) M %d S %d" % (name, T, P, N, ntrans, lo, hi, M, S))


def main():
    rng = np.random.default_rng(20261020)
    out = {"note": np.array(
        "spectra = the reference's heart.fft_transforms(traces, get_valid_spectrum_data(1 / (ntrans deltat), band), outmode='array') "
        "with pyrocko.trace.nextpow2 restated as 2 ** ceil(log2 n); syn = the reference's SeismicGFLibrary.stack_all (numpy mode) "
        "summed over the slip variables at the reference's fast_sweep start times; logpt = the numpy restatement of "
        "multivariate_normal_chol (tests/spectrum_ref.py) on data_spec - spec."),
        "kernel_cases": np.array(len(KERNEL_CASES)), "model_cases": np.array([c["name"] for c in MODEL_CASES])}
    for i, (N, R, deltat, band) in enumerate(KERNEL_CASES):
        traces = rng.standard_normal((R, N)) * 10.0 ** rng.uniform(-3.0, 3.0, (R, 1))
        ntrans, (lo, hi), s = ref_spectra(traces, deltat, band)
        pre = "k%d_" % i
        out.update({pre + "traces": traces, pre + "deltat": np.array(deltat), pre + "band": np.array(band),
                    pre + "lohi": np.array([lo, hi]), pre + "ntrans": np.array(ntrans), pre + "spectra": s})
        print("k%d N %d ntrans %d band %s -> [%d, %d)" % (i, N, ntrans, band, lo, hi))
    for spec in MODEL_CASES:
        gen_model(spec, rng, out)
    path = os.path.join(GOLDEN, "spectrum.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f kB)" % (path, os.path.getsize(path) / 1e3))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
