"""
TEST INFRASTRUCTURE ONLY: numpy restatement of the spectrum domain of a seismic wavemap, pinned bit for bit to
tests/golden/spectrum.npz (written by tools/gen_golden_spectrum.py from the reference's own functions) by
tests/test_spectrum_host.py, and used as the expected side of tests/test_gpu_spectrum.py.

  nextpow2                pyrocko.trace.nextpow2, RESTATED FROM MEMORY (pyrocko is not in the tree): 2 ** ceil(log2 n)
  valid_spectrum_indices  beat/utility.py:1604-1610 get_valid_spectrum_data, with deltaf = 1 / (ntrans * deltat)
                          (beat/heart.py:3122-3124)
  spec                    beat/heart.py:4091-4155 fft_transforms(outmode="array"): abs(rfft(y, ntrans))[lo:hi]
  residual                data_spec - spec(syn)            (beat/models/seismic.py:932-941, beat/pytensorf.py:294-311)
  logpt                   beat/models/distributions.py:108-140 multivariate_normal_chol with M = hi - lo samples
"""
import numpy as np

LOG_2PI = np.log(2.0 * np.pi)
EPS53 = 2.0 ** -53


def nextpow2(n):
    return int(2 ** int(np.ceil(np.log2(n))))


def valid_spectrum_indices(nsamples, deltat, taper_frequencies):
    """-> ntrans, (lo, hi)"""
    ntrans = nextpow2(nsamples)
    deltaf = 1.0 / (ntrans * deltat)
    lower_f, upper_f = taper_frequencies
    return ntrans, (int(np.floor(lower_f / deltaf)), int(np.ceil(upper_f / deltaf)))


def spec(y, ntrans, lo, hi):
    """rows of y (n, N) -> (n, hi - lo), one transform per trace as the reference's loop"""
    y = np.atleast_2d(np.asarray(y, dtype=np.float64))
    out = np.zeros((y.shape[0], hi - lo))
    for i, tr in enumerate(y):
        out[i] = np.abs(np.fft.rfft(tr, ntrans))[lo:hi]
    return out


def residual(data_spec, syn, ntrans, lo, hi):
    """data_spec (T, M), syn (T, N) -> (T, M)"""
    return data_spec - spec(syn, ntrans, lo, hi)


def misfits(weights, res):
    """|W_t r_t|^2 per dataset: weights (T,) scalars or (T, M, M)"""
    w = np.asarray(weights, dtype=np.float64)
    out = np.zeros(res.shape[0])
    for t in range(res.shape[0]):
        tmp = w[t] * res[t] if w.ndim == 1 else w[t].dot(res[t])
        out[t] = tmp.dot(tmp)
    return out


def logpt(weights, slog_pdet, hp, res):
    """distributions.py:119-138: hp (T,) the hyper-parameter of every dataset (the shared one repeated when not
    hp_specific); res (T, M)"""
    M = res.shape[1]
    q = misfits(weights, res)
    out = np.zeros(res.shape[0])
    for t in range(res.shape[0]):
        norm = M * (2 * hp[t] + LOG_2PI)
        out[t] = (-0.5) * (slog_pdet[t] + norm + (1 / np.exp(hp[t] * 2)) * q[t])
    return out


def load_case(g, name):
    """the arrays of one case of tests/golden/spectrum.npz, without the prefix"""
    pre = name + "_"
    return dict((k[len(pre):], g[k]) for k in g.files if k.startswith(pre))


def case_weights(case, kind):
    return {"scalar": case["w_scalar"], "bidiag": case["w_bidiag"], "dense": case["w_dense"]}[kind]


def make_wavemap(case, interp="nn", weights="scalar", hp_specific=False, domain="spectrum", name="any_P_0"):
    """one wavemap over a model case of the fixture, the case's two libraries behind uparr and uperp: in the spectrum domain
    with the case's weights of a kind ("scalar", "bidiag", "dense"), in the time domain with unit scalars"""
    from beat_amd.ffi import SeismicGFLibrary, SeismicGFLibraryConfig
    from beat_amd.models import SeismicWavemap
    lgrid = case["lgrid"]
    gfs = {}
    for v in ("uparr", "uperp"):
        G = case["G_" + v]
        gf = SeismicGFLibrary(SeismicGFLibraryConfig(dimensions=G.shape, starttime_sampling=float(lgrid[1]),
                                                     duration_sampling=float(lgrid[3]), starttime_min=float(lgrid[0]),
                                                     duration_min=float(lgrid[2]), component=v, mapnumber=0))
        gf.setup(*G.shape, allocate=True)
        gf._gfmatrix[:] = G
        gfs[v] = gf
    T = case["data"].shape[0]
    ts = ("time_shifts", case["sidx"]) if int(case["has_shift"]) else None
    hypers = [("h_any_P_T", t if hp_specific else 0) for t in range(T)]
    kw, w = {}, np.ones(T)
    if domain == "spectrum":
        kw = dict(domain="spectrum", deltat=float(case["deltat"]), taper_frequencies=tuple(float(f) for f in case["band"]))
        w = case_weights(case, weights)
    return SeismicWavemap(gfs, case["data"], w, case["slog"], hypers, ts,
                          "multilinear" if interp == "ml" else "nearest_neighbor", name=name, **kw)


def build_problem(case, wavemaps, geodetic=None, laplacian=None, extra_vars=()):
    """FFIProblem over a model case of the fixture with slip variables (uparr, uperp) and the case's layout and prior box;
    extra_vars: (name, size, lower, upper) appended to the layout (their columns of Q are the caller's)"""
    from collections import OrderedDict

    from beat_amd.models import FFIProblem, ParameterLayout
    names, sizes = [str(n) for n in case["names"]], [int(s) for s in case["sizes"]]
    lower, upper, o = {}, {}, 0
    for n, s in zip(names, sizes):
        lower[n], upper[n] = case["lower"][o:o + s], case["upper"][o:o + s]
        o += s
    for n, s, lo, up in extra_vars:
        names.append(n)
        sizes.append(int(s))
        lower[n], upper[n] = np.full(int(s), float(lo)), np.full(int(s), float(up))
    lay = ParameterLayout(OrderedDict(zip(names, sizes)))
    grid = case["grid"]
    prob = FFIProblem(lay, [int(grid[0])], [int(grid[1])], [float(grid[2])], ["uparr", "uperp"], list(wavemaps), geodetic,
                      laplacian, lower, upper)
    return prob, lay


def bin_bound(y, ntrans):
    """the per-bin bound of the kernel against numpy for a trace y: 8 max(1, log2 ntrans) 2^-53 |y|_2, the classical
    O(eps log n |y|_2) error of an FFT with a constant of 8"""
    y = np.atleast_2d(y)
    return 8.0 * max(1.0, np.log2(ntrans)) * EPS53 * np.sqrt((y * y).sum(axis=1))


# ---- the cases of the kernel test (tests/test_gpu_spectrum.py test 1; tools/spectrum_timing.py records their bound ratios)
# nextpow2 of these is every power of two from 2 to 8192; N = ntrans and N = ntrans / 2 + 1 for 16, 32, 64 (one wavefront, less
# than a quad per lane), 512 (the largest one-wavefront shape), 1024 (the smallest one-workgroup shape, odd stage count), 2048
KERNEL_SIZES = (2, 3, 5, 8, 9, 16, 17, 32, 33, 64, 120, 127, 128, 129, 257, 512, 513, 1024, 1025, 2048, 4096, 4097)
KERNEL_ROWS = (1, 7, 130)
_TRACES = {}


def kernel_traces(N):
    """130 seeded rows of N samples (normal draws scaled by 10**U(-3, 3)), ntrans and their full numpy spectra, made once
    and read-only"""
    if N not in _TRACES:
        rng = np.random.default_rng(1000 + N)
        R = max(KERNEL_ROWS)
        y = rng.standard_normal((R, N)) * 10.0 ** rng.uniform(-3.0, 3.0, (R, 1))
        ntrans = nextpow2(N)
        full = np.abs(np.fft.rfft(y, ntrans, axis=1))
        full.setflags(write=False)
        y.setflags(write=False)
        _TRACES[N] = (y, ntrans, full)
    return _TRACES[N]


def kernel_bands(ntrans):
    """full, DC only, Nyquist only, one interior bin, an interior range (where the transform has them)"""
    n2 = ntrans // 2
    bands = {"full": (0, n2 + 1), "dc": (0, 1), "nyquist": (n2, n2 + 1)}
    if n2 >= 2:
        bands["interior_bin"] = (n2 // 2, n2 // 2 + 1)
    if n2 >= 4:
        bands["interior_range"] = (n2 // 4, 3 * n2 // 4 + 1)
    return bands


def kernel_bound_ratio(ctx, N):
    """largest |device - numpy| / bin_bound over the rows counts and bands of trace length N -> (ntrans, ratio, where)"""
    y, ntrans, full = kernel_traces(N)
    bound = bin_bound(y, ntrans)[:, None]
    worst, where = 0.0, None
    for R in KERNEL_ROWS:
        for name, (lo, hi) in kernel_bands(ntrans).items():
            got = ctx.amp_spectrum_batch(np.ascontiguousarray(y[:R]), ntrans, (lo, hi))
            assert got.shape == (R, hi - lo)
            ratio = float((np.abs(got - full[:R, lo:hi]) / bound[:R]).max())
            if ratio >= worst:
                worst, where = ratio, (R, name)
    return ntrans, worst, where
