"""
Times the posterior marginals on the GPU against the host route they replace, on the same box:

  population    a 4096 x 1204 FFI population, 10 selected columns (device tensor in, tensors out)
  trace         a 10^5 x 10 thinned trace
  per function  sort_columns, percentiles (8 of them, on the handle), make_bins, histograms (40 bins, on the handle), the
                three from X in one go, hist2d (45 pairs, 40 x 40), kde2d / correlation_kdes (45 pairs, 200 x 200)
  lune_kde      4096 and 10^5 MTQT draws on the 200 x 200 lune grid
  host          numpy.percentile / numpy.histogram / numpy.histogram2d per column (pair); scipy.stats.gaussian_kde on the
                200 x 200 grid for ONE pair (times 45 pairs = the figure reported, marked as such); the reference's chunked
                numpy evaluation of the von Mises-Fisher sum restated here (chunks of 500 draws; for 10^5 draws ten chunks
                are timed and scaled, marked as such)

Device times: HIP events around ``iters`` calls after a warm-up call, ``iters`` chosen so that a window lasts about half a
second; medians over ``reps`` windows.  For k_pair_kde2d and k_sph_kde the kernel's own time (``Context.kernel_time``) and
the fraction of the FP64 vector rate (256 CUs x 64 lanes x 2.4 GHz lane-instructions per second) that the count of
exponential terms implies, with the vector instructions per term counted in the ISA of the inner loops (hipcc -S):
117 per 4 terms for k_pair_kde2d, 161 per 4 for k_sph_kde (which divides by sigma^2 per term, as the reference's formula
does); the narrow shapes' loops, unrolled, come to the same per term (117 per 4, 81 per 2).

    python tools/time_marginals.py [--out profiles/marginals_timing.json] [--reps 3]
"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginals_timing.json"))
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

import torch  # noqa: E402
from scipy import stats as sstats  # noqa: E402

import beat_amd  # noqa: E402
from beat_amd import marginals as m  # noqa: E402

ctx = beat_amd.get_context(0)          # raises without a GPU: there is nothing to time on a CPU
dev = torch.device("cuda", 0)
FP64_LANE_INSTR_PER_S = 256 * 64 * 2.4e9
VALU_PER_TERM = {"pair_kde2d": 117.0 / 4.0, "sph_kde": 161.0 / 4.0}
Q8 = [0, 0.01, 5, 50, 68, 95, 99.99, 100]


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)), n=len(v))


def device_time(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    iters = int(min(max(0.5 / max(time.perf_counter() - t0, 1e-6), 1), 200))
    out = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    d = stats(out)
    d["iters"] = iters
    return d


def host_time(fn, reps=None):
    out = []
    for _ in range(reps or args.reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def kernel_time(name, fn, terms):
    ctx.enable_timing(True)
    ctx.reset_timing()
    fn()
    torch.cuda.synchronize()
    ms, n = ctx.kernel_time(name)
    ctx.enable_timing(False)
    per = ms / max(n, 1)
    return OrderedDict(kernel_ms=float(per), launches=int(n), exponential_terms=float(terms),
                       valu_per_term=VALU_PER_TERM[name],
                       fp64_vector_fraction=float(terms * VALU_PER_TERM[name] / (per * 1e-3) / FP64_LANE_INSTR_PER_S))


def scipy_pair(x, y, grid=200):
    X, Y = np.mgrid[x.min():x.max():grid * 1j, y.min():y.max():grid * 1j]
    return np.reshape(sstats.gaussian_kde(np.vstack([x, y]))(np.vstack([X.ravel(), Y.ravel()])).T, X.shape)


def columns_case(name, X, cols):
    print("== %s %s, %d columns" % (name, X.shape, len(cols)), flush=True)
    Xd = torch.from_numpy(X).to(dev)
    ctx.use_torch_stream()
    pairs = m.correlation_pairs(cols)
    D = X[:, cols]
    h = m.sort_columns(Xd, cols)
    edges = m.make_bins(h, 41, [0.01, 99.99])
    case = OrderedDict(case=name, n=int(X.shape[0]), V=int(X.shape[1]), columns=len(cols), pairs=int(pairs.shape[0]))
    case["sort_columns"] = device_time(lambda: m.sort_columns(Xd, cols))
    case["percentiles_on_handle"] = device_time(lambda: m.percentiles(h, Q8))
    case["make_bins_on_handle"] = device_time(lambda: m.make_bins(h, 41, [0.01, 99.99]))
    case["histograms_on_handle"] = device_time(lambda: m.histograms(h, edges=edges))

    def all_three():
        hh = m.sort_columns(Xd, cols)
        m.percentiles(hh, Q8)
        m.histograms(hh, edges=m.make_bins(hh, 41, [0.01, 99.99]))
    case["sort_percentiles_bins_histograms"] = device_time(all_three)

    def host_three():
        np.percentile(D, Q8, axis=0)
        for k in range(D.shape[1]):
            qu = np.percentile(D[:, k], [0.01, 99.99])
            np.histogram(D[:, k], bins=np.linspace(qu[0], qu[-1], 41), density=True)
    case["host_percentiles_bins_histograms"] = host_time(host_three)
    case["hist2d_40x40"] = device_time(lambda: m.hist2d(Xd, pairs, bins=(40, 40)))
    case["host_histogram2d_40x40"] = host_time(
        lambda: [np.histogram2d(X[:, i], X[:, j], bins=(40, 40), density=True) for i, j in pairs])
    print("   kde2d ...", flush=True)
    case["kde2d_200x200"] = device_time(lambda: m.kde2d(Xd, pairs, grid=200))
    case["k_pair_kde2d"] = kernel_time("pair_kde2d", lambda: m.kde2d(Xd, pairs, grid=200),
                                       float(pairs.shape[0]) * 200 * 200 * X.shape[0])
    print("   scipy, one pair ...", flush=True)
    i, j = pairs[0]
    one = host_time(lambda: scipy_pair(X[:, i], X[:, j]), reps=1)
    case["host_scipy_kde_one_pair"] = one
    case["host_scipy_kde_all_pairs_scaled_ms"] = one["median_ms"] * pairs.shape[0]
    Z = m.kde2d(Xd, pairs[:1], grid=200)[0][0].cpu().numpy()
    Zs = scipy_pair(X[:, i], X[:, j])
    case["kde2d_vs_scipy_rel_max"] = float(np.abs(Z - Zs).max() / Zs.max())
    print(json.dumps(case), flush=True)
    return case


def vmf_chunks(lats0, lons0, lats, lons, sigma, nchunk=None):
    """the host route of spherical_kde_op restated: chunks of 500 draws, exp of the (grid, chunk) matrix summed"""
    def unit(la, lo):
        t, p = np.deg2rad(90.0 - la), np.deg2rad(np.mod(lo, 360.0))
        return np.array([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)])
    x, norm = unit(lats, lons), m.vmf_norm(sigma)
    kde = np.zeros(lats.shape)
    done = 0
    for s in range(0, lats0.size, 500):
        x0 = unit(lats0[s:s + 500], lons0[s:s + 500])
        kde += np.exp(norm + np.tensordot(x, x0, axes=[[0], [0]]) / sigma ** 2).sum(axis=-1)
        done += 1
        if nchunk and done >= nchunk:
            break
    return kde


def lune_case(n):
    print("== lune_kde %d draws" % n, flush=True)
    from beat_amd.sources import v_to_gamma, w_to_delta
    rng = np.random.default_rng(n)
    v, w = rng.uniform(-0.3, 0.3, n), rng.uniform(-1.0, 1.0, n)
    case = OrderedDict(case="lune_kde", draws=n, grid=[200, 200])
    case["lune_kde"] = device_time(lambda: m.lune_kde(v, w))
    kde, lats, lons = m.lune_kde(v, w)
    gamma, delta = np.rad2deg(v_to_gamma(v)), np.rad2deg(w_to_delta(w))
    sigma = 1.06 * m.vonmises_std(lons=gamma, lats=delta) * n ** -0.2
    case["sigma"] = float(sigma)
    case["lune_kde_fixed_sigma"] = device_time(lambda: m.lune_kde(v, w, sigma=sigma))
    case["k_sph_kde"] = kernel_time("sph_kde", lambda: m.lune_kde(v, w, sigma=sigma), float(n) * 200 * 200)
    nchunk = None if n <= 5000 else 10
    host = host_time(lambda: vmf_chunks(delta, gamma, lats, lons, sigma, nchunk), reps=1)
    case["host_numpy_chunks"] = host
    case["host_chunks_timed"] = int(nchunk or -(-n // 500))
    case["host_numpy_all_chunks_scaled_ms"] = host["median_ms"] * (-(-n // 500)) / case["host_chunks_timed"]
    if nchunk is None:
        want = vmf_chunks(delta, gamma, lats, lons, sigma)
        case["lune_kde_vs_host_units"] = float(np.abs(kde - want).max() / ((1 + 1 / sigma ** 2) * 2.0 ** -53 * want.max()))
    print(json.dumps(case), flush=True)
    return case


out = OrderedDict(device=torch.cuda.get_device_name(0), reps=args.reps, fp64_lane_instr_per_s=FP64_LANE_INSTR_PER_S, cases=[])
rng = np.random.default_rng(0)
pop = rng.standard_normal((4096, 1204)) * rng.uniform(0.1, 10.0, 1204) + rng.uniform(-5.0, 5.0, 1204)
out["cases"].append(columns_case("population", pop, [3, 17, 150, 151, 400, 401, 777, 900, 1100, 1203]))
L = np.linalg.cholesky(0.5 * np.eye(10) + 0.5)
trace = rng.standard_normal((100000, 10)) @ L.T
out["cases"].append(columns_case("trace", trace, list(range(10))))
for n in (4096, 100000):
    out["cases"].append(lune_case(n))
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print("wrote", args.out)
