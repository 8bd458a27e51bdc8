"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/marginals.npz by running the REFERENCE's own marginal-plot functions on seeded inputs, and 50-digit
mpmath values of both density sums on small cases.  Needs the reference tree (oracle/ref_import.py finds it), scipy,
matplotlib and mpmath, so it runs where that tree is mounted; the fixture it writes is data (inputs and expected outputs,
none of the reference's text).

    python tools/gen_golden_marginals.py

Reference entry points exercised:
  beat/plotting/common.py:248-258    hist_binning
  beat/plotting/common.py:261-397    histplot_op, through a stub ``ax`` whose ``hist`` records the bins / density /
                                     cumulative it is given and applies numpy.histogram; get_xlim / set_xlim are inert
  beat/plotting/common.py:445-461    kde2plot_op, through a stub ``ax`` whose ``imshow`` records rot90(Z) and the extent
  beat/plotting/common.py:471-523    spherical_kde_op
  beat/models/distributions.py:245-337   vonmises_fisher, vonmises_std
  beat/utility.py:1334-1352          get_fit_indexes

Keys: "hb" (mind, maxd, nbins, bins) rows; per KDE case k "kde<k>_x", "_y", "_Z" (the reference's, on its mgrid points),
"_extent", "_Zmp" (50-digit sums on linspace points, rounded to double), "_scipy_units" (scipy's distance from _Zmp at the
same points in units of 2^-53 max Z); per histogram case "hist<k>_d", "_bins", "_edges", "_n", "_cumulative", "_quants";
per spherical case "sph<k>_lats0", "_lons0", "_lats", "_lons", "_sigma", "_kde" (the reference's), "_kdemp", "_ref_units"
(the reference's distance in units of (1 + 1/sigma^2) 2^-53 max), "_vmf" (vonmises_fisher of the first 3 samples),
"_sigmahat" (vonmises_std(lats=lats0, lons=lons0)); "fit_llk" (rows) and "fit_idx" (mean, min, max per row).
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
# beat/plotting/__init__ imports every plotting module: an empty package with the directory as its path lets
# beat.plotting.common be imported on its own
_pkg = types.ModuleType("beat.plotting")
_pkg.__path__ = [os.path.join(ref_import.REFERENCE_ROOT, "beat", "plotting")]
sys.modules["beat.plotting"] = _pkg
_pkg = types.ModuleType("beat.models")      # (the same for beat.models.distributions)
_pkg.__path__ = [os.path.join(ref_import.REFERENCE_ROOT, "beat", "models")]
sys.modules["beat.models"] = _pkg
common = importlib.import_module("beat.plotting.common")
distributions = importlib.import_module("beat.models.distributions")
utility = importlib.import_module("beat.utility")

GOLDEN = os.path.join(ROOT, "tests", "golden")
KDE_GRID = (9, 7)
SPH_GRID = (7, 6)


class _KdeAx(object):
    def imshow(self, img, extent=None, **kwargs):
        self.img, self.extent = np.array(img), np.array(extent, dtype=np.float64)


class _HistAx(object):
    def hist(self, d, bins=None, density=None, cumulative=False, **kwargs):
        self.bins, self.density, self.cumulative = bins, density, cumulative
        n, edges = np.histogram(d, bins=bins, density=density)
        if cumulative:
            n = (n * np.diff(edges)).cumsum() if density else n.cumsum()      # matplotlib's Axes.hist
        self.n, self.edges = n, edges
        return n, edges, []

    def get_xlim(self):
        return 0.0, 1.0

    def set_xlim(self, *a):
        pass

    def plot(self, *a, **k):
        pass

    def text(self, *a, **k):
        pass


def _kde_mp(x, y, gxs, gys):
    import mpmath as mp
    mp.mp.dps = 50
    n = len(x)
    X, Y = [mp.mpf(float(v)) for v in x], [mp.mpf(float(v)) for v in y]
    mx, my = mp.fsum(X) / n, mp.fsum(Y) / n
    f2 = mp.mpf(n) ** (-mp.mpf(1) / 3)
    cxx = mp.fsum([(a - mx) ** 2 for a in X]) / (n - 1) * f2
    cyy = mp.fsum([(b - my) ** 2 for b in Y]) / (n - 1) * f2
    cxy = mp.fsum([(a - mx) * (b - my) for a, b in zip(X, Y)]) / (n - 1) * f2
    det = cxx * cyy - cxy * cxy
    ixx, iyy, ixy = cyy / det, cxx / det, -cxy / det
    norm = 1 / (2 * mp.pi * n * mp.sqrt(det))
    Z = np.empty((len(gxs), len(gys)))
    for a, gx in enumerate(gxs):
        for b, gy in enumerate(gys):
            gx_, gy_ = mp.mpf(float(gx)), mp.mpf(float(gy))
            s = mp.fsum([mp.exp(-(ixx * (gx_ - p) ** 2 + 2 * ixy * (gx_ - p) * (gy_ - q) + iyy * (gy_ - q) ** 2) / 2)
                         for p, q in zip(X, Y)])
            Z[a, b] = float(s * norm)
    return Z


def _sph_mp(lats0, lons0, lats, lons, sigma):
    import mpmath as mp
    mp.mp.dps = 50

    def unit(lat, lon):
        t = (90 - mp.mpf(float(lat))) * mp.pi / 180
        p = (mp.mpf(float(lon)) % 360) * mp.pi / 180
        return mp.sin(t) * mp.cos(p), mp.sin(t) * mp.sin(p), mp.cos(t)

    s = mp.mpf(float(sigma))
    k = 1 / s ** 2
    norm = -mp.log(4 * mp.pi * s ** 2) - mp.log(mp.sinh(k))
    U0 = [unit(a, b) for a, b in zip(lats0.ravel(), lons0.ravel())]
    out = np.empty(lats.size)
    for i, (a, b) in enumerate(zip(lats.ravel(), lons.ravel())):
        g = unit(a, b)
        out[i] = float(mp.fsum([mp.exp(norm + (g[0] * u[0] + g[1] * u[1] + g[2] * u[2]) * k) for u in U0]))
    return out.reshape(lats.shape)


def main():
    from scipy import stats
    rng = np.random.default_rng(20261020)
    out = {}

    # ---- hist_binning
    rows = []
    for mind, maxd, nbins in ((0.0, 1.0, 40), (-3.7, 12.25, 40), (1.0, 1.0, 40), (1e-6, 3e-6, 40), (-1e5, 2.5e5, 40),
                              (0.0, 0.3, 7), (2.0, 2.0 + 1e-15, 40), (0.1, 0.7, 40), (0.0, 4.1, 40)):
        rows.append((mind, maxd, nbins, common.hist_binning(np.float64(mind), np.float64(maxd), nbins=nbins)))
    out["hb"] = np.array(rows, dtype=np.float64)

    # ---- kde2plot_op and the 50-digit sums
    k = 0
    scales = (1e-6, 1.0, 1e5)
    for n in (3, 65, 130, 200):
        for rho in (0.0, 0.3, 0.9, -0.999):
            sx, sy = scales[k % 3], scales[(k + 1) % 3]
            z = rng.standard_normal((2, n))
            x = sx * (3.0 + z[0])
            y = sy * (-3.0 + rho * z[0] + np.sqrt(1.0 - rho * rho) * z[1])
            ax = _KdeAx()
            common.kde2plot_op(ax, x, y, grid=KDE_GRID[0])      # (the reference's grid is square)
            gxs, gys = np.linspace(x.min(), x.max(), KDE_GRID[0]), np.linspace(y.min(), y.max(), KDE_GRID[1])
            Zmp = _kde_mp(x, y, gxs, gys)
            G = np.meshgrid(gxs, gys, indexing="ij")
            Zs = stats.gaussian_kde(np.vstack([x, y]))(np.vstack([G[0].ravel(), G[1].ravel()])).reshape(KDE_GRID)
            key = "kde%d" % k
            out[key + "_x"], out[key + "_y"] = x, y
            out[key + "_Z"], out[key + "_extent"] = np.rot90(ax.img, -1), ax.extent
            out[key + "_Zmp"] = Zmp
            out[key + "_scipy_units"] = np.float64(np.abs(Zs - Zmp).max() / (2.0 ** -53 * Zmp.max()))
            k += 1
    out["kde_n"] = np.int64(k)

    # ---- histplot_op
    k = 0
    for n, cumulative in ((1, False), (65, False), (1000, True), (4097, False), (4097, True)):
        d = np.round(rng.normal(2.0, 1.5, n), 2)
        ax = _HistAx()
        common.histplot_op(ax, d[None, :], kwargs={"cumulative": cumulative, "nsources": 1})
        key = "hist%d" % k
        out[key + "_d"], out[key + "_bins"], out[key + "_edges"], out[key + "_n"] = d, np.int64(ax.bins), ax.edges, ax.n
        out[key + "_cumulative"] = np.bool_(ax.cumulative)
        assert ax.density is True
        out[key + "_quants"] = np.percentile(d, q=[0.01, 99.99, 5, 68, 95])
        k += 1
    out["hist_n"] = np.int64(k)

    # ---- spherical_kde_op
    k = 0
    lons, lats = np.meshgrid(np.linspace(-30.0, 30.0, SPH_GRID[1]), np.linspace(-90.0, 90.0, SPH_GRID[0]))
    for n, sigma in ((1, 0.3), (65, 0.05), (130, 0.3), (501, 0.01)):
        lats0 = rng.normal(20.0, 8.0, n)
        lons0 = rng.normal(-5.0, 6.0, n)
        kde, _, _ = common.spherical_kde_op(lats0, lons0, lats=lats, lons=lons, grid_size=SPH_GRID, sigma=sigma)
        kmp = _sph_mp(lats0, lons0, lats, lons, sigma)
        key = "sph%d" % k
        out[key + "_lats0"], out[key + "_lons0"], out[key + "_sigma"] = lats0, lons0, np.float64(sigma)
        out[key + "_kde"], out[key + "_kdemp"] = kde, kmp
        out[key + "_ref_units"] = np.float64(np.abs(kde - kmp).max() / ((1.0 + 1.0 / sigma ** 2) * 2.0 ** -53 * kmp.max()))
        out[key + "_vmf"] = distributions.vonmises_fisher(lats=lats, lons=lons, lats0=lats0[:3], lons0=lons0[:3], sigma=sigma)
        out[key + "_sigmahat"] = np.float64(distributions.vonmises_std(lats=lats0, lons=lons0)) if n > 1 else np.float64(np.nan)
        k += 1
    out["sph_lats"], out["sph_lons"], out["sph_n"] = lats, lons, np.int64(k)

    # ---- get_fit_indexes
    llk = np.round(rng.normal(-100.0, 5.0, (4, 37)), 1)
    out["fit_llk"] = llk
    out["fit_idx"] = np.array([[utility.get_fit_indexes(r)[key] for key in ("mean", "min", "max")] for r in llk], dtype=np.int64)

    path = os.path.join(GOLDEN, "marginals.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))
    for i in range(int(out["kde_n"])):
        print("kde%d n=%d scipy %.1f units" % (i, out["kde%d_x" % i].size, out["kde%d_scipy_units" % i]))
    for i in range(int(out["sph_n"])):
        print("sph%d n=%d sigma=%g reference %.2f units" % (i, out["sph%d_lats0" % i].size, out["sph%d_sigma" % i],
                                                            out["sph%d_ref_units" % i]))


if __name__ == "__main__":
    main()
