"""TEST INFRASTRUCTURE ONLY.  numpy restatement of the resolution-based discretization (reference
beat/ffi/fault.py:1520-1987 with beat/ffi/base.py:804-1002 and beat/models/laplacian.py:261-298) on dense host arrays,
independent of beat_amd's device path: Green's functions from the float64 Okada oracle (oracle/okada_oracle.py), the
resolution by the reference's expression ``inv(Gd^T Gd).dot(G^T G)``, the division penalties as numpy writes them.  Also
the fixture problem the generator (tools/gen_golden_discretization.py) and the tests share."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import okada_oracle  # noqa: E402

d2r = np.pi / 180.0
km = 1000.0
COMPONENTS = {"uparr": (0.0, None), "uperp": (-90.0, None), "utens": (0.0, 1.0)}


# ------------------------------------------------------------------------------------------ geometry
def _vectors(p):
    st, dp = p[3] * d2r, p[4] * d2r
    sv = np.array([np.sin(st), np.cos(st), 0.0])
    dv = np.array([np.cos(dp) * np.cos(st), -np.cos(dp) * np.sin(st), np.sin(dp)])
    return sv, dv


def patches(p, nl, nw):
    sv, dv = _vectors(p)
    length, width = p[6] / float(nl), p[7] / float(nw)
    cen = np.array([p[0], p[1], p[2]]) + 0.5 * p[7] * dv
    top = cen - 0.5 * p[7] * dv
    out = []
    for j in range(nw):
        for i in range(nl):
            q = np.array(p, dtype=np.float64)
            q[:3] = top + sv * ((i + 0.5 - 0.5 * nl) * length) + dv * (j * width)
            q[6], q[7] = length, width
            out.append(q)
    return np.array(out)


def centers(params):
    return np.array([np.array([p[0], p[1], p[2]]) + 0.5 * p[7] * _vectors(p)[1] for p in params])


def n_patches(extent, size):
    return int(np.ceil(np.round(extent / size, decimals=4)))


def component_rows(params, comp):
    out = np.array(params, dtype=np.float64, copy=True)
    out[:, 5] += COMPONENTS[comp][0]
    out[:, 8] = 1.0
    if COMPONENTS[comp][1] is not None:
        out[:, 9] = COMPONENTS[comp][1]
    return out


def disp_neu(row, east, north, nu):
    """(nobs, 3) = [north, east, up] of one source row"""
    ue, un, uz = okada_oracle.rect_source(east, north, *row, nu=nu)
    return np.stack([un, ue, uz], axis=1)


def library(rows, east, north, los, odw, nu):
    """base.py:813 per row -> (nrows, nobs)"""
    return np.array([(disp_neu(r, east, north, nu) * los).sum(axis=1) * odw for r in rows])


# ------------------------------------------------------------------------------------------ operators
def distances(points, ref_points):
    d = points[:, None, :] - ref_points[None, :, :]
    s = d[..., 0] ** 2
    for k in range(1, d.shape[2]):
        s = s + d[..., k] ** 2
    return np.sqrt(s)


def smoothing_correlated(coords, kind="gaussian"):
    """rows added in ascending order: the documented order of the device and host operator"""
    d = distances(coords, coords)
    np.fill_diagonal(d, 1.0)
    a = 1.0 / (d * d) if kind == "gaussian" else 1.0 / np.exp(d)
    np.fill_diagonal(a, 0.0)
    s = np.zeros(a.shape[0])
    for i in range(a.shape[0]):
        s = s + a[i]
    np.fill_diagonal(a, -s)
    return a


def resolution(G, L, epsilon):
    """fault.py:1805-1815 as written: G (nobs, P)"""
    smoothing_op = L * epsilon ** 2
    GG = G.T.dot(G)
    Gdamped = np.vstack((G, smoothing_op))
    return np.linalg.inv(Gdamped.T.dot(Gdamped)).dot(GG)


def resolution_cholesky(G, L, epsilon):
    """the same matrix by an algebraically equal float64 route: a Cholesky solve of the normal equations"""
    smoothing_op = L * epsilon ** 2
    GG = G.T.dot(G)
    N = GG + smoothing_op.T.dot(smoothing_op)
    c = np.linalg.cholesky(N)
    y = np.linalg.solve(c, GG)
    return np.linalg.solve(c.T, y)


def rating(widths, lengths, cen, bottom_depth_m, depth_penalty, data_coords, mean_R):
    """fault.py:1893-1929 -> (rating, patch_data_distance_mins); c3's two sums in ascending index order"""
    area_pen = widths * lengths
    c1 = np.exp(-depth_penalty * cen[:, 2] * km / bottom_depth_m)
    dmin = distances(data_coords, cen[:, :2]).min(axis=0)
    c2 = dmin.min() / dmin
    ipd = distances(cen[:, :2], cen[:, :2])
    res_w = mean_R * ipd
    num, den = np.zeros(len(cen)), np.zeros(len(cen))
    for j in range(len(cen)):
        num = num + res_w[:, j]
        den = den + ipd[j, :]
    return area_pen * c1 * c2 * (num / den), dmin


def division_mapping(npatches, div_idxs, subfault_npatches):
    """a divided patch is replaced in place by its two halves"""
    div = set(int(i) for i in div_idxs)
    old2new, div2new, new_counts = {}, {}, []
    bounds = np.cumsum([0] + list(subfault_npatches))
    tot = half = 0
    for s in range(len(subfault_npatches)):
        start = tot
        for i in range(bounds[s], bounds[s + 1]):
            if i in div:
                div2new[half], div2new[half + 1] = tot, tot + 1
                half += 2
                tot += 2
            else:
                old2new[i] = tot
                tot += 1
        new_counts.append(tot - start)
    return old2new, div2new, np.array(new_counts)


# ------------------------------------------------------------------------------------------ the loop
def optimize(cfg, subfaults, east, north, los, odw, nu, varnames, library_fn=None):
    """-> dict(params, subfault_npatches, mean_R, R_matrix, generations=[...], gfs (ncomp, P, nobs)); cfg: dict of the
    ResolutionDiscretizationConfig fields.  library_fn(rows) overrides the Okada oracle."""
    lib = library_fn or (lambda rows: library(rows, east, north, los, odw, nu))
    data_coords = np.stack([east, north], axis=1)
    rows, counts = [], []
    for i, sf in enumerate(subfaults):
        npw = n_patches(sf[7], 2 * cfg["patch_widths_max"][i])
        npl = n_patches(sf[6], 2 * cfg["patch_lengths_max"][i])
        rows.append(patches(sf, npl, npw))
        counts.append(npl * npw)
    params = np.vstack(rows)
    gfs = [lib(component_rows(params, c)) for c in varnames]
    div_idxs = []
    for i, sf in enumerate(subfaults):
        if not (sf[7] <= cfg["patch_widths_min"][i] or sf[6] <= cfg["patch_lengths_min"][i]):
            div_idxs.extend(range(int(np.sum(counts[:i])), int(np.sum(counts[:i + 1]))))
    bottom_m = np.array([(np.array(sf[:3]) + sf[7] * _vectors(sf)[1])[2] for sf in subfaults]) * km
    fixed, gens = set(), []
    tobedivided = len(params)
    while tobedivided:
        old2new, div2new, new_counts = division_mapping(len(params), div_idxs, counts)
        divided = [q for i in div_idxs for q in (patches(params[i], 2, 1) if params[i][6] >= params[i][7]
                                                 else patches(params[i], 1, 2))]
        new_params = np.zeros((int(new_counts.sum()), 10))
        new_gfs = [np.zeros((len(new_params), east.size)) for _ in varnames]
        div_gfs = [lib(component_rows(np.array(divided), c)) if divided else None for c in varnames]
        for o, n in old2new.items():
            new_params[n] = params[o]
            for k in range(len(varnames)):
                new_gfs[k][n] = gfs[k][o]
        for h, n in div2new.items():
            new_params[n] = divided[h]
            for k in range(len(varnames)):
                new_gfs[k][n] = div_gfs[k][h]
        params, gfs, counts = new_params, new_gfs, [int(c) for c in new_counts]
        fixed = set(old2new[i] for i in fixed)
        cen = centers(params)
        L = smoothing_correlated(cen, "gaussian")
        Rs, diags = [], []
        for k in range(len(varnames)):
            Rm = resolution(gfs[k].T, L, cfg["epsilon"])
            R = np.diag(Rm)
            Rs.append(Rm)
            diags.append(R)
            R_idxs = np.argwhere(R > cfg["resolution_thresh"]).ravel().tolist()
            fixed.update(np.argwhere(R <= cfg["resolution_thresh"]).ravel().tolist())
        sf_of = np.repeat(np.arange(len(counts)), counts)
        w, ln = params[:, 7], params[:, 6]
        at_min = set(np.argwhere((w <= np.array(cfg["patch_widths_min"])[sf_of])
                                 | (ln <= np.array(cfg["patch_lengths_min"])[sf_of])).ravel().tolist())
        above = set(np.argwhere((w > np.array(cfg["patch_widths_max"])[sf_of])
                                | (ln > np.array(cfg["patch_lengths_max"])[sf_of])).ravel().tolist())
        fixed = fixed.difference(above)
        cand = set(R_idxs).difference(at_min, fixed).union(above)
        mean_R = np.vstack(diags).mean(0).ravel()
        gen = dict(fixed_idxs=sorted(fixed), subfault_npatches=list(counts), R_diags=np.array(diags), mean_R=mean_R,
                   candidates=sorted(cand), at_min=sorted(at_min), gfs=np.array(gfs), L=L, params=params.copy(),
                   rating=None, dmin=None)
        if cand:
            rt, dmin = rating(w, ln, cen, bottom_m[sf_of], cfg["depth_penalty"], data_coords, mean_R)
            order = rt.argsort()[::-1]
            sel = np.array([r for r in order if r in cand])
            idxs = sel[:int(np.ceil(cfg["alpha"] * len(sel)))]
            gen.update(rating=rt, dmin=dmin, rated_sel=sel, n_cut=len(idxs))
            tobedivided = len(idxs)
            div_idxs = sorted(int(i) for i in idxs)
        else:
            tobedivided = 0
            div_idxs = []
        gen["sf_div_idxs"] = np.array(div_idxs, dtype=np.int64)
        gens.append(gen)
    return dict(params=params, subfault_npatches=counts, mean_R=mean_R, R_matrix=np.dstack(Rs).mean(2),
                generations=gens, gfs=np.array(gfs))


# ------------------------------------------------------------------------------------------ the fixture problem
def fixture_problem():
    """two subfaults (one dipping 60 deg, one vertical at exactly 90 deg), 70 points in two datasets (45 + 25) with
    distinct line-of-sight vectors and non-unit weights, an asymmetric geometry"""
    rng = np.random.RandomState(20261019)
    subfaults = np.array([
        # east north depth strike dip rake length width slip opening   [km, deg, m]
        [0.7, -1.3, 0.4, 37.0, 60.0, 12.0, 12.0, 8.0, 1.0, 0.0],
        [9.1, 6.2, 0.9, 118.0, 90.0, -35.0, 8.0, 6.5, 1.0, 0.0],
    ])
    n1, n2 = 45, 25
    east = np.concatenate([rng.uniform(-14.0, 16.0, n1), rng.uniform(-6.0, 19.0, n2)])
    north = np.concatenate([rng.uniform(-13.0, 12.0, n1), rng.uniform(-4.0, 15.0, n2)])
    # multiples of 1/64 km: the datasets hold metres, and (x * 1000) / 1000 gives x back exactly for these
    east, north = np.round(east * 64.0) / 64.0, np.round(north * 64.0) / 64.0

    def los(inc, head, n):
        inc, head = np.deg2rad(inc), np.deg2rad(head)
        return np.tile([np.sin(inc) * np.cos(head - 1.5 * np.pi), np.sin(inc) * np.sin(head - 1.5 * np.pi),
                        np.cos(inc)], (n, 1))

    los_vectors = np.vstack([los(33.0, -167.0, n1), los(41.0, -13.0, n2)])
    odw = np.concatenate([rng.uniform(0.6, 1.7, n1), rng.uniform(0.8, 2.3, n2)])
    cfg = dict(epsilon=0.02, epsilon_search_runs=3, resolution_thresh=0.95, depth_penalty=3.5, alpha=0.3,
               patch_widths_min=[1.0, 1.7], patch_widths_max=[2.0, 1.7], patch_lengths_min=[1.0, 2.0],
               patch_lengths_max=[2.0, 2.0])
    return dict(subfaults=subfaults, east=east, north=north, los=los_vectors, odw=odw, sizes=[n1, n2], nu=0.25,
                cfg=cfg, varnames=["uparr", "uperp"])
