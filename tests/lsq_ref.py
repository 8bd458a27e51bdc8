"""numpy restatement of the least-squares start (csrc/lsq.hip; reference beat/models/problems.py:753-873): the design
matrix A and right-hand side d of a point, row order seismic (wavemap, target, sample), geodetic, laplacian; the active set
of Lawson & Hanson on the normal equations as the kernel runs it; the bounds the tests hold both to.  Test infrastructure
only: nothing here is imported by the product."""
import numpy as np

EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------- design matrix
def time_indexes(x, xmin, dx, interpolation):
    """beat/ffi/base.py:486-568: nearest neighbour round((x - min) / dx).astype(int16); multilinear ceil and the factor
    ceil - x (the weight of the floor node)"""
    y = (np.asarray(x, dtype=np.float64) - xmin) / dx
    if interpolation == "nearest_neighbor":
        return np.round(y).astype("int16"), None
    c = np.ceil(y).astype("int16")
    return c, c - y


def seismic_design(G, grid, starttimes, durations, interpolation):
    """A [(T N), P]: column p = the synthetic of patch p alone with unit slip (stack_all with patchidxs=[p], slips=[1.]).
    G [T, P, D, S, N]; grid = (st_min, st_dt, du_min, du_dt); starttimes [T, P]; durations [P]"""
    T, P, D, S, N = G.shape
    st_min, st_dt, du_min, du_dt = grid
    si, sf = time_indexes(starttimes, st_min, st_dt, interpolation)
    di, df = time_indexes(durations, du_min, du_dt, interpolation)
    tt, pp = np.meshgrid(np.arange(T), np.arange(P), indexing="ij")
    dd = np.broadcast_to(di[None, :], (T, P))
    if interpolation == "nearest_neighbor":
        R = G[tt, pp, dd, si, :]                                    # [T, P, N]
    else:
        rt = np.broadcast_to(df[None, :], (T, P))[..., None]
        stf = sf[..., None]
        # base.py:663-698: (st ceil, rt ceil), (st floor, rt ceil), (st ceil, rt floor), (st floor, rt floor), summed in
        # this order with plain products
        R = ((1 - stf) * (1 - rt)) * G[tt, pp, dd, si, :]
        R = R + (stf * (1.0 - rt)) * G[tt, pp, dd, si - 1, :]
        R = R + ((1 - stf) * rt) * G[tt, pp, dd - 1, si, :]
        R = R + (stf * rt) * G[tt, pp, dd - 1, si - 1, :]
    return np.ascontiguousarray(R.transpose(0, 2, 1).reshape(T * N, P))


def design(case, c):
    """(A, d) of chain c of a fixture case (dict of arrays, tools/gen_golden_lsq.py)"""
    rows, rhs = [], []
    P = int(case["P"])
    for w in range(int(case["nwm"])):
        G = case["wm%d_G" % w]
        st = case["st0"][c][None, :] - case["wm%d_shift" % w][c][:, None]      # seismic.py:1283-1296
        interp = "multilinear" if int(case["wm%d_ml" % w]) else "nearest_neighbor"
        rows.append(seismic_design(G, case["wm%d_grid" % w], st, case["durations"][c], interp))
        rhs.append(case["wm%d_data" % w].ravel())
    if int(case["has_geo"]):
        rows.append(case["geo_G"].T)
        rhs.append(case["geo_data"] - case["geo_corr"][c])
    h = float(case["h"][c])
    rows.append(case["L"] * h ** 2.0)
    rhs.append(np.zeros(P))
    return np.vstack(rows), np.concatenate(rhs)


# ------------------------------------------------------------------------------------------------- active set
def nnls_normal(Nm, b, maxiter=None):
    """Lawson & Hanson's active set on N = A^T A, b = A^T d as k_nnls runs it -> (x, iters, status, removed).
    iters counts the solves of the passive system; status 0 ok, 1 cap reached, 2 non-finite / not positive definite;
    removed: variables that left the passive set (the inner loop)"""
    Nm, b = np.asarray(Nm, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = b.size
    maxiter = 3 * n if not maxiter else int(maxiter)
    if not (np.isfinite(Nm).all() and np.isfinite(b).all()):
        return np.full(n, np.nan), 0, 2, 0
    tol = 10.0 * n * EPS * (np.abs(b).max() if n else 0.0)
    x, w = np.zeros(n), b.copy()
    passive, inP = [], np.zeros(n, dtype=bool)
    iters = removed = 0
    while len(passive) < n:
        cand = np.where(~inP, w, -np.inf)
        j = int(np.argmax(cand))
        if not cand[j] > tol:
            break
        passive.append(j)
        inP[j] = True
        while True:
            if iters >= maxiter:
                return x, iters, 1, removed
            iters += 1
            idx = np.array(passive)
            try:
                Lc = np.linalg.cholesky(Nm[np.ix_(idx, idx)])
            except np.linalg.LinAlgError:
                return np.full(n, np.nan), iters, 2, removed
            s = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b[idx]))
            if not s.min() < 0:
                break
            neg = s < 0
            alpha = (x[idx][neg] / (x[idx][neg] - s[neg])).min()
            x[idx] = x[idx] * (1.0 - alpha) + alpha * s
            keep = x[idx] > tol
            removed += int((~keep).sum())
            for k in idx[~keep]:
                inP[k] = False
                x[k] = 0.0
            passive = [k for k in passive if inP[k]]
            if not passive:
                s = np.zeros(0)
                break
        x[:] = 0.0
        x[np.array(passive, dtype=int)] = s
        w = b - Nm @ x
    return x, iters, 0, removed


def passive_cond(A, m):
    """cond_2 of the columns of A on the support of m (1 for an empty support)"""
    sup = np.nonzero(m)[0]
    return float(np.linalg.cond(A[:, sup])) if sup.size else 1.0


def solution_bound(A, m_ref):
    """|m - m_ref|_inf allowed to a solution through the normal equations: they square the condition number of the
    passive columns; 10^3 is the margin"""
    return 1e3 * EPS * passive_cond(A, m_ref) ** 2 * float(np.abs(m_ref).max())


def decision_floor(A, m):
    """the smallest margin (a fraction of its decision's scale) at which a float64 active set through the normal equations
    is held to take the decisions of the exact one: the relative error solution_bound allows to a solution.  A condition
    on the inputs of a decision-exact test, checked on the reference alone."""
    return 1e3 * EPS * passive_cond(A, m) ** 2


def nnls_system(n, seed, rho, frac, noise, rows=None):
    """a seeded system (A [rows, n], d [rows]) for the active set: entries of B multiples of 1/64 in [-127/64, 127/64],
    A = B + rho (B one column to the left + B one column to the right, zeros shifted in), x_true uniform in (0.5, 2) with
    probability frac, else 0, d = A x_true + noise sqrt(n) standard normal.  rho = 0: removals are rare; rho = 0.45:
    neighbouring columns correlate, variables leave the passive set often, cond_2 of the passive columns stays below 20."""
    rng = np.random.default_rng(seed)
    rows = 2 * n if rows is None else int(rows)
    B = rng.integers(-127, 128, (rows, n)) / 64.0
    left, right = np.zeros_like(B), np.zeros_like(B)
    left[:, :-1], right[:, 1:] = B[:, 1:], B[:, :-1]
    A = B + rho * (left + right)
    x_true = np.where(rng.random(n) < frac, rng.uniform(0.5, 2.0, n), 0.0)
    d = A @ x_true + noise * np.sqrt(n) * rng.standard_normal(rows)
    return A, d


LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def _solve_refined(NL, bL, idx):
    """N_PP s = b_P: a float64 Cholesky solve and two refinements on the long-double residual -> (s, |residual|_2 + the
    bound of the residual's own rounding: over lambda_min(N_PP) it bounds |s - exact|_2)"""
    from scipy.linalg import cho_factor, cho_solve
    Npp = NL[np.ix_(idx, idx)]
    bp = bL[idx]
    cf = cho_factor(Npp.astype(np.float64))
    s = cho_solve(cf, bp.astype(np.float64)).astype(LD)
    for _ in range(2):
        s = s + cho_solve(cf, (bp - Npp @ s).astype(np.float64)).astype(LD)
    res = bp - Npp @ s
    own = (len(idx) + 2) * EPS_LD * (np.abs(Npp) @ np.abs(s) + np.abs(bp))
    return s, float(np.sqrt((res * res).sum()) + np.sqrt((own * own).sum()))


def nnls_margins(Nm, b, maxiter=None):
    """nnls_normal with every compared quantity (w, s, alpha, the interpolated x) in long double -> dict:
    x (float64), iters, status, removed, events (one (passive variables before the step, variables that left) per removal
    step), entered (the variables in their order of entry, re-entries included), margins (the smallest of each kind of
    decision, a fraction of that decision's scale, inf where the decision never came up):
      arg    largest minus second largest candidate w, over max|b|
      tol    |w_j - tol| at every entry and at the stop, over max|b|
      neg    min|s_k| over max|s|, at every solve
      alpha  the gap between the two smallest ratios x / (x - s)
      keep   min |x_k - tol| over max|s|, over the variables that stay after a removal step
    and solve_err, the bound of the solves' own error in the same units: the largest over all solves of |ds| / max|s|,
    |N|_inf |ds| / max|b| and of the error |ds| gives a ratio, with |ds| <= |residual| / lambda_min(N_EE), E the variables
    that ever entered (Cauchy interlacing: every passive block is a principal block of N_EE)."""
    NL, bL = np.asarray(Nm, dtype=np.float64).astype(LD), np.asarray(b, dtype=np.float64).astype(LD)
    n = bL.size
    maxiter = 3 * n if not maxiter else int(maxiter)
    bmax = float(np.abs(bL).max())
    tol = LD(10.0 * n * EPS * bmax)                    # the kernel's float64 number
    norm_inf = float(np.abs(NL).sum(axis=1).max())
    mg = dict(arg=np.inf, tol=np.inf, neg=np.inf, alpha=np.inf, keep=np.inf)
    x, w = np.zeros(n, dtype=LD), bL.copy()
    passive, inP, entered, events = [], np.zeros(n, dtype=bool), [], []
    iters = removed = status = 0
    raw_err = 0.0

    def result():
        solve_err = 0.0
        if entered:
            E = np.unique(entered)
            ev = np.linalg.eigvalsh(NL[np.ix_(E, E)].astype(np.float64))
            assert ev[0] > 1e-10 * ev[-1], "nnls_margins: the entered block is not safely positive definite"
            solve_err = raw_err / float(ev[0])
        return dict(x=x.astype(np.float64), iters=iters, status=status, removed=removed, events=events, entered=entered,
                    margins=dict((k, float(v)) for k, v in mg.items()), solve_err=solve_err)

    while len(passive) < n:
        cand = np.where(~inP, w, -np.inf)
        j = int(np.argmax(cand))
        if bmax == 0.0:
            break
        mg["tol"] = min(mg["tol"], abs(cand[j] - tol) / bmax)
        if not cand[j] > tol:
            break
        if n - len(passive) > 1:
            second = np.partition(cand, n - 2)[n - 2]
            mg["arg"] = min(mg["arg"], (cand[j] - second) / bmax)
        passive.append(j)
        entered.append(j)
        inP[j] = True
        while True:
            if iters >= maxiter:
                status = 1
                return result()
            iters += 1
            idx = np.array(passive)
            s, ds = _solve_refined(NL, bL, idx)
            smax = float(np.abs(s).max())
            raw_err = max(raw_err, ds / smax, norm_inf * ds / bmax)
            mg["neg"] = min(mg["neg"], np.abs(s).min() / smax)
            if not s.min() < 0:
                break
            neg = s < 0
            xp = x[idx]
            ratio = xp[neg] / (xp[neg] - s[neg])
            raw_err = max(raw_err, float((ds * (np.abs(xp[neg]) + np.abs(s[neg])) / (xp[neg] - s[neg]) ** 2).max()))
            if ratio.size > 1:
                two = np.partition(ratio, 1)[:2]
                mg["alpha"] = min(mg["alpha"], two[1] - two[0])
            alpha = ratio.min()
            xp = xp * (1 - alpha) + alpha * s
            x[idx] = xp
            keep = xp > tol
            if keep.any():
                mg["keep"] = min(mg["keep"], np.abs(xp[keep] - tol).min() / smax)
            events.append((len(passive), int((~keep).sum())))
            removed += int((~keep).sum())
            for k in idx[~keep]:
                inP[k] = False
                x[k] = 0
            passive = [k for k in passive if inP[k]]
            if not passive:
                s = np.zeros(0, dtype=LD)
                break
        x[:] = 0
        x[np.array(passive, dtype=int)] = s
        w = bL - NL[:, passive] @ x[passive]
    return result()


def gram_bound(A):
    """entrywise bound of |fl(A^T A) - A^T A| for two floating-point evaluations in any order of summation: each is within
    (n_rows + 2) 2^-53 (|A|^T |A|)_ij of the exact value (n products, n - 1 sums, a mirrored copy or blend rounding)"""
    Aa = np.abs(A)
    return 2.0 * (A.shape[0] + 2) * 2.0 ** -53 * (Aa.T @ Aa)


def rhs_bound(A, d):
    return 2.0 * (A.shape[0] + 2) * 2.0 ** -53 * (np.abs(A).T @ np.abs(d))


# ------------------------------------------------------------------------------------------------- fixture cases -> problems
def load_case(g, name):
    """the arrays of one case of tests/golden/lsq.npz, without the prefix"""
    pre = name + "_"
    return dict((k[len(pre):], g[k]) for k in g.files if k.startswith(pre))


def synthetic_case(grid, T, N, interpolation, C, seed, h=(0.5, 1.0), nshift=2):
    """a seeded seismic case of any size in the layout of the fixture's (no A, d, m_ref; st0 is left to the caller):
    grid = (n dip, n strike, patch size)"""
    rng = np.random.default_rng(seed)
    nd, ns, psz = grid
    P = nd * ns
    D, du_min, du_dt, st_min, st_dt = 3, 0.5, 0.5, 0.0, 0.5
    vel, time, shift = (2.5, 4.0), (0.5, 1.0), (-0.5, 0.5)
    S = int(np.ceil(((nd + ns) * psz / vel[0] + time[1] + shift[1]) / st_dt)) + 2
    names = ["uparr", "uperp", "durations", "velocities", "nucleation_strike", "nucleation_dip", "time", "time_shifts",
             "h_seis", "h_laplacian"]
    sizes = [P, P, P, P, 1, 1, 1, nshift, 1, 1]
    lo = [0.0, -1.0, du_min, vel[0], 0.0, 0.0, time[0], shift[0], -1.0, h[0]]
    up = [5.0, 1.0, du_min + (D - 1) * du_dt, vel[1], ns * psz - 0.51 * psz, nd * psz - 0.51 * psz, time[1], shift[1], 1.0, h[1]]
    lower = np.concatenate([np.full(s, v) for s, v in zip(sizes, lo)])
    upper = np.concatenate([np.full(s, v) for s, v in zip(sizes, up)])
    Q = lower + (upper - lower) * rng.random((C, lower.size))
    offs = dict(zip(names, np.concatenate([[0], np.cumsum(sizes)[:-1]])))
    sidx = np.arange(T) % nshift
    # the smoothing operator of synthetic.py's problems (any invertible operator serves the normal equations)
    from beat_amd.synthetic import smoothing_operator_nearest_neighbor
    case = dict(P=np.array(P), grids=np.array([grid], dtype=np.float64), nwm=np.array(1), names=np.array(names),
                sizes=np.array(sizes), lower=lower, upper=upper, Q=Q, L=smoothing_operator_nearest_neighbor(ns, nd, psz, psz),
                has_geo=np.array(0), has_ramp=np.array(0), geo_sizes=np.zeros(0, dtype=np.int64),
                h=Q[:, offs["h_laplacian"]].copy(), durations=Q[:, offs["durations"]:offs["durations"] + P].copy(),
                wm0_G=rng.integers(-127, 128, (T, P, D, S, N)) / 64.0, wm0_grid=np.array([st_min, st_dt, du_min, du_dt]),
                wm0_ml=np.array(int(interpolation == "multilinear")), wm0_data=3.0 * rng.integers(-127, 128, (T, N)) / 64.0,
                wm0_sidx=sidx, wm0_has_shift=np.array(1),
                wm0_shift=Q[:, offs["time_shifts"]:offs["time_shifts"] + nshift][:, sidx].copy())
    return case


def build_problem(case, seed=5):
    """FFIProblem over a case: slip variables (uparr, uperp), unit scalar weights, the case's layout and prior box.  The
    uperp libraries (not part of the least-squares problem) are seeded noise."""
    from collections import OrderedDict

    from beat_amd.ffi import (GeodeticGFLibrary, GeodeticGFLibraryConfig, SeismicGFLibrary,
                              SeismicGFLibraryConfig)
    from beat_amd.models import FFIProblem, GeodeticData, ParameterLayout, RampConfig, SeismicWavemap
    rng = np.random.default_rng(seed)
    names, sizes = [str(n) for n in case["names"]], [int(s) for s in case["sizes"]]
    lay = ParameterLayout(OrderedDict(zip(names, sizes)))
    lower, upper = {}, {}
    for n in names:
        o = lay.offsets[n]
        lower[n], upper[n] = case["lower"][o:o + lay.varsizes[n]], case["upper"][o:o + lay.varsizes[n]]
    P = int(case["P"])
    wavemaps = []
    for w in range(int(case["nwm"])):
        G = case["wm%d_G" % w]
        grid = case["wm%d_grid" % w]
        gfs = {}
        for v in ("uparr", "uperp"):
            gf = SeismicGFLibrary(SeismicGFLibraryConfig(dimensions=G.shape, starttime_sampling=float(grid[1]),
                                                         duration_sampling=float(grid[3]), starttime_min=float(grid[0]),
                                                         duration_min=float(grid[2]), component=v, mapnumber=w))
            gf.setup(*G.shape, allocate=True)
            gf._gfmatrix[:] = G if v == "uparr" else rng.standard_normal(G.shape)
            gfs[v] = gf
        T = G.shape[0]
        ts = ("time_shifts", case["wm%d_sidx" % w]) if int(case["wm%d_has_shift" % w]) else None
        wavemaps.append(SeismicWavemap(gfs, case["wm%d_data" % w], np.ones(T), np.zeros(T), [("h_seis", 0)] * T, ts,
                                       "multilinear" if int(case["wm%d_ml" % w]) else "nearest_neighbor", name="any_P_%d" % w))
    geodetic = None
    if int(case["has_geo"]):
        gsz = [int(n) for n in case["geo_sizes"]]
        ggfs = {}
        for v in ("uparr", "uperp"):
            gg = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=(P, sum(gsz)), component=v))
            gg.setup(P, sum(gsz), allocate=True)
            gg._gfmatrix[:] = case["geo_G"] if v == "uparr" else 0.1 * rng.standard_normal((P, sum(gsz)))
            ggfs[v] = gg
        corrections = None
        if int(case["has_ramp"]):
            ramp_ = RampConfig(dataset_names=["scene_0"], enabled=True).init_correction()
            ramp_.setup_correction(case["geo_north"], case["geo_east"], None, None, "scene_0")
            corrections = [[ramp_]] + [[] for _ in gsz[1:]]
        geodetic = GeodeticData(ggfs, case["geo_data"], case["geo_odw"], gsz, [1.0] * len(gsz), [0.0] * len(gsz),
                                [("h_geo", 0)] * len(gsz), corrections=corrections)
    grids = case["grids"]
    prob = FFIProblem(lay, [int(g[0]) for g in grids], [int(g[1]) for g in grids], [float(g[2]) for g in grids],
                      ["uparr", "uperp"], wavemaps, geodetic, (case["L"], 0.0), lower, upper)
    return prob, lay
