"""
A numpy restatement of the mechanism-ensemble arrays (beat_amd/mechanisms.py, csrc/mechanism.hpp, csrc/mechanisms.hip), one
draw at a time where the reference loops (beat/plotting/seismic.py):

  :1334-1384   lower_focalsphere_angles       -> focal_grid
  :1387-1425   mts2amps                       -> unit6, amplitudes, fuzzy_count, fuzzy_sum, mts2amps
  :1689-1696   MomentTensor.standard_decomposition, as fuzzy_mt_decomposition reads it -> standard_decomposition
  :2183-2310   draw_hudson's (u, v)           -> hudson_uv
  :1223-1224   the ensemble thinning          -> thin

The decomposition, the inverse projections and Hudson's projection restate pyrocko from memory (pyrocko is not installed
where these tests run); they are the rules the issue states, not a verified copy of pyrocko's behaviour.  Eigen-systems come
from ``numpy.linalg.eigh`` here (LAPACK), from Jacobi rotations in the code under test: the two agree to rounding, not to
the bit, so comparisons of decomposed quantities carry a bound; the (pixel, draw) accumulations are exact restatements.
"""
import numpy as np

PARTS = ("iso", "dc", "clvd", "dev", "full")
SQRT2 = 1.4142135623730951


def symmat6(m):
    mnn, mee, mdd, mne, mnd, med = [float(v) for v in m]
    return np.array([[mnn, mne, mnd], [mne, mee, med], [mnd, med, mdd]])


def to6(m9):
    return np.array([m9[0, 0], m9[1, 1], m9[2, 2], m9[0, 1], m9[0, 2], m9[1, 2]])


def eigensystem(m):
    """ascending eigenvalues and eigenvector columns of symmat6(m)"""
    return np.linalg.eigh(symmat6(m))


def standard_decomposition(m):
    """-> (moments (5,), ratios (5,), parts (5, 6)) in the order of PARTS"""
    m9 = symmat6(m)
    third = np.trace(m9) / 3.0
    m_iso = third * np.eye(3)
    m_dev = m9 - m_iso
    e, v = np.linalg.eigh(m_dev)
    order = np.argsort(np.abs(e), kind="stable")
    e, v = e[order], v[:, order]
    moment_iso, moment_dev = abs(third), np.abs(e).max()
    moment = moment_iso + moment_dev
    if moment_dev < 1e-6 * moment_iso:
        signed_dc = 0.0
    else:
        signed_dc = e[2] * (1.0 + 2.0 * min(0.0, e[0] / e[2]))
    m_dc = signed_dc * (np.outer(v[:, 2], v[:, 2]) - np.outer(v[:, 1], v[:, 1]))
    m_clvd = m_dev - m_dc
    moments = np.array([moment_iso, abs(signed_dc), moment_dev - abs(signed_dc), moment_dev, moment])
    ratios = moments / moment
    ratios[4] = 1.0
    return moments, ratios, np.array([to6(p) for p in (m_iso, m_dc, m_clvd, m_dev, m9)])


def unit6(m):
    """the six entries of m9 / (sqrt(sum m9 ** 2) / sqrt 2) (seismic.py:1410-1417)"""
    m9 = symmat6(m)
    with np.errstate(invalid="ignore", divide="ignore"):
        return to6(m9 / (np.sqrt(np.sum(m9 ** 2)) / SQRT2))


def hudson_uv(evals):
    """Hudson, Pearce & Rogers (1989) from the three eigenvalues of the full tensor, in any order"""
    m3, m2, m1 = np.sort(np.asarray(evals, dtype=np.float64))
    iso = (m1 + m2 + m3) / 3.0
    d1, d2, d3 = m1 - iso, m2 - iso, m3 - iso
    big = max(abs(d1), abs(d3))
    k = iso / (abs(iso) + big)
    t = 2.0 * d2 / big if big != 0.0 else 0.0
    tau = t * (1.0 - abs(k))
    if tau * k <= 0.0:
        return tau, k
    if tau > 0.0:
        den = 1.0 - tau / 2.0 if tau < 4.0 * k else 1.0 - 2.0 * k
    else:
        den = 1.0 + tau / 2.0 if tau > 4.0 * k else 1.0 + 2.0 * k
    return tau / den, k / den


def hudson_of(m):
    return hudson_uv(np.linalg.eigvalsh(symmat6(m)))


def thin(n_mts, nensemble):
    return np.floor(np.arange(0, n_mts, float(n_mts) / nensemble)).astype("int32")


# ------------------------------------------------------------------------------------------------ the focal-sphere grid
def focal_grid(res, projection="lambert"):
    """-> (inside (res * res,) bool, takeoff, azimuth of the pixels inside, x, y); pixel iy * res + ix is (x[ix], y[iy])"""
    x = np.linspace(-1.0, 1.0, res)
    y = np.linspace(-1.0, 1.0, res)
    px, py = np.meshgrid(x, y)            # rows: y, columns: x -- tile / repeat
    p0, p1 = px.ravel(), py.ravel()
    inside = p0 ** 2 + p1 ** 2 <= 1.0
    p0, p1 = p0[inside], p1[inside]
    r2 = p0 ** 2 + p1 ** 2
    if projection == "lambert":
        vz, vy, vx = 1.0 - r2, np.sqrt(2.0 - r2) * p0, np.sqrt(2.0 - r2) * p1
    elif projection == "stereographic":
        vz, vy, vx = -(r2 - 1.0) / (r2 + 1.0), 2.0 * p0 / (r2 + 1.0), 2.0 * p1 / (r2 + 1.0)
    elif projection == "orthographic":
        vz, vy, vx = np.sqrt(np.maximum(1.0 - r2, 0.0)), p0, p1
    else:
        raise ValueError(projection)
    r = np.sqrt(vx ** 2 + vy ** 2 + vz ** 2)
    return inside, np.arccos(vz / r), np.arctan2(vy, vx), x, y


# ------------------------------------------------------------------------------------------------ (pixel, draw) sums
def amplitudes(rw, u):
    """(npix,): the amplitudes of one unit tensor u (6,) at the pixels of rw (6, npix), products and sums one by one in
    the order the kernels state (numpy's elementwise operations round once each and fuse nothing)"""
    with np.errstate(invalid="ignore"):
        a = rw[0] * u[0] + rw[1] * u[1]
        for k in range(2, 6):
            a = a + rw[k] * u[k]
    return a


def fuzzy_count(unit, rw):
    """unit (n, P, 6), rw (6, npix) -> int64 counts (P, npix) of the draws with a > 0"""
    n, P = unit.shape[:2]
    c = np.zeros((P, rw.shape[1]), dtype=np.int64)
    for i in range(n):
        for p in range(P):
            with np.errstate(invalid="ignore"):
                c[p] += amplitudes(rw, unit[i, p]) > 0
    return c


def fuzzy_sum(unit, rw):
    """unit (n, P, 6), rw (6, npix) -> (P, npix): the amplitudes added draw by draw in ascending order"""
    n, P = unit.shape[:2]
    s = np.zeros((P, rw.shape[1]))
    for i in range(n):
        for p in range(P):
            s[p] += amplitudes(rw, unit[i, p])
    return s


def to_grid(values, inside, n, res):
    """(P, npix) counts or sums -> (P, res, res): values / n inside, NaN outside"""
    out = np.full((values.shape[0], res * res), np.nan)
    out[:, inside] = values.astype(np.float64) / float(n)
    return out.reshape(-1, res, res)


def mts2amps(mts, projection, beachball_type, res, rw, mask=True):
    """the grid of an ensemble (n, 6) by numpy's own decomposition; rw (6, npix) of the grid's pixels"""
    which = {"full": 4, "deviatoric": 3, "dc": 1}[beachball_type]
    inside = focal_grid(res, projection)[0]
    unit = np.array([[unit6(standard_decomposition(m)[2][which])] for m in mts])
    vals = fuzzy_count(unit, rw) if mask else fuzzy_sum(unit, rw)
    return to_grid(vals, inside, len(mts), res)[0], unit
