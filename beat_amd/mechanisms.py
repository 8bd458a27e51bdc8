"""
The arrays behind the three figures of a moment-tensor ensemble, computed on the device for whole populations -- what the
reference computes draw by draw in a Python loop:

  beat/plotting/seismic.py:1334-1425    ``lower_focalsphere_angles`` / ``mts2amps`` (``beat plot fuzzy_beachball``)
  beat/plotting/seismic.py:1664-1850    ``fuzzy_mt_decomposition`` (``beat plot fuzzy_mt_decomp``)
  beat/plotting/seismic.py:2183-2310    ``draw_hudson`` (``beat plot hudson``)
  beat/plotting/seismic.py:1223-1224    the thinning of an ensemble to ``nensemble`` draws

``mts`` is (n, 6) = (mnn, mee, mdd, mne, mnd, med) or (n, 3) = strike, dip, rake in degrees -- the two forms
``extract_mt_components`` produces, and what ``f.moment_tensors(Q)`` returns: a numpy array (results are numpy) or a
torch-cuda tensor (results are tensors on its device).  ``ctx=None`` takes ``get_context``.  Plotting itself (colour maps,
the best-solution contour, the beachball outline) stays with the caller.  There is no CPU fallback: without a GPU the device
functions raise ``BeatAmdError``.

UNVERIFIED RESTATEMENTS.  pyrocko is not a dependency of this package and was not at hand when this was written, so the
following are restated from memory of its published source and pinned only to multi-precision evaluations of the rules as
stated here (csrc/mechanism.hpp, tests/mechanisms_ref.py):
  * ``MomentTensor.standard_decomposition`` and ``deco_part``;
  * ``beachball.inverse_project`` and ``numpy_xyz2rtp`` (``lower_focalsphere_angles``);
  * Hudson's (u, v) with T = 2 m2' / D; the sign convention of ``pyrocko.plot.hudson.project`` has not been compared.

Deviations from the reference, all stated where they apply:
  * a row with a non-finite entry, or an all-zero tensor, raises ``ValueError`` naming the row (numpy would spread NaN over
    the whole grid);
  * the amplitude of a (pixel, draw) pair is summed in one stated order, ``((((r0 u0 + r1 u1) + r2 u2) + r3 u3) + r4 u4)
    + r5 u5`` (the reference's ``dot`` leaves the order to BLAS);
  * ``view`` other than ``"top"`` raises ``NotImplementedError`` (the view rotations are pyrocko's).
"""
import numpy as np

from . import mechanisms_binding as mb
from ._marshal import is_dev, upload
from .engine import get_context
from .heart import calculate_radiation_weights, radiation_function_mapping

PROJECTIONS = ("lambert", "stereographic", "orthographic")
PART_NAMES = mb.PART_NAMES
MT_TYPES = {"full": "full", "deviatoric": "dev", "dc": "dc"}      # deco_part's mt_type -> the part of the decomposition


# ------------------------------------------------------------------------------------------------ host functions
def thin_ensemble(n_mts, nensemble):
    """the indices of the ``nensemble`` draws the figures take from ``n_mts`` (seismic.py:1223-1224):
    ``floor(arange(0, n_mts, n_mts / nensemble))`` as int32"""
    n_mts, nensemble = int(n_mts), int(nensemble)
    if n_mts < 1 or nensemble < 1:
        raise ValueError("thin_ensemble: need n_mts >= 1 and nensemble >= 1, got %d and %d" % (n_mts, nensemble))
    csteps = float(n_mts) / nensemble
    return np.floor(np.arange(0, n_mts, csteps)).astype("int32")


def inverse_project(points, projection="lambert"):
    """(m, 2) points of the unit disc -> (m, 3) unit vectors of the lower focal sphere (pyrocko's
    ``beachball.inverse_project``, restated from memory, unverified)"""
    points = np.asarray(points, dtype=np.float64)
    out = np.zeros((points.shape[0], 3), dtype=np.float64)
    rsqr = points[:, 0] ** 2 + points[:, 1] ** 2
    if projection == "lambert":
        out[:, 2] = 1.0 - rsqr
        out[:, 1] = np.sqrt(2.0 - rsqr) * points[:, 0]
        out[:, 0] = np.sqrt(2.0 - rsqr) * points[:, 1]
    elif projection == "stereographic":
        out[:, 2] = -(rsqr - 1.0) / (rsqr + 1.0)
        out[:, 1] = 2.0 * points[:, 0] / (rsqr + 1.0)
        out[:, 0] = 2.0 * points[:, 1] / (rsqr + 1.0)
    elif projection == "orthographic":
        out[:, 2] = np.sqrt(np.maximum(1.0 - rsqr, 0.0))
        out[:, 1] = points[:, 0]
        out[:, 0] = points[:, 1]
    else:
        raise ValueError("unknown projection %r (%s)" % (projection, ", ".join(PROJECTIONS)))
    return out


def lower_focalsphere_angles(grid_resolution, projection):
    """-> (amps, takeoff, azimuths, ii_ok, x, y), the reference's tuple (seismic.py:1334-1384): ``amps`` (res * res,) NaN
    outside the unit disc and 0 inside; the takeoff angle and azimuth [rad] of the ``ii_ok.sum()`` pixels inside; pixel
    ``iy * res + ix`` is ``(x[ix], y[iy])``.  theta = arccos(z / r), phi = arctan2(y, x) of the inverse projection
    (pyrocko's ``numpy_xyz2rtp``, restated from memory, unverified)."""
    res = mb.check_resolution(grid_resolution)
    if projection not in PROJECTIONS:
        raise ValueError("unknown projection %r (%s)" % (projection, ", ".join(PROJECTIONS)))
    x = np.linspace(-1.0, 1.0, res)
    y = np.linspace(-1.0, 1.0, res)
    vecs2 = np.zeros((res * res, 2), dtype=np.float64)
    vecs2[:, 0] = np.tile(x, res)
    vecs2[:, 1] = np.repeat(y, res)
    ii_ok = vecs2[:, 0] ** 2 + vecs2[:, 1] ** 2 <= 1.0
    amps = np.full(res * res, np.nan, dtype=np.float64)
    amps[ii_ok] = 0.0
    v = inverse_project(vecs2[ii_ok, :], projection)
    r = np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2 + v[:, 2] ** 2)
    return amps, np.arccos(v[:, 2] / r), np.arctan2(v[:, 1], v[:, 0]), ii_ok, x, y


_SPHERES = {}


def focal_sphere(grid_resolution, projection, wavename="any_P"):
    """-> (rw (6, npix), pixel_index int64 (npix,), x, y) of a grid: the propagation coefficients of the pixels inside the
    unit disc (``heart.calculate_radiation_weights``), formed on the host once per (resolution, projection, wave)"""
    if wavename not in radiation_function_mapping:
        raise ValueError("unknown wavename %r (%s)" % (wavename, ", ".join(sorted(radiation_function_mapping))))
    key = (mb.check_resolution(grid_resolution), projection, wavename)
    if key not in _SPHERES:
        _, takeoff, azimuths, ii_ok, x, y = lower_focalsphere_angles(grid_resolution, projection)
        rw = np.ascontiguousarray(calculate_radiation_weights(takeoff, azimuths, wavename=wavename), dtype=np.float64)
        if len(_SPHERES) >= 8:
            _SPHERES.clear()
        _SPHERES[key] = (rw, np.flatnonzero(ii_ok).astype(np.int64), x, y)
    return _SPHERES[key]


# ------------------------------------------------------------------------------------------------ device functions
def _on_device(mts, ctx):
    """-> (ctx, the draws as a device tensor, host?); the argument rules are checked before the device is touched"""
    if is_dev(mts):
        X, _, _ = mb.check_mts(mts.contiguous())
        return (ctx or get_context(X.device.index)), X, False
    X, _, _ = mb.check_mts(np.asarray(mts, dtype=np.float64))
    ctx = ctx or get_context()      # (raises without the library or a GPU)
    return ctx, upload(X, "cuda:%d" % ctx.device, np.float64), True


def _back(a, host):
    return a.cpu().numpy() if host else a


class EigenSystems(object):
    """``evals`` (n, 3) ascending, ``evecs`` (n, 3, 3): column j of ``evecs[i]`` is the eigenvector of ``evals[i, j]``"""

    def __init__(self, evals, evecs):
        self.evals, self.evecs = evals, evecs


class Decompositions(object):
    """``moments`` (n, 5), ``ratios`` (n, 5), ``parts`` (n, 5, 6) in the order ``names`` = iso, dc, clvd, dev, full"""
    names = PART_NAMES

    def __init__(self, moments, ratios, parts):
        self.moments, self.ratios, self.parts = moments, ratios, parts

    def part(self, name):
        return self.parts[:, PART_NAMES.index(name), :]


def eigensystems(mts, ctx=None):
    """the eigen-decomposition of every draw's full tensor (cyclic Jacobi rotations, csrc/mechanism.hpp)"""
    ctx, X, host = _on_device(mts, ctx)
    r = mb.mt_decompose(ctx, X, want=("evals", "evecs"))
    return EigenSystems(_back(r["evals"], host), _back(r["evecs"], host))


def standard_decompositions(mts, ctx=None):
    """``MomentTensor.standard_decomposition`` of every draw (seismic.py:1689-1696; restated, unverified):
    m_iso = tr/3 I; the deviatoric rest split into the double couple ``signed_dc (v2 v2^T - v1 v1^T)`` and the CLVD, with
    ``signed_dc = e2 (1 + 2 min(0, e0 / e2))`` of the deviatoric eigenvalues ordered by magnitude (0 where the deviatoric
    moment is below 1e-6 of the isotropic one); moment = |tr/3| + max|e|; ratios are moments over it -> ``Decompositions``"""
    ctx, X, host = _on_device(mts, ctx)
    r = mb.mt_decompose(ctx, X, want=("moments", "ratios", "parts"))
    return Decompositions(_back(r["moments"], host), _back(r["ratios"], host), _back(r["parts"], host))


def _mt_type(mt_type):
    if mt_type not in MT_TYPES:
        raise ValueError("unknown mt_type %r (%s)" % (mt_type, ", ".join(MT_TYPES)))
    return PART_NAMES.index(MT_TYPES[mt_type])


def deco_parts(mts, mt_type="full", ctx=None):
    """(n, 6): the ``full``, ``deviatoric`` or ``dc`` part of every draw (pyrocko's ``beachball.deco_part``, view "top")"""
    p = _mt_type(mt_type)
    ctx, X, host = _on_device(mts, ctx)
    return _back(mb.mt_decompose(ctx, X, want=("parts",))["parts"][:, p, :].contiguous(), host)


def hudson_project(mts, ctx=None):
    """-> (u, v), each (n,): the source-type coordinates of Hudson, Pearce & Rogers (1989) of every draw, from the
    eigenvalues m1 >= m2 >= m3 of the full tensor: k = iso / (|iso| + D), T = 2 m2' / D, tau = T (1 - |k|), then the
    quadrant rules (csrc/mechanism.hpp).  The sign convention has not been compared with pyrocko's."""
    ctx, X, host = _on_device(mts, ctx)
    uv = mb.mt_decompose(ctx, X, want=("uv",))["uv"]
    return _back(uv[:, 0].contiguous(), host), _back(uv[:, 1].contiguous(), host)


def _check_view(view):
    if view != "top":
        raise NotImplementedError("view %r: only the view from the top is built here (the rotations of the other views "
                                  "are pyrocko's)" % (view,))


def mts2amps(mts, projection, beachball_type, grid_resolution=200, mask=True, view="top", wavename="any_P", ctx=None,
             shape=None):
    """-> (amps (ny, nx), x, y): the reference's ``mts2amps`` (seismic.py:1387-1425) for the whole ensemble at once.  Per
    draw the ``beachball_type`` part (``full``, ``deviatoric``, ``dc``) is scaled to ``sqrt(sum m9^2) = sqrt 2`` and
    multiplied with the propagation coefficients of ``wavename`` (``any_P``, ``any_SV``, ``any_SH``) at every pixel of the
    unit disc; ``mask``: a positive amplitude counts 1, anything else 0.  ``amps`` is the mean over the draws, NaN outside
    the disc.  With ``mask`` the counts are integers: the result does not depend on the launch (``shape``: None, "wide",
    "narrow").  Without, every pixel adds its draws in ascending order.  A non-finite or all-zero row raises ``ValueError``
    naming it (numpy would spread NaN over the grid)."""
    _check_view(view)
    p = _mt_type(beachball_type)
    mb.check_shape(shape)
    rw, pix, x, y = focal_sphere(grid_resolution, projection, wavename)
    ctx, X, host = _on_device(mts, ctx)
    unit = mb.mt_decompose(ctx, X, want=("unit",))["unit"][:, p:p + 1, :].contiguous()
    res = int(grid_resolution)
    amps = mb.fuzzy_amps(ctx, unit, rw, pix, res, res, mask=mask, shape=shape)[0]
    if host:
        return amps.cpu().numpy(), x.copy(), y.copy()
    return amps, upload(x, amps.device), upload(y, amps.device)


class DecompositionAmps(object):
    """what ``fuzzy_mt_decomposition`` draws and annotates per part, in the order ``names``: ``amps`` (5, ny, nx);
    ``ratio_mean``, ``ratio_spread`` (max - min) (5,); ``ratio_percent`` (5, 2), the (2.5, 97.5) percentiles of
    ``ratios * 100``; ``x``, ``y`` the pixel coordinates"""
    names = PART_NAMES

    def __init__(self, amps, x, y, ratio_mean, ratio_spread, ratio_percent):
        self.amps, self.x, self.y = amps, x, y
        self.ratio_mean, self.ratio_spread, self.ratio_percent = ratio_mean, ratio_spread, ratio_percent


def decomposition_amps(mts, grid_resolution=400, projection="lambert", ctx=None):
    """the five fuzzy beachballs of ``fuzzy_mt_decomposition`` (seismic.py:1738-1786) from ONE decomposition launch and ONE
    count launch, and the numbers it annotates (:1766-1770) through ``marginals.percentiles`` -> ``DecompositionAmps``"""
    from . import marginals
    rw, pix, x, y = focal_sphere(grid_resolution, projection, "any_P")
    ctx, X, host = _on_device(mts, ctx)
    r = mb.mt_decompose(ctx, X, want=("ratios", "unit"))
    res = int(grid_resolution)
    amps = mb.fuzzy_amps(ctx, r["unit"], rw, pix, res, res, mask=True)
    qu = marginals.percentiles(r["ratios"] * 100.0, [2.5, 97.5])
    ext = marginals.percentiles(r["ratios"], [0.0, 100.0])
    mean, spread = r["ratios"].mean(0), ext[:, 1] - ext[:, 0]
    if host:
        return DecompositionAmps(amps.cpu().numpy(), x.copy(), y.copy(), mean.cpu().numpy(), spread.cpu().numpy(), qu.cpu().numpy())
    return DecompositionAmps(amps, upload(x, amps.device), upload(y, amps.device), mean, spread, qu)
