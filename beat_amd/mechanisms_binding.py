"""
The Python binding of the mechanism-ensemble entries of ``libbeat_amd.so`` (``beatamd_mt_decompose``,
``beatamd_fuzzy_amps``; csrc/mechanisms.hip, csrc/mechanism.hpp) as functions of a ``Context`` (``ctx``, beat_amd.engine).
The argument rules that need no device are checked here ahead of the call (the library checks them again); results live on
the side of the first array argument.  ``beat_amd.mechanisms`` is the public interface on top.
"""
import numpy as np

from . import _lib
from ._lib import check, ptr
from ._marshal import as_input, checked, on_side

MAX_DRAWS = 1 << 24            # csrc/kernels.hpp MC_MAX_N
MAX_RESOLUTION = 4096          # csrc/kernels.hpp MC_MAX_RES
CHUNK = 512                    # csrc/kernels.hpp MC_CHUNK: draws a workgroup counts before its atomics
PART_NAMES = ("iso", "dc", "clvd", "dev", "full")      # the order of standard_decomposition
NPART = len(PART_NAMES)
KIND_M6, KIND_SDR = 0, 1
OUTPUTS = (("evals", (3,)), ("evecs", (3, 3)), ("moments", (NPART,)), ("ratios", (NPART,)), ("parts", (NPART, 6)),
           ("unit", (NPART, 6)), ("uv", (2,)))          # in the order of the C entry
SHAPES = {None: 0, "wide": 1, "narrow": 2}              # the launch shapes of the count kernel


def check_shape(shape):
    if shape not in SHAPES:
        raise ValueError("unknown launch shape %r (None, 'wide' or 'narrow')" % (shape,))
    return SHAPES[shape]


def check_mts(mts):
    """mts as the library reads them: a contiguous float64 (n, 6) array of (mnn, mee, mdd, mne, mnd, med) or (n, 3) of
    strike, dip, rake in degrees, n >= 1 -> (mts, n, kind)"""
    X = as_input(mts)
    if len(X.shape) != 2 or X.shape[0] < 1 or X.shape[1] not in (3, 6):
        raise ValueError("mts must be (n, 6) moment tensors or (n, 3) strike, dip, rake with n >= 1, got %s"
                         % (tuple(X.shape),))
    if X.shape[0] > MAX_DRAWS:
        raise ValueError("%d draws, at most 2^24 in one call" % X.shape[0])
    return X, int(X.shape[0]), (KIND_M6 if X.shape[1] == 6 else KIND_SDR)


def check_resolution(grid_resolution):
    if np.ndim(grid_resolution) != 0 or int(grid_resolution) != grid_resolution or not 1 <= grid_resolution <= MAX_RESOLUTION:
        raise ValueError("grid_resolution must be an integer in [1, %d], got %r" % (MAX_RESOLUTION, grid_resolution))
    return int(grid_resolution)


def _refused(rc):
    """ValueError with the library's message, which names the row, for BEATAMD_ENAN; the usual mapping otherwise"""
    if rc == _lib.ENAN:
        raise ValueError(_lib.load().beatamd_last_error().decode("utf-8", "replace"))
    check(rc)


def mt_decompose(ctx, mts, want=None):
    """mts (n, 6) or (n, 3) -> dict of the arrays named in ``want`` (None: all of ``OUTPUTS``), each (n,) + its shape, on
    the side of ``mts``.  ValueError names the first row that is non-finite or, for tensors, all zero."""
    ctx._adopt_stream(mts)
    X, n, kind = check_mts(mts)
    names = [k for k, _ in OUTPUTS]
    want = names if want is None else list(want)
    for k in want:
        if k not in names:
            raise ValueError("mt_decompose: unknown output %r (%s)" % (k, ", ".join(names)))
    out = dict((k, checked(None, X, (n,) + tail, np.float64, k, of="mts")) for k, tail in OUTPUTS if k in want)
    _refused(ctx._lib.beatamd_mt_decompose(ctx._h, n, kind, ptr(X), *[ptr(out.get(k)) for k in names]))
    return out


def fuzzy_amps(ctx, unit, rw, pixel_index, ny, nx, mask=True, shape=None):
    """unit (n, P, 6), rw (6, npix), pixel_index (npix,) cells of the (ny, nx) grid -> amps (P, ny, nx) on the side of
    ``unit``: NaN outside the pixels, the fraction of draws with a positive amplitude (mask) or the mean amplitude inside"""
    ctx._adopt_stream(unit)
    unit = as_input(unit)
    if len(unit.shape) != 3 or unit.shape[0] < 1 or unit.shape[1] < 1 or unit.shape[2] != 6:
        raise ValueError("unit must be (n, P, 6) with n, P >= 1, got %s" % (tuple(unit.shape),))
    n, P = int(unit.shape[0]), int(unit.shape[1])
    if n > MAX_DRAWS:
        raise ValueError("%d draws, at most 2^24 in one call" % n)
    ny, nx = check_resolution(ny), check_resolution(nx)
    shape = check_shape(shape)
    if len(rw.shape) != 2 or rw.shape[0] != 6:
        raise ValueError("rw must be (6, npix), got %s" % (tuple(rw.shape),))
    npix = int(rw.shape[1])
    if npix > ny * nx:
        raise ValueError("%d pixels in a grid of %d x %d" % (npix, ny, nx))
    rw = on_side(rw, unit, np.float64, (6, npix), "rw")
    pixel_index = as_input(pixel_index, np.int64)     # (either side: the library checks it against the grid on the host)
    if tuple(pixel_index.shape) != (npix,):
        raise ValueError("pixel_index must be (%d,), got %s" % (npix, tuple(pixel_index.shape)))
    amps = checked(None, unit, (P, ny, nx), np.float64, "amps", of="unit")
    check(ctx._lib.beatamd_fuzzy_amps(ctx._h, n, P, ptr(unit), npix, ptr(rw), ptr(pixel_index), ny, nx, int(bool(mask)), shape,
                                      ptr(amps)))
    return amps
