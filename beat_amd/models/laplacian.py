"""Smoothing operators of a finite fault with the reference's names (beat/models/laplacian.py:180-298 and
FaultGeometry.get_smoothing_operator, beat/ffi/fault.py:790-828).  Host functions: what a user hands to ``FFIProblem``
as the dense Laplacian ``L`` (its prior keeps ``log_determinant(L.T * L)`` elementwise, laplacian.py:58).  The
correlated operator also runs on the device (``Context.smoothing_correlated``, csrc/resolution.hip) for the
resolution-based discretization, which never copies it to the host."""
import numpy as np

from ..synthetic import smoothing_operator_nearest_neighbor
from ..utility import distances


class InvalidDiscretizationError(Exception):
    """beat/ffi/fault.py: the operator asked for does not exist for this discretization"""


def get_smoothing_operator_nearest_neighbor(n_patch_strike, n_patch_dip, patch_size_strike, patch_size_dip):
    """laplacian.py:209-258: second-order Laplacian between neighbouring patches of ONE flat subfault [km]; the
    arithmetic is ``beat_amd.synthetic.smoothing_operator_nearest_neighbor``'s"""
    return smoothing_operator_nearest_neighbor(n_patch_strike, n_patch_dip, patch_size_strike, patch_size_dip)


def get_smoothing_operator_correlated(patches_coords, correlation_function="gaussian"):
    """laplacian.py:261-298: patches_coords (npatches, 3) [km] -> (npatches, npatches), off-diagonal 1 / d^2
    ("gaussian") or 1 / exp(d) ("exponential") of the inter-patch distance d, diagonal minus the column sum.

    Summation order: column j adds the rows i = 0, 1, ... in ascending order from zero.  That is the order of numpy's
    ``a.sum(0)`` on a C-contiguous array at every npatches (numpy's pairwise blocks of 128 serve reductions along the
    contiguous axis only, so there is no npatches from which the two differ); the device kernel k_smooth_corr_diag
    adds in the same order, so both give the same bits wherever sqrt, the division and exp round alike."""
    patches_coords = np.ascontiguousarray(patches_coords, dtype=np.float64)
    d = distances(patches_coords, patches_coords)
    np.fill_diagonal(d, 1.0)          # (the zero distance of a patch to itself has no inverse)
    if correlation_function == "gaussian":
        a = 1 / np.power(d, 2)
    elif correlation_function == "exponential":
        a = 1 / np.exp(d)
    else:
        raise ValueError('Resolution based discretization does not support "nearest_neighbor" correlation function!')
    np.fill_diagonal(a, 0.0)
    np.fill_diagonal(a, -a.sum(0))
    return a


def get_smoothing_operator(subfault_discretizations=None, patches_coords=None, correlation_function="nearest_neighbor"):
    """FaultGeometry.get_smoothing_operator (fault.py:790-828) for a fault of several subfaults.

    "nearest_neighbor": ``subfault_discretizations`` is one (n_patch_strike, n_patch_dip, patch_size_strike,
    patch_size_dip) per subfault of a UNIFORM discretization; the operators are put on the block diagonal (no
    smoothing across subfaults).  None -- a fault that is not uniformly discretized -- raises the reference's
    InvalidDiscretizationError.  Any other correlation function: the correlated operator of the event-relative patch
    centres ``patches_coords`` (npatches, 3) [km]."""
    if correlation_function == "nearest_neighbor":
        if subfault_discretizations is None:
            raise InvalidDiscretizationError(
                "Nearest neighbor correlation Laplacian is only "
                'available for "uniform" discretization! Please change'
                " either correlation_function or the discretization.")
        Ls = [get_smoothing_operator_nearest_neighbor(*sd) for sd in subfault_discretizations]
        n = sum(L.shape[0] for L in Ls)
        out = np.zeros((n, n))
        o = 0
        for L in Ls:
            out[o:o + L.shape[0], o:o + L.shape[0]] = L
            o += L.shape[0]
        return out
    return get_smoothing_operator_correlated(patches_coords, correlation_function)
