"""Host helpers with the reference's names (beat/utility.py)."""
import numpy as np


def positions2idxs(positions, cell_size, min_pos=0.0, backend=np, dtype="int16"):
    """utility.py:1542-1558 (round-half-even, int16)"""
    return backend.round((positions - min_pos - (cell_size / 2.0)) / cell_size).astype(dtype)


def ensure_cov_psd(cov):
    """utility.py:1034-1056"""
    try:
        np.linalg.cholesky(cov)
        return cov
    except np.linalg.LinAlgError:
        return repair_covariance(cov)


def repair_covariance(x, epsilon=np.finfo(np.float64).eps):
    """utility.py:1113-1138: clip the eigenvalues at epsilon and transform back"""
    eigval, eigvec = np.linalg.eigh(x)
    val = np.maximum(eigval, epsilon)
    return eigvec.dot(np.diag(val)).dot(eigvec.T)


def nextpow2(n):
    """pyrocko.trace.nextpow2: the transform length heart.fft_transforms pads a trace of n samples to.  RESTATED FROM
    MEMORY (pyrocko is not in the tree): ``2 ** ceil(log2(n))``"""
    return int(2 ** int(np.ceil(np.log2(n))))


def get_valid_spectrum_data(deltaf, taper_frequencies=[0, 1.0]):
    """utility.py:1604-1610: (lower_idx, upper_idx) of the valid frequency range of a spectrum sampled at deltaf"""
    lower_f, upper_f = taper_frequencies
    lower_idx = int(np.floor(lower_f / deltaf))
    upper_idx = int(np.ceil(upper_f / deltaf))
    return lower_idx, upper_idx


def get_data_radiant(data):
    """utility.py:1611-1619: angle of the data extent, data (n, 2)"""
    return np.arctan2(data[:, 1].max() - data[:, 1].min(), data[:, 0].max() - data[:, 0].min())


def find_elbow(data, theta=None, rotate_left=False):
    """utility.py:1622-1655: index of the point closest to the turning point of data (n, 2) after rotating it by
    theta (default: get_data_radiant); -> (index, rotated_data)"""
    if theta is None:
        theta = get_data_radiant(data)
    if rotate_left:
        theta = 2 * np.pi - theta
    co, si = np.cos(theta), np.sin(theta)
    rotation_matrix = np.array(((co, -si), (si, co)))
    rotated_data = data.dot(rotation_matrix)
    return rotated_data[:, 1].argmin(), rotated_data


def distances(points, ref_points):
    """utility.py:1695-1723: Cartesian distances (n_points, n_ref_points) of points (n, d) to ref_points (m, d); the d
    squares are summed in axis order"""
    nref_points = ref_points.shape[0]
    ndim = points.shape[1]
    ndim_ref = ref_points.shape[1]
    if ndim != ndim_ref:
        raise TypeError("Coordinates to calculate differences must have the same number "
                        "of dimensions! Given dimensions are {} and {}".format(ndim, ndim_ref))
    points_rep = np.tile(points, nref_points).reshape(points.shape[0], nref_points, ndim)
    return np.sqrt(np.power(points_rep - ref_points, 2).sum(axis=2))


def normalized_resolution_spread(resolution, nparams):
    """ffi/fault.py:2047-2054 (Atzori et al. 2019): between 0 and 1, the closer to zero the better resolved"""
    return np.linalg.norm(resolution - np.eye(nparams)) / nparams


def running_window_rms(data, window_size, mode="valid"):
    """utility.py:1141-1161"""
    data2 = np.power(data, 2)
    window = np.ones(window_size) / float(window_size)
    return np.sqrt(np.convolve(data2, window, mode))
