"""numpy restatement of the Euler-pole arithmetic the device does (csrc/corrections.hip states the same order):

    rlat = pole_lat * d2r ; rlon = pole_lon * d2r ; e2 = 2 f - f * f
    N  = a / sqrt(1 - e2 * (sin(rlat) * sin(rlat)))
    px = ((N * cos(rlat)) * cos(rlon)) / r ; py = ((N * cos(rlat)) * sin(rlon)) / r ; pz = ((N * (1 - e2)) * sin(rlat)) / r
    w  = ((omega * 1e-6) * d2r) * r ; coef = (w * px, w * py, w * pz)

and of the coupling lines ffi/fault.py:1497, 1514-1517.  Test infrastructure: written from the formulas, it imports
nothing of beat_amd."""
import numpy as np

D2R = np.pi / 180.0
U = 2.0 ** -53


def coefficients(pole_lat, pole_lon, omega, earth):
    r, a, f = [float(v) for v in earth]
    pole_lat, pole_lon, omega = [np.asarray(v, dtype=np.float64) for v in (pole_lat, pole_lon, omega)]
    rlat, rlon = pole_lat * D2R, pole_lon * D2R
    e2 = 2.0 * f - f * f
    sl, cl, so, co = np.sin(rlat), np.cos(rlat), np.sin(rlon), np.cos(rlon)
    N = a / np.sqrt(1.0 - e2 * (sl * sl))
    px, py, pz = ((N * cl) * co) / r, ((N * cl) * so) / r, ((N * (1.0 - e2)) * sl) / r
    w = ((omega * 1e-6) * D2R) * r
    return np.stack([w * px, w * py, w * pz], axis=-1)


def omega_prime(omega, earth):
    return np.abs(np.asarray(omega, dtype=np.float64) * 1e-6 * D2R * float(earth[0]))


def bound(omega, earth, los):
    """16 * 2^-53 * |w'| * |l_i|_1 per observation"""
    return 16.0 * U * omega_prime(omega, earth) * np.abs(los).sum(axis=1)


def linear(B, coef):
    """the device's sum order: (B0 c0 + B1 c1) + B2 c2"""
    return (B[:, 0] * coef[0] + B[:, 1] * coef[1]) + B[:, 2] * coef[2]


def euler_slips(Bp, coef):
    return np.abs(linear(Bp, coef))


def backslip2coupling(backslips, es):
    with np.errstate(divide="ignore", invalid="ignore"):
        coupling = backslips / es
        coupling[coupling < 0.0] = 0.0
        coupling[coupling > 1.0] = 1.0
        return coupling * 100
