"""numpy restatement of the reference's dataset corrections (test infrastructure, like philox_ref.py):

  beat/heart.py:4494-4512            get_ramp_displacement
  beat/heart.py:4441-4491            velocities_from_strain_rate_tensor (on local norths / easts [m])
  beat/models/corrections.py:198-205 mask and line-of-sight projection of the strain-rate velocities
  beat/models/geodetic.py:411-427    apply_corrections: residuals[i] -= correction, in list order

pinned to the reference's own numbers in tests/golden/geo_corrections.npz by tests/test_corrections_host.py."""
import numpy as np

km = 1000.0
nanostrain = 1e-9


def ramp(north_shifts, east_shifts, azimuth_ramp, range_ramp, offset):
    locx, locy = east_shifts / km, north_shifts / km
    return locy * azimuth_ramp + locx * range_ramp + offset


def strain_rate(norths, easts, los, mask, exx, eyy, exy, rotation):
    D = np.array([[float(exx), 0.5 * float(exy + rotation)],
                  [0.5 * float(exy - rotation), float(eyy)]]) * nanostrain
    v_x, v_y = D.dot(np.atleast_2d(np.vstack([norths, easts])))
    v = np.zeros((norths.size, 3))
    v[:, 0] = v_x
    v[:, 1] = v_y
    if mask.any():
        v[mask, :] = 0.0
    return (v * los).sum(axis=1)


def apply_corrections(residuals, corrections):
    """residuals: one array per dataset; corrections: one list of correction arrays per dataset"""
    out = []
    for res, corrs in zip(residuals, corrections):
        res = np.array(res, dtype=np.float64)
        for c in corrs:
            res -= c
        out.append(res)
    return out


def contract(B, coefs):
    """the arithmetic the library documents for one term: ((B0*c0 + B1*c1) + B2*c2) + B3*c3, plain products
    and sums from left to right"""
    corr = B[:, 0] * coefs[0]
    for k in range(1, B.shape[1]):
        corr = corr + B[:, k] * coefs[k]
    return corr


def strain_bound(B, coefs):
    """|folded columns - reference| <= 16 * 2^-53 * sum_k |B[:, k] * coef_k|: both sides are sums of at most four
    products of once-rounded factors"""
    return 16 * 2.0 ** -53 * np.abs(B * np.asarray(coefs)[None, :]).sum(axis=1)
