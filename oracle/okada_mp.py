"""
TEST INFRASTRUCTURE ONLY -- multi-precision half-space displacements (mpmath).

The float64 oracle (okada_oracle.py) restates the same formulas as the kernel, in the same number
format: a formulation that is ill-conditioned is ill-conditioned in both.  This file evaluates
Okada (1985) eqs (25)-(30) and Mogi (1958) at DPS >= 50 decimal digits, so that its rounded result
is the value of the formulas themselves:

  * the general-dip expressions are used for EVERY dip, however close to vertical -- their
    cancellation costs about 2*log10(1/|cos dip|) digits, 22 of the 60 at 90 - 1e-9 degrees;
  * the vertical expressions (Okada's case cos(dip) = 0) only where the dip is 90 degrees exactly.
    tests/test_okada_mp.py checks that the two meet: the result at 90 - 1e-9 and the one at 90
    differ by no more than 1e-9 * slip.

Okada's rules for the removable singularities are kept (p. 1148): q = 0 -> the arc tangent of
xi*eta/(q*R) is 0; xi = 0 -> I5 = 0.  A point with R + eta = 0 is refused: the fixture holds generic
points only.  Conventions of the rectangular source are those of okada_oracle.rect_source (anchor
at the centre of the top edge, opening_fraction, km / deg / m).

build_rows() draws the inputs of tests/golden/okada_mp.npz; oracle/gen_golden.py evaluates them.
"""
import numpy as np

DPS = 60

# columns of one fixture row
COLUMNS = ("east_shift", "north_shift", "depth", "strike", "dip", "rake", "length", "width", "slip",
           "opening_fraction", "nu", "east", "north")

# the dip ladder of the fixture [deg]: towards vertical, through it, and both sides of the |cos(dip)| = 1e-7 =
# cos(90 - 5.73e-6 deg) up to which kernel and float64 oracle evaluate a source as vertical
# (okada_oracle.VERTICAL_COS): 5.7e-6 deg from vertical is inside, 5.8e-6 deg outside
LADDER_DIPS = (89.0, 89.9, 89.99, 89.999, 89.9995, 89.9999, 89.99999, 90.0 - 5.8e-6, 90.0 - 5.7e-6, 89.999999,
               90.0 - 1e-9, 90.0, 90.0 + 1e-7, 90.0 + 5.7e-6, 90.0 + 5.8e-6, 90.0005, 90.001)


def _mp():
    import mpmath
    return mpmath


def _sincos_deg(mp, deg):
    """(sin, cos) of an angle in degrees; exact at the multiples of 90"""
    d = mp.mpf(deg)
    r = d % 360
    for k, sc in ((0, (0, 1)), (90, (1, 0)), (180, (0, -1)), (270, (-1, 0))):
        if r == k:
            return mp.mpf(sc[0]), mp.mpf(sc[1])
    a = d * mp.pi / 180
    return mp.sin(a), mp.cos(a)


def _corner(mp, xi, eta, q, sd, cd, a):
    """the strike-slip, dip-slip and tensile corner terms f(xi, eta) of eqs (25)-(27)"""
    R = mp.sqrt(xi * xi + eta * eta + q * q)
    yt = eta * cd + q * sd
    dt = eta * sd - q * cd
    X = mp.sqrt(xi * xi + q * q)
    Re, Rd, Rx = R + eta, R + dt, R + xi
    if Re == 0 or Rd == 0 or Rx == 0:
        raise ValueError("singular point (R + eta, R + d~ or R + xi vanishes)")
    lnRe = mp.log(Re)
    if cd != 0:
        I5 = 0 if xi == 0 else a * 2 / cd * mp.atan((eta * (X + q * cd) + X * (R + X) * sd) / (xi * (R + X) * cd))
        I4 = a / cd * (mp.log(Rd) - sd * lnRe)
        I3 = a * (yt / (cd * Rd) - lnRe) + sd / cd * I4
        I1 = a * (-xi / (cd * Rd)) - sd / cd * I5
    else:
        I5 = -a * xi * sd / Rd
        I4 = -a * q / Rd
        I3 = a / 2 * (eta / Rd + yt * q / (Rd * Rd) - lnRe)
        I1 = -a / 2 * xi * q / (Rd * Rd)
    I2 = a * (-lnRe) - I3
    at = 0 if q == 0 else mp.atan(xi * eta / (q * R))
    qRe, qRx = q / (R * Re), q / (R * Rx)
    ss = (xi * qRe + at + I1 * sd, yt * qRe + q * cd / Re + I2 * sd, dt * qRe + q * sd / Re + I4 * sd)
    ds = (q / R - I3 * sd * cd, yt * qRx + cd * at - I1 * sd * cd, dt * qRx + sd * at - I5 * sd * cd)
    tf = (q * qRe - I3 * sd * sd, -dt * qRx - sd * (xi * qRe - at) - I1 * sd * sd,
          yt * qRx + cd * (xi * qRe - at) - I5 * sd * sd)
    return ss, ds, tf


def okada85_local(x, y, d, dip_deg, L, W, U1, U2, U3, nu=0.25, dps=DPS):
    """Okada's own frame (see okada_oracle.okada85_local), one point -> (ux, uy, uz) as mpf"""
    mp = _mp()
    with mp.workdps(dps):
        x, y, d, L, W, nu = [mp.mpf(v) for v in (x, y, d, L, W, nu)]
        sd, cd = _sincos_deg(mp, dip_deg)
        return _local(mp, x, y, d, sd, cd, L, W, mp.mpf(U1), mp.mpf(U2), mp.mpf(U3), nu)


def _local(mp, x, y, d, sd, cd, L, W, U1, U2, U3, nu):
    p = y * cd + d * sd
    q = y * sd - d * cd
    a = 1 - 2 * nu
    tot = [[mp.mpf(0)] * 3 for _ in range(3)]
    for sg, xi, eta in ((1, x, p), (-1, x, p - W), (-1, x - L, p), (1, x - L, p - W)):
        terms = _corner(mp, xi, eta, q, sd, cd, a)
        for t in range(3):
            tot[t] = [tot[t][k] + sg * terms[t][k] for k in range(3)]
    c = 1 / (2 * mp.pi)
    return tuple(-U1 * c * tot[0][k] - U2 * c * tot[1][k] + U3 * c * tot[2][k] for k in range(3))


def rect_source(east, north, east_shift, north_shift, depth, strike, dip, rake, length, width, slip,
                opening_fraction=0.0, nu=0.25, dps=DPS):
    """okada_oracle.rect_source at one point (east, north) -> (ue, un, uz_up) as mpf"""
    mp = _mp()
    with mp.workdps(dps):
        e, n, es, ns, depth, L, W, slip, f, nu = [mp.mpf(v) for v in (east, north, east_shift, north_shift, depth,
                                                                      length, width, slip, opening_fraction, nu)]
        ex, nx = _sincos_deg(mp, strike)
        ey, ny = nx, -ex
        sd, cd = _sincos_deg(mp, dip)
        sr, cr = _sincos_deg(mp, rake)
        d_bot = depth + W * sd
        oe = es - L * ex / 2 + W * cd * ey
        on = ns - L * nx / 2 + W * cd * ny
        de, dn = e - oe, n - on
        x = de * ex + dn * nx
        y = -(de * ey + dn * ny)
        shear = slip * (1 - abs(f))
        ux, uy, uz = _local(mp, x, y, d_bot, sd, cd, L, W, shear * cr, shear * sr, slip * f, nu)
        return ux * ex - uy * ey, ux * nx - uy * ny, +uz


def mogi(east, north, east_shift, north_shift, depth, volume_change, nu=0.25, dps=DPS):
    """okada_oracle.mogi at one point -> (ue, un, uz_up) as mpf"""
    mp = _mp()
    with mp.workdps(dps):
        de = (mp.mpf(east) - mp.mpf(east_shift)) * 1000
        dn = (mp.mpf(north) - mp.mpf(north_shift)) * 1000
        d = mp.mpf(depth) * 1000
        R2 = de * de + dn * dn + d * d
        c = (1 - mp.mpf(nu)) / mp.pi * mp.mpf(volume_change) / (R2 * mp.sqrt(R2))
        return c * de, c * dn, c * d


def evaluate_row(kind, row, dps=DPS):
    """one fixture row (COLUMNS) -> (ue, un, uz) rounded to float64; kind 0 rectangular, 1 Mogi"""
    es, ns, depth, strike, dip, rake, L, W, slip, f, nu, e, n = [float(v) for v in row]
    if int(kind) == 1:
        u = mogi(e, n, es, ns, depth, slip, nu, dps)
    else:
        u = rect_source(e, n, es, ns, depth, strike, dip, rake, L, W, slip, f, nu, dps)
    return tuple(float(v) for v in u)


# ------------------------------------------------------------------------------------------------- fixture inputs
def _box_source(rng):
    """one source from the prior box of tests/test_geometry.py (rake and opening fraction free)"""
    return dict(east_shift=rng.uniform(-5, 5), north_shift=rng.uniform(-5, 5), depth=rng.uniform(0.5, 9.0),
                strike=rng.uniform(0, 360), dip=rng.uniform(5, 85), rake=rng.uniform(-180, 180),
                length=rng.uniform(0.5, 10), width=rng.uniform(0.5, 8), slip=rng.uniform(0.01, 1.0),
                opening_fraction=rng.uniform(-1, 1), nu=0.25)


def _row(src, east, north):
    return [src[k] for k in COLUMNS[:11]] + [east, north]


def _local_to_map(src, x, y):
    """the map position (east, north) of the point (x, y) of Okada's frame (float64, as rect_source)"""
    st, dp = np.deg2rad(src["strike"]), np.deg2rad(src["dip"])
    ex, nx = np.sin(st), np.cos(st)
    ey, ny = np.cos(st), -np.sin(st)
    oe = src["east_shift"] - 0.5 * src["length"] * ex + src["width"] * np.cos(dp) * ey
    on = src["north_shift"] - 0.5 * src["length"] * nx + src["width"] * np.cos(dp) * ny
    return oe + x * ex - y * ey, on + x * nx - y * ny


def build_rows(seed=19850801):
    """-> (group names [nrow], kind [nrow], rows [nrow, 13]); every group holds one nu and one kind, so that a group
    is one launch of the batched displacement kernel"""
    rng = np.random.default_rng(seed)
    groups, kinds, rows = [], [], []

    def add(group, src, east, north, kind=0):
        groups.append(group)
        kinds.append(kind)
        rows.append(_row(src, float(east), float(north)))

    for _ in range(64):
        add("prior_box", _box_source(rng), rng.uniform(-15, 15), rng.uniform(-15, 15))
    for _ in range(16):                                 # another Poisson ratio (one launch holds one)
        add("prior_box_nu", dict(_box_source(rng), nu=0.31), rng.uniform(-15, 15), rng.uniform(-15, 15))
    for dist in (100.0, 1000.0):
        for _ in range(12):
            az = rng.uniform(0, 2 * np.pi)
            add("far_%d" % dist, _box_source(rng), dist * np.sin(az), dist * np.cos(az))
    for depth in (0.0, 1e-9):
        for _ in range(8):
            add("surface_breaking", dict(_box_source(rng), depth=depth), rng.uniform(-15, 15), rng.uniform(-15, 15))
    offsets = (1e-14, 1e-12, 1e-10, 1e-8, 1e-6)
    for k in range(20):                                 # next to the q = 0 trace of the extended fault plane
        src = _box_source(rng)
        dp = np.deg2rad(src["dip"])
        d_bot = src["depth"] + src["width"] * np.sin(dp)
        y0 = d_bot * np.cos(dp) / np.sin(dp)
        off = offsets[k % 5] * (1 if k % 2 else -1)
        add("near_q0", src, *_local_to_map(src, rng.uniform(-1, 2) * src["length"], y0 + off))
    for k in range(20):                                 # next to the xi = 0 lines through the fault's ends
        src = _box_source(rng)
        off = offsets[k % 5] * (1 if k % 2 else -1)
        add("near_xi0", src, *_local_to_map(src, (src["length"] if k % 4 < 2 else 0.0) + off, rng.uniform(-12, 12)))
    for dip in (1e-3, 0.0):
        for _ in range(8):
            add("dip_flat", dict(_box_source(rng), dip=dip), rng.uniform(-15, 15), rng.uniform(-15, 15))
    for dip in (95.0, 90.1):
        for _ in range(8):
            add("dip_over", dict(_box_source(rng), dip=dip), rng.uniform(-15, 15), rng.uniform(-15, 15))
    for _ in range(16):
        src = dict.fromkeys(COLUMNS[:11], 0.0)
        src.update(east_shift=rng.uniform(-5, 5), north_shift=rng.uniform(-5, 5), depth=rng.uniform(0.5, 9.0),
                   slip=rng.uniform(1e5, 1e7), nu=0.25)
        add("mogi", src, rng.uniform(-15, 15), rng.uniform(-15, 15), kind=1)
    ladder = [(_box_source(rng), rng.uniform(-15, 15), rng.uniform(-15, 15)) for _ in range(6)]
    for dip in LADDER_DIPS:                             # the same six sources and points at every dip
        for src, e, n in ladder:
            add("dip_ladder", dict(src, dip=dip), e, n)
    return np.array(groups), np.array(kinds, dtype=np.int32), np.array(rows, dtype=np.float64)


def evaluate_rows(kinds, rows, dps=DPS):
    return np.array([evaluate_row(k, r, dps) for k, r in zip(kinds, rows)], dtype=np.float64)
