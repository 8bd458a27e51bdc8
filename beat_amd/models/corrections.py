"""
Hierarchical corrections of geodetic datasets -- the counterpart of

  beat/models/corrections.py:46-87      RampCorrection       (orbital ramp of a SAR scene)
  beat/models/corrections.py:90-140     EulerPoleCorrection  (rigid rotation of a GNSS network about an Euler pole)
  beat/models/corrections.py:143-205    StrainRateCorrection (strain-rate tensor of a GNSS network)
  beat/config.py:802-909                the configuration holders, the hierarchical names, the order of the terms
  beat/models/geodetic.py:411-427       GeodeticComposite.apply_corrections (residuals[i] -= correction)

The reference subtracts every enabled correction of a dataset from its weighted residual before
``multivariate_normal_chol`` (geodetic.py:1076-1077); the coefficients are sampled with everything else.  Here
every correction is a linear term ``sum_k B[:, k] * coef_k`` over at most four constant basis columns
(``basis()``), uploaded once and subtracted on the device in the kernel that forms the residual
(``beatamd_ffi_model_add_geodetic_corrections``).  ``get_displacements(hierarchicals, point)`` is the host
(numpy) evaluation post-processing calls, the reference's ``point`` branch.

The Euler-pole correction is such a linear term too, over three columns, but its coefficients are not entries of q:
they are ``omega' * p``, a function of the three sampled variables (pole_lat, pole_lon, omega) that the device derives
per chain (``k_pole_coef``) in front of every kernel that subtracts corrections (``EulerPoleCorrection``; kind 1 of
``beatamd_ffi_model_add_geodetic_corrections_kinds``).  The earth's radius, equatorial radius and oblateness behind
``geodetic_to_ecef`` are data (``EarthModel``), handed to the device with the term.
"""
import numpy as np

km = 1000.0
nanostrain = 1e-9
d2r = np.pi / 180.0
MAX_COLUMNS = 4
KIND_LINEAR, KIND_EULER_POLE = 0, 1


def _point_values(point, names, suffixes):
    """{suffix: value} of the correction's variables; KeyError if one is missing"""
    return dict((s, point[n]) for n, s in zip(names, suffixes))


class CorrectionConfig(object):
    """config.py:802-825: which datasets a correction acts on, and whether it is enabled"""
    feature = "Correction"
    _suffixes = ("",)

    def __init__(self, dataset_names=(), enabled=False):
        self.dataset_names = list(dataset_names)
        self.enabled = bool(enabled)

    def get_suffixes(self):
        return list(self._suffixes)

    def check_consistency(self):
        if self.enabled and not self.dataset_names:
            raise AttributeError("%s correction is enabled but names no dataset" % self.feature)


class RampConfig(CorrectionConfig):
    """config.py:872-892"""
    feature = "Ramps"
    _suffixes = ("azimuth_ramp", "range_ramp", "offset")

    def get_hierarchical_names(self, name, number=0):
        # config.py:881-886: "<dataset>_<suffix>", only for the datasets the ramp is configured for
        if name not in self.dataset_names:
            return []
        return ["%s_%s" % (name, s) for s in self.get_suffixes()]

    def init_correction(self):
        self.check_consistency()
        return RampCorrection(self)


class GNSSCorrectionConfig(CorrectionConfig):
    """config.py:828-837: a correction of a GNSS network -- station lists, names "<number>_<suffix>" """

    def __init__(self, dataset_names=(), enabled=False, station_blacklist=(), station_whitelist=()):
        CorrectionConfig.__init__(self, dataset_names, enabled)
        self.station_blacklist = list(station_blacklist)
        self.station_whitelist = list(station_whitelist)

    def get_hierarchical_names(self, name=None, number=0):
        # config.py:836-837: "<number>_<suffix>"
        return ["%s_%s" % (number, s) for s in self.get_suffixes()]


class StrainRateConfig(GNSSCorrectionConfig):
    """config.py:856-869"""
    feature = "Strain Rate"
    _suffixes = ("exx", "eyy", "exy", "rotation")

    def init_correction(self):
        self.check_consistency()
        return StrainRateCorrection(self)


class EulerPoleConfig(GNSSCorrectionConfig):
    """config.py:840-853; pole_lat, pole_lon [deg], omega [deg / Myr]"""
    feature = "Euler Pole"
    _suffixes = ("pole_lat", "pole_lon", "omega")

    def init_correction(self):
        self.check_consistency()
        return EulerPoleCorrection(self)


class EarthModel(object):
    """The three constants behind ``heart.velocities_from_pole`` (heart.py:4350, 4379-4383): ``radius`` [m] scales
    the ECEF vectors and the rotation rate, ``equator_radius`` [m] and ``oblateness`` are the ellipsoid of
    ``orthodrome.geodetic_to_ecef``.  They are data: the device gets them with every pole term.

    Defaults: pyrocko's ``orthodrome.earthradius``, ``earthradius_equator`` and ``earth_oblateness`` where pyrocko
    imports.  Otherwise 6371.0e3, 6378.14e3 and 1/298.257223563 -- pyrocko's values AS RECALLED: pyrocko was not
    installed where this was written, so nobody has checked the three numbers against it.  Pass your own to be sure."""
    RADIUS, EQUATOR_RADIUS, OBLATENESS = 6371.0e3, 6378.14e3, 1.0 / 298.257223563

    def __init__(self, radius=None, equator_radius=None, oblateness=None):
        if radius is None or equator_radius is None or oblateness is None:
            try:
                from pyrocko import orthodrome
                dflt = (orthodrome.earthradius, orthodrome.earthradius_equator, orthodrome.earth_oblateness)
            except ImportError:
                dflt = (self.RADIUS, self.EQUATOR_RADIUS, self.OBLATENESS)
        self.radius = float(dflt[0] if radius is None else radius)
        self.equator_radius = float(dflt[1] if equator_radius is None else equator_radius)
        self.oblateness = float(dflt[2] if oblateness is None else oblateness)

    @classmethod
    def sphere(cls, radius=None):
        """``earth_shape="sphere"`` of the reference (heart.py:4372-4376): the same formulas with
        equator_radius = radius and oblateness = 0, i.e. unit vectors of geocentric latitude / longitude"""
        r = cls(radius, 1.0, 0.0).radius
        return cls(r, r, 0.0)

    def as_tuple(self):
        return (self.radius, self.equator_radius, self.oblateness)

    def geodetic_to_ecef(self, lat, lon):
        """x, y, z [m] of points on the ellipsoid (altitude 0), the textbook closed form:
        N = a / sqrt(1 - e2 sin(lat)^2), e2 = 2f - f^2; (N cos(lat) cos(lon), N cos(lat) sin(lon), N (1 - e2) sin(lat))"""
        f, a = self.oblateness, self.equator_radius
        e2 = 2.0 * f - f * f
        rlat, rlon = np.asarray(lat, dtype=np.float64) * d2r, np.asarray(lon, dtype=np.float64) * d2r
        sl, cl, so, co = np.sin(rlat), np.cos(rlat), np.sin(rlon), np.cos(rlon)
        N = a / np.sqrt(1.0 - e2 * (sl * sl))
        return (N * cl) * co, (N * cl) * so, (N * (1.0 - e2)) * sl


class Correction(object):
    kind = KIND_LINEAR
    order = 3      # place among a dataset's terms (config.py:904-909 iter_corrections: ramp, Euler poles, strain rates)

    def __init__(self, correction_config):
        self.config = correction_config
        self.correction_names = None

    def get_required_coordinate_names(self):
        raise NotImplementedError()

    def get_point_rvs(self, point):
        return _point_values(point, self.correction_names, self.config.get_suffixes())

    def _values(self, hierarchicals, point):
        """the coefficients by suffix: from ``point``, else (fixed variables) from ``hierarchicals``"""
        if not self.correction_names:
            raise ValueError("Requested correction, but is not setup or configured!")
        try:
            return self.get_point_rvs(point if point else hierarchicals)
        except KeyError:
            if not point or not hierarchicals:
                raise
            return self.get_point_rvs(hierarchicals)

    def basis(self):
        """(n, K) constant columns; the correction is ``sum_k basis[:, k] * coef_k`` with the coefficients in the
        order of ``config.get_suffixes()``"""
        raise NotImplementedError()


class RampCorrection(Correction):
    """corrections.py:46-87 / heart.py:4494-4512: ``locy*azimuth_ramp + locx*range_ramp + offset`` with the local
    coordinates in km"""
    order = 0

    def get_required_coordinate_names(self):
        return ["east_shifts", "north_shifts"]

    def setup_correction(self, locy, locx, los_vector, data_mask, dataset_name, number=0):
        self.east_shifts = np.asarray(locx, dtype=np.float64)
        self.north_shifts = np.asarray(locy, dtype=np.float64)
        self.correction_names = self.config.get_hierarchical_names(name=dataset_name, number=number)

    def get_displacements(self, hierarchicals, point=None):
        v = self._values(hierarchicals, point)
        locx, locy = self.east_shifts / km, self.north_shifts / km
        return locy * v["azimuth_ramp"] + locx * v["range_ramp"] + v["offset"]

    def basis(self):
        locx, locy = self.east_shifts / km, self.north_shifts / km
        return np.stack([locy, locx, np.ones_like(locx)], axis=1)


def reproject_local(lats, lons):
    """norths, easts [m] of geographic points about their midpoint, as heart.py:4481-4482 obtains them: pyrocko's
    ``orthodrome.geographic_midpoint`` and ``latlon_to_ne_numpy`` (no reprojection of our own)"""
    try:
        from pyrocko import orthodrome
    except ImportError:
        raise ImportError(
            "the strain-rate correction needs local coordinates: pyrocko (orthodrome.geographic_midpoint, "
            "latlon_to_ne_numpy) is not installed to reproject lats / lons; pass "
            "local_coordinates=(norths, easts) in metres to setup_correction()")
    lats, lons = np.asarray(lats, dtype=np.float64), np.asarray(lons, dtype=np.float64)
    mid_lat, mid_lon = orthodrome.geographic_midpoint(lats, lons)
    return orthodrome.latlon_to_ne_numpy(mid_lat, mid_lon, lats, lons)


def _station_frame(lat, lon):
    """the local frame of points at lat / lon [deg]: the ECEF components (each (n,)) of the unit vectors north, east
    and DOWN -- the third row of the rotation in heart.velocities_from_pole points to the earth's centre, and the
    reference projects on it as it stands"""
    sin_lat, cos_lat = np.sin(lat * d2r), np.cos(lat * d2r)
    sin_lon, cos_lon = np.sin(lon * d2r), np.cos(lon * d2r)
    north = (-sin_lat * cos_lon, -sin_lat * sin_lon, cos_lat)
    east = (-sin_lon, cos_lon, np.zeros_like(sin_lon))
    down = (-cos_lat * cos_lon, -cos_lat * sin_lon, -sin_lat)
    return north, east, down


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


class EulerPoleCorrection(Correction):
    """corrections.py:90-140 / heart.py:4326-4392: velocities of a rigid rotation about an Euler pole at the stations,
    projected on the line of sight.  With x_i = ecef(lat_i, lon_i, 0) / r_earth, T_i the ECEF -> NEU rotation and l_i
    the line of sight:

        corr_i = l_i . T_i (w' p x x_i) = sum_k B[i, k] coef_k ,   B[i, :] = x_i x (T_i^T l_i) ,   coef = w' p
        p = ecef(pole_lat, pole_lon, 0) / r_earth ,   w' = omega * 1e-6 * (pi / 180) * r_earth

    so the term is linear in three numbers derived from (pole_lat, pole_lon, omega): ``coefficients()`` on the host,
    ``k_pole_coef`` on the device, in ONE order of operations:

        rlat = pole_lat * d2r ; rlon = pole_lon * d2r ; e2 = 2 f - f * f
        N = a / sqrt(1 - e2 * (sin(rlat) * sin(rlat)))
        px = ((N * cos(rlat)) * cos(rlon)) / r ; py = ((N * cos(rlat)) * sin(rlon)) / r
        pz = ((N * (1 - e2)) * sin(rlat)) / r
        w' = ((omega * 1e-6) * d2r) * r ;  coef = (w' * px, w' * py, w' * pz)

    ``get_displacements`` evaluates in the reference's order of steps (cross product, rotation into the local frame,
    line of sight, masked rows zero); it and the linear form lie within 16 * 2^-53 * |w'| * |l_i|_1 of the reference's
    values."""
    kind = KIND_EULER_POLE
    order = 1

    def get_required_coordinate_names(self):
        return ["lons", "lats"]

    def setup_correction(self, locy, locx, los_vector, data_mask, dataset_name, number=0, earth=None):
        """locy / locx: lats / lons [deg] (the reference's arguments); earth: EarthModel (None: the defaults)"""
        self.lats = np.asarray(locy, dtype=np.float64)
        self.lons = np.asarray(locx, dtype=np.float64)
        self.los_vector = np.asarray(los_vector, dtype=np.float64)
        self.data_mask = np.asarray(data_mask, dtype=bool)
        self.earth = earth if earth is not None else EarthModel()
        if not (self.lats.shape == self.lons.shape == self.data_mask.shape == self.los_vector.shape[:1]
                and self.los_vector.shape[1:] == (3,)):
            raise ValueError("coordinates, mask and line-of-sight vectors differ in length")
        self.correction_names = self.config.get_hierarchical_names(name=dataset_name, number=number)

    def get_station_coordinates(self, mask=None):
        if mask is None:
            mask = self.data_mask
        return np.array(self.lats)[~mask], np.array(self.lons)[~mask]

    def velocities(self, pole_lat, pole_lon, omega):
        """(n, 3) velocities [m / yr] of the stations in their local frames (north, east, third axis): the rotation
        vector w' p crossed with the station's scaled position, component by component, then one dot product per axis
        -- the reference's order of steps (heart.py:4379-4392: cross product, scaling by w', rotation), not its lines"""
        r = self.earth.radius
        sx, sy, sz = [c / r for c in self.earth.geodetic_to_ecef(self.lats, self.lons)]
        px, py, pz = [float(c) / r for c in self.earth.geodetic_to_ecef(pole_lat, pole_lon)]
        rate = omega * 1e-6 * d2r * r
        v = (rate * (py * sz - pz * sy), rate * (pz * sx - px * sz), rate * (px * sy - py * sx))
        return np.stack([_dot3(axis, v) for axis in _station_frame(self.lats, self.lons)], axis=1)

    def get_displacements(self, hierarchicals, point=None):
        v = self._values(hierarchicals, point)
        vels = self.velocities(float(v["pole_lat"]), float(v["pole_lon"]), float(v["omega"]))
        if self.data_mask.any():
            vels[self.data_mask] = 0.0
        return (vels * self.los_vector).sum(axis=1)

    def basis(self):
        x = np.stack(self.earth.geodetic_to_ecef(self.lats, self.lons), axis=1) / self.earth.radius
        north, east, down = _station_frame(self.lats, self.lons)
        ln, le, ld = self.los_vector.T
        u = np.stack([(north[k] * ln + east[k] * le) + down[k] * ld for k in range(3)], axis=1)     # T_i^T l_i
        B = np.cross(x, u)
        B[self.data_mask, :] = 0.0
        return B

    def coefficients(self, pole_lat, pole_lon, omega):
        """(3,) ``w' p`` in the order of operations of the class docstring (scalars, or arrays of equal shape ->
        (..., 3))"""
        return pole_coefficients(pole_lat, pole_lon, omega, self.earth)


def pole_coefficients(pole_lat, pole_lon, omega, earth):
    r = earth.radius
    px, py, pz = earth.geodetic_to_ecef(pole_lat, pole_lon)
    w = ((np.asarray(omega, dtype=np.float64) * 1e-6) * d2r) * r
    return np.stack([w * (px / r), w * (py / r), w * (pz / r)], axis=-1)


class StrainRateCorrection(Correction):
    """corrections.py:143-205 / heart.py:4441-4491: velocities ``D . [norths; easts]`` of the 2-d strain-rate tensor
    ``D = [[exx, (exy + rotation)/2], [(exy - rotation)/2, eyy]] * 1e-9``, zero at masked stations, projected on
    the line of sight (north, east components).  ``basis()`` folds D into one column per coefficient:

        exx: ns*n*l_n    eyy: ns*e*l_e    exy: ns/2*(e*l_n + n*l_e)    rotation: ns/2*(e*l_n - n*l_e)

    the same value in another rounding order (equal to the reference within 16 ulp of sum_k |B_k coef_k|)."""
    order = 2

    def get_required_coordinate_names(self):
        return ["lons", "lats"]

    def setup_correction(self, locy, locx, los_vector, data_mask, dataset_name, number=0, local_coordinates=None):
        """locy / locx: lats / lons [deg] (the reference's arguments); local_coordinates: (norths, easts) [m] about
        the network's midpoint, required where pyrocko is not installed to derive them"""
        self.lats = None if locy is None else np.asarray(locy, dtype=np.float64)
        self.lons = None if locx is None else np.asarray(locx, dtype=np.float64)
        self.los_vector = np.asarray(los_vector, dtype=np.float64)
        self.data_mask = np.asarray(data_mask, dtype=bool)
        if local_coordinates is None:
            local_coordinates = reproject_local(self.lats, self.lons)
        self.norths = np.asarray(local_coordinates[0], dtype=np.float64)
        self.easts = np.asarray(local_coordinates[1], dtype=np.float64)
        if not (self.norths.shape == self.easts.shape == self.data_mask.shape == self.los_vector.shape[:1]):
            raise ValueError("coordinates, mask and line-of-sight vectors differ in length")
        self.correction_names = self.config.get_hierarchical_names(name=dataset_name, number=number)

    def get_station_coordinates(self, mask=None):
        if mask is None:
            mask = self.data_mask
        return np.array(self.lats)[~mask], np.array(self.lons)[~mask]

    def get_displacements(self, hierarchicals, point=None):
        v = self._values(hierarchicals, point)
        exx, eyy = float(v["exx"]), float(v["eyy"])
        exy, rot = float(v["exy"]), float(v["rotation"])
        D = np.array([[exx, 0.5 * (exy + rot)], [0.5 * (exy - rot), eyy]]) * nanostrain
        v_x, v_y = D.dot(np.vstack([self.norths, self.easts]))
        v_xyz = np.zeros((self.norths.size, 3))
        v_xyz[:, 0] = v_x
        v_xyz[:, 1] = v_y
        if self.data_mask.any():
            v_xyz[self.data_mask, :] = 0.0
        return (v_xyz * self.los_vector).sum(axis=1)

    def basis(self):
        n, e = self.norths, self.easts
        ln, le = self.los_vector[:, 0], self.los_vector[:, 1]
        B = np.stack([nanostrain * n * ln,
                      nanostrain * e * le,
                      nanostrain / 2 * (e * ln + n * le),
                      nanostrain / 2 * (e * ln - n * le)], axis=1)
        B[self.data_mask, :] = 0.0
        return B


def correction_tables(corrections, sizes, layout, fixed=None, kinds=False):
    """What ``beatamd_ffi_model_add_geodetic_corrections`` takes, from one list of set-up correction objects per
    dataset (None / empty: no correction): (dataset index, column count, basis, offsets in q, fixed values) per term,
    in the order the terms are subtracted: per dataset the reference's ``iter_corrections`` (config.py:904-909) --
    ramp, Euler poles, strain rates, each kind in the order given.  A variable named in the layout is sampled (offset),
    one named in ``fixed`` is constant (offset -1); a name in neither raises KeyError.

    kinds=True: two more lists, what ``beatamd_ffi_model_add_geodetic_corrections_kinds`` takes in addition -- the
    kind per term (0: the offsets name the coefficients; 1: Euler pole, the offsets name pole_lat, pole_lon, omega) and
    the (radius, equator_radius, oblateness) of the term's EarthModel (zeros for a linear term).  Without it a table
    that holds a pole term is refused: five lists cannot describe it."""
    fixed = fixed or {}
    if corrections is None:
        corrections = []
    if len(corrections) not in (0, len(sizes)):
        raise ValueError("corrections: one list per dataset expected (%d datasets, %d lists)"
                         % (len(sizes), len(corrections)))
    ds, ncol, basis, offs, fixs, kind, earth = [], [], [], [], [], [], []
    for d, corrs in enumerate(corrections):
        for corr in sorted(corrs or [], key=lambda c: c.order):       # (stable)
            if not corr.correction_names:
                raise ValueError("correction of dataset %d is not set up (setup_correction)" % d)
            B = np.ascontiguousarray(corr.basis(), dtype=np.float64)
            if B.shape[0] != sizes[d] or not (1 <= B.shape[1] <= MAX_COLUMNS):
                raise ValueError("correction of dataset %d: basis %s for %d observations" % (d, B.shape, sizes[d]))
            if len(corr.correction_names) != B.shape[1]:
                raise ValueError("correction of dataset %d: %d names for %d basis columns"
                                 % (d, len(corr.correction_names), B.shape[1]))
            if corr.kind != KIND_LINEAR and not kinds:
                raise ValueError("correction of dataset %d (%s) is no plain linear term: correction_tables(kinds=True)"
                                 % (d, type(corr).__name__))
            off, fix = [], []
            for name in corr.correction_names:
                if name in layout.offsets:
                    off.append(layout.offset(name, 0))
                    fix.append(0.0)
                elif name in fixed:
                    off.append(-1)
                    fix.append(float(np.ravel(fixed[name])[0]))
                else:
                    raise KeyError("correction variable %s is neither sampled nor fixed" % name)
            ds.append(d)
            ncol.append(B.shape[1])
            basis.append(B)
            offs.append(off)
            fixs.append(fix)
            kind.append(int(corr.kind))
            earth.append(corr.earth.as_tuple() if corr.kind == KIND_EULER_POLE else (0.0, 0.0, 0.0))
    if kinds:
        return ds, ncol, basis, offs, fixs, kind, earth
    return ds, ncol, basis, offs, fixs
