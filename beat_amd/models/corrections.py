"""
Hierarchical corrections of geodetic datasets -- the counterpart of

  beat/models/corrections.py:46-87      RampCorrection       (orbital ramp of a SAR scene)
  beat/models/corrections.py:143-205    StrainRateCorrection (strain-rate tensor of a GNSS network)
  beat/config.py:802-892                the configuration holders and the hierarchical names
  beat/models/geodetic.py:411-427       GeodeticComposite.apply_corrections (residuals[i] -= correction)

The reference subtracts every enabled correction of a dataset from its weighted residual before
``multivariate_normal_chol`` (geodetic.py:1076-1077); the coefficients are sampled with everything else.  Here
every correction is a linear term ``sum_k B[:, k] * coef_k`` over at most four constant basis columns
(``basis()``), uploaded once and subtracted on the device in the kernel that forms the residual
(``beatamd_ffi_model_add_geodetic_corrections``).  ``get_displacements(hierarchicals, point)`` is the host
(numpy) evaluation post-processing calls, the reference's ``point`` branch.

The Euler-pole correction (corrections.py:90-140) is not offered: its velocities are not linear in the sampled
pole position, and the spherical geometry behind them is pyrocko's.
"""
import numpy as np

km = 1000.0
nanostrain = 1e-9
MAX_COLUMNS = 4


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


class StrainRateConfig(CorrectionConfig):
    """config.py:828-837, 856-869"""
    feature = "Strain Rate"
    _suffixes = ("exx", "eyy", "exy", "rotation")

    def __init__(self, dataset_names=(), enabled=False, station_blacklist=(), station_whitelist=()):
        CorrectionConfig.__init__(self, dataset_names, enabled)
        self.station_blacklist = list(station_blacklist)
        self.station_whitelist = list(station_whitelist)

    def get_hierarchical_names(self, name=None, number=0):
        # config.py:836-837: "<number>_<suffix>"
        return ["%s_%s" % (number, s) for s in self.get_suffixes()]

    def init_correction(self):
        self.check_consistency()
        return StrainRateCorrection(self)


class Correction(object):
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


class StrainRateCorrection(Correction):
    """corrections.py:143-205 / heart.py:4441-4491: velocities ``D . [norths; easts]`` of the 2-d strain-rate tensor
    ``D = [[exx, (exy + rotation)/2], [(exy - rotation)/2, eyy]] * 1e-9``, zero at masked stations, projected on
    the line of sight (north, east components).  ``basis()`` folds D into one column per coefficient:

        exx: ns*n*l_n    eyy: ns*e*l_e    exy: ns/2*(e*l_n + n*l_e)    rotation: ns/2*(e*l_n - n*l_e)

    the same value in another rounding order (equal to the reference within 16 ulp of sum_k |B_k coef_k|)."""

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


def correction_tables(corrections, sizes, layout, fixed=None):
    """What ``beatamd_ffi_model_add_geodetic_corrections`` takes, from one list of set-up correction objects per
    dataset (None / empty: no correction): (dataset index, column count, basis, offsets in q, fixed values) per term,
    in the order the terms are subtracted.  A coefficient named in the layout is sampled (offset), one named in
    ``fixed`` is constant (offset -1); a name in neither raises KeyError."""
    fixed = fixed or {}
    if corrections is None:
        corrections = []
    if len(corrections) not in (0, len(sizes)):
        raise ValueError("corrections: one list per dataset expected (%d datasets, %d lists)"
                         % (len(sizes), len(corrections)))
    ds, ncol, basis, offs, fixs = [], [], [], [], []
    for d, corrs in enumerate(corrections):
        for corr in (corrs or []):
            if not corr.correction_names:
                raise ValueError("correction of dataset %d is not set up (setup_correction)" % d)
            B = np.ascontiguousarray(corr.basis(), dtype=np.float64)
            if B.shape[0] != sizes[d] or not (1 <= B.shape[1] <= MAX_COLUMNS):
                raise ValueError("correction of dataset %d: basis %s for %d observations" % (d, B.shape, sizes[d]))
            if len(corr.correction_names) != B.shape[1]:
                raise ValueError("correction of dataset %d: %d names for %d basis columns"
                                 % (d, len(corr.correction_names), B.shape[1]))
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
    return ds, ncol, basis, offs, fixs
