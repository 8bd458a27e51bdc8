"""
First-motion polarity likelihood of a point-source moment tensor: the counterpart of ``PolarityComposite``
(beat/models/polarity.py:32-134) for whole populations of chains.

    sampled source parameters -> normalised moment tensor -> radiation amplitude per station
                              -> cumulative-normal likelihood per station (``polarity_like``, a vector)

The forward model runs in one kernel launch per evaluation (csrc/polarity.hip) inside the same fused Metropolis step as
every other composite; the prior box, SMC / PT / Metropolis, graph capture and the chain files are the shared code path.

What stays outside: ray tracing.  In the reference ``PolarityMapping.update_targets`` asks pyrocko's cake for the
takeoff angles of every station (heart.py, third-party arithmetic); here they are inputs of ``PolarityMap``.  They
depend on the source location, so a sampled location (north_shift, east_shift, depth) is refused: the composite is the
reference's ``is_location_fixed=True`` case (the shipped example project MTQT_polarity fixes the location).
"""
import numpy as np

from .. import heart, polarity_binding
from ..engine import get_context
from ..sources import SOURCE_KINDS
from .problem import LogpForwFunc

LOCATION_VARIABLES = ("north_shift", "east_shift", "depth")
WAVENAMES = ("any_P", "any_SH", "any_SV")


def polarity_hyper_name(wavename, mapnumber):
    """config.py:785-792: ``h_<name>_pol_<i>``"""
    return "_".join(("h", wavename, "pol", str(mapnumber)))


class PolarityMap(object):
    """one polarity map (heart.PolarityMapping): the stations of one wave type.

    name                 "any_P", "any_SH" or "any_SV"
    takeoff_angles_rad   (n_t,) from the downward vertical, [0, pi]
    azimuths_rad         (n_t,) from north
    polarities           (n_t,) observed first motions, +1 / -1 (0: no reading, both outcomes weigh one half)
    """

    def __init__(self, name, takeoff_angles_rad, azimuths_rad, polarities):
        if name not in WAVENAMES:
            raise ValueError("polarity map %r: the wave type is one of %s" % (name, ", ".join(WAVENAMES)))
        self.name = name
        self.takeoff_angles_rad = np.ascontiguousarray(takeoff_angles_rad, dtype=np.float64).ravel()
        self.azimuths_rad = np.ascontiguousarray(azimuths_rad, dtype=np.float64).ravel()
        pol = np.asarray(polarities)
        self.dataset = pol.astype(np.int16).ravel()
        if not (self.takeoff_angles_rad.size == self.azimuths_rad.size == self.dataset.size >= 1):
            raise ValueError("polarity map %s: %d takeoff angles, %d azimuths, %d polarities"
                             % (name, self.takeoff_angles_rad.size, self.azimuths_rad.size, self.dataset.size))
        if np.any(pol != self.dataset.reshape(pol.shape)) or np.any(np.abs(self.dataset) > 1):
            raise ValueError("polarity map %s: polarities are +1, -1 or 0" % name)
        self._radiation_weights = None
        self.update_radiation_weights()

    @property
    def n_t(self):
        return int(self.dataset.size)

    def update_radiation_weights(self):
        self._radiation_weights = heart.calculate_radiation_weights(self.takeoff_angles_rad, self.azimuths_rad, self.name)

    def get_radiation_weights(self):
        return self._radiation_weights


class PolarityProblem(object):
    """
    layout       ParameterLayout over the sampled variables (source variables and hyper-parameters, one entry each)
    source_kind  "mtqt" (w, v, kappa, sigma, h), "mt" (mnn, mee, mdd, mne, mnd, med) or "dc" (strike, dip, rake [deg])
    maps         list of PolarityMap
    hypers       per map the name of its sigma (None: ``h_<name>_pol_<i>`` for every map); sampled where the layout
                 holds it, constant where ``fixed`` does
    fixed        dict name -> value of everything that is not sampled
    gamma        probability of a wrong polarity reading (polarity.py:45)
    geodetic     optionally a GeodeticGeometryProblem over the SAME layout: both composites in one model, the geodetic
                 columns first
    """

    def __init__(self, layout, source_kind, maps, hypers=None, fixed=None, gamma=0.2, lower=None, upper=None,
                 geodetic=None):
        if source_kind not in SOURCE_KINDS:
            raise ValueError("unknown polarity source kind %r (one of %s)" % (source_kind, ", ".join(sorted(SOURCE_KINDS))))
        self.layout = layout
        self.source_kind = source_kind
        self.maps = list(maps)
        if not self.maps:
            raise ValueError("a polarity problem needs at least one polarity map")
        self.hypers = list(hypers) if hypers is not None else [polarity_hyper_name(m.name, i)
                                                                for i, m in enumerate(self.maps)]
        if len(self.hypers) != len(self.maps):
            raise ValueError("%d hyper-parameter names for %d polarity maps" % (len(self.hypers), len(self.maps)))
        self.fixed = dict(fixed or {})
        self.gamma = float(gamma)
        self.lower, self.upper = lower, upper
        if geodetic is not None and geodetic.layout is not layout:
            raise ValueError("the geodetic composite of a polarity problem is described over the same layout object")
        sampled = [v for v in LOCATION_VARIABLES if v in layout.offsets]
        if sampled:
            raise NotImplementedError(
                "a sampled source location (%s) is not available for the polarity composite: the takeoff angles depend on "
                "it and their ray tracing is pyrocko's -- fix the location (is_location_fixed, pytensorf.py:355-362)"
                % ", ".join(sampled))
        for name in layout.offsets:
            if layout.varsizes[name] != 1 and geodetic is None:
                raise ValueError("variable %s has %d entries: the polarity composite has one source" % (name, layout.varsizes[name]))
        # what LogpForwFunc expects of a problem
        self.wavemaps, self.geodetic, self.laplacian, self.polarity = [], geodetic, None, self

    @property
    def n_t(self):
        return sum(m.n_t for m in self.maps)

    @property
    def hyper_names(self):
        return list(self.hypers)

    @property
    def out_names(self):
        geo = self.geodetic.out_names[:-1] if self.geodetic is not None else []
        return geo + ["polarity_like"] + ["like"]

    def _slots(self, names, what):
        off = -np.ones(len(names), dtype=np.int64)
        fix = np.zeros(len(names))
        for k, name in enumerate(names):
            if name in self.layout.offsets:
                off[k] = self.layout.offset(name, 0)
            elif name in self.fixed:
                fix[k] = float(np.ravel(self.fixed[name])[0])
            else:
                raise KeyError("%s %s is neither sampled nor fixed" % (what, name))
        return off, fix

    def source_tables(self):
        """(6,) offsets in q (-1: fixed) and fixed values of the source variables, in the kernel's order"""
        names = SOURCE_KINDS[self.source_kind][1]
        off, fix = -np.ones(6, dtype=np.int64), np.zeros(6)
        off[:len(names)], fix[:len(names)] = self._slots(names, "source parameter")
        return off, fix

    def hyper_tables(self):
        return self._slots(self.hypers, "hyper-parameter")

    def radiation_weights(self):
        """(6, n_t) of all maps side by side"""
        return np.ascontiguousarray(np.concatenate([m.get_radiation_weights() for m in self.maps], axis=1))

    def observations(self):
        return np.concatenate([m.dataset for m in self.maps]).astype(np.float64)

    def source(self, point):
        """the host source object (beat_amd.sources) at a point {name: value}"""
        cls, names = SOURCE_KINDS[self.source_kind]
        vals = dict(self.fixed)
        vals.update(point)
        return cls(**{n: float(np.ravel(vals[n])[0]) for n in names})

    def compile(self, ctx=None):
        from .. import _lib
        ctx = ctx or get_context()
        L = _lib.FfiLayout()
        L.nparams = self.layout.size
        L.nvar = 0
        for i in range(4):
            L.slip_off[i] = -1
        for f in ("durations_off", "velocities_off", "nuc_strike_off", "nuc_dip_off", "time_off", "h_laplacian_off"):
            setattr(L, f, -1)
        mid = ctx.ffi_model_create(L, [], [], [])
        if self.geodetic is not None:
            self.geodetic.add_to_model(ctx, mid)
        off, fix = self.source_tables()
        hoff, hfix = self.hyper_tables()
        polarity_binding.ffi_model_add_polarity(ctx, mid, self.source_kind, off, fix, [m.n_t for m in self.maps], self.radiation_weights(),
                                                self.observations(), self.gamma, hoff, hfix)
        return LogpForwFunc(ctx, mid, self)
