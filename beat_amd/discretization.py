"""Resolution-based discretization of finite-fault surfaces for geodetic data (Atzori & Antonioli 2011; Atzori et al.
2019), the reference's ``discretization: resolution``: ``optimize_discretization`` / ``optimize_damping``
(beat/ffi/fault.py:1520-1987, :2047-2206) with ``ResolutionDiscretizationConfig`` (beat/config.py:396-464).

Patches are a struct of arrays: one row of the ten kernel parameters of ``HalfspaceSource.kernel_parameters`` per patch
(east_shift, north_shift, depth [km], strike, dip, rake [deg], length, width [km], slip [m], opening_fraction; the depth
is the TOP centre as in beat/sources.py:46-257) and the index of its subfault.  All subfaults share the event's reference
location and centres are local Cartesian: no reprojection.

The Green's functions, the smoothing operator, the resolution matrix and the division rating are computed and kept on
the device (csrc/geolib.hip, csrc/resolution.hip); per generation only diag(R), the rating and the patch attributes
cross to the host, where the discrete decisions (thresholds, argsort, the alpha cut) are taken as the reference takes
them."""
import copy
import os

import numpy as np

from . import utility
from ._marshal import upload
from .heart import HalfspaceEngine, concatenate_datasets

km = 1000.0
d2r = np.pi / 180.0

# fault.py:69-73: the unit slip of each slip component, the rake relative to the source's
slip_directions = {
    "uparr": {"slip": 1.0, "rake": 0.0},
    "uperp": {"slip": 1.0, "rake": -90.0},
    "utens": {"slip": 1.0, "rake": 0.0, "opening_fraction": 1.0},
}

EAST, NORTH, DEPTH, STRIKE, DIP, RAKE, LENGTH, WIDTH, SLIP, OPENING = range(10)


# ---------------------------------------------------------------------------------------------- patches
def strikevector(p):
    """sources.py:74-84"""
    return np.array([np.sin(p[STRIKE] * d2r), np.cos(p[STRIKE] * d2r), 0.0])


def dipvector(p):
    """sources.py:56-72"""
    return np.array([np.cos(p[DIP] * d2r) * np.cos(p[STRIKE] * d2r),
                     -np.cos(p[DIP] * d2r) * np.sin(p[STRIKE] * d2r),
                     np.sin(p[DIP] * d2r)])


def _top(p):
    return np.array([p[EAST], p[NORTH], p[DEPTH]])


def center(p):
    """sources.py:97-116: (east, north, depth) of the centre; the depth slot is the top depth"""
    return _top(p) + 0.5 * p[WIDTH] * dipvector(p)


def bottom_center(p):
    """sources.py:139-153"""
    return _top(p) + p[WIDTH] * dipvector(p)


def bottom_depth(p):
    """sources.py:155-157"""
    return float(bottom_center(p)[2])


def bottom_left(p):
    """sources.py:159-161"""
    return bottom_center(p) - 0.5 * strikevector(p) * p[LENGTH]


def get_n_patches(extent, patch_size):
    """sources.py:259-277: patches of ``patch_size`` along a side of length ``extent`` (round to 4 decimals, then ceil)"""
    return int(np.ceil(np.round(extent / patch_size, decimals=4)))


def cut_patches(p, nl, nw):
    """RectangularSource.patches (sources.py:201-257): the source row ``p`` cut into nl (strike) x nw (dip) patches,
    (nl * nw, 10), row-wise from shallow to deep; every other slot is the source's"""
    p = np.asarray(p, dtype=np.float64)
    length = p[LENGTH] / float(nl)
    width = p[WIDTH] / float(nw)
    sv, dv = strikevector(p), dipvector(p)
    top = center(p) - 0.5 * p[WIDTH] * dv       # center2top_depth(center), sources.py:118-137
    out = np.tile(p, (nl * nw, 1))
    for j in range(nw):
        for i in range(nl):
            sub_top = top + sv * ((i + 0.5 - 0.5 * nl) * length) + dv * (j * width)
            row = out[j * nl + i]
            row[EAST], row[NORTH], row[DEPTH] = sub_top
            row[LENGTH], row[WIDTH] = length, width
    return out


def divide_patch(p):
    """fault.py:1685-1691: in two along the longer side (along strike on a tie)"""
    return cut_patches(p, 2, 1) if p[LENGTH] >= p[WIDTH] else cut_patches(p, 1, 2)


def component_parameters(params, component):
    """fault.py:1279-1282: the rows with the unit slip of a slip component: rake + 0 (uparr), rake - 90 (uperp),
    opening_fraction 1 (utens); slip 1"""
    if component not in slip_directions:
        raise ValueError("Component %s not supported: %s" % (component, ", ".join(slip_directions)))
    mod = slip_directions[component]
    out = np.array(params, dtype=np.float64, copy=True).reshape(-1, 10)
    out[:, RAKE] += mod["rake"]
    out[:, SLIP] = mod["slip"]
    if "opening_fraction" in mod:
        out[:, OPENING] = mod["opening_fraction"]
    return out


class PatchSet(object):
    """struct of arrays: ``params`` (P, 10) kernel parameters and ``subfault`` (P,) index of each patch's subfault"""

    def __init__(self, params, subfault):
        self.params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, 10)
        self.subfault = np.ascontiguousarray(subfault, dtype=np.int64).reshape(-1)
        if self.subfault.size != self.params.shape[0]:
            raise ValueError("one subfault index per patch")

    def __len__(self):
        return self.params.shape[0]

    lengths = property(lambda self: self.params[:, LENGTH])
    widths = property(lambda self: self.params[:, WIDTH])

    @property
    def centers(self):
        return np.array([center(p) for p in self.params]).reshape(-1, 3)


def get_division_mapping(patch_idxs, div_idxs, subfault_npatches):
    """fault.py:1386-1433 with its return values: (old2new {old patch index -> new index} of the undivided patches,
    div2new {running index of a half -> new index}, new_subfault_npatches).  A divided patch is replaced in place by
    its two halves; ``div2new`` counts the halves in the order the patches are divided."""
    div = set(int(i) for i in div_idxs)
    subfault_npatches = np.asarray(subfault_npatches)
    old2new, div2new = {}, {}
    new_subfault_npatches = np.zeros_like(subfault_npatches)
    tot = half = old = 0
    sf_idx = in_sf_old = in_sf_new = 0
    for patch_idx in patch_idxs:
        if patch_idx in div:
            for _ in range(2):
                div2new[half] = tot
                half += 1
                tot += 1
            in_sf_new += 2
        else:
            old2new[old] = tot
            tot += 1
            in_sf_new += 1
        old += 1
        in_sf_old += 1
        if in_sf_old == subfault_npatches[sf_idx]:
            new_subfault_npatches[sf_idx] = in_sf_new
            sf_idx += 1
            in_sf_old = in_sf_new = 0
    return old2new, div2new, new_subfault_npatches


# ---------------------------------------------------------------------------------------------- configuration
class ResolutionDiscretizationConfig(object):
    """config.py:396-464, field names and defaults"""

    def __init__(self, epsilon=4.0e-3, epsilon_search_runs=1, resolution_thresh=0.999, depth_penalty=3.5, alpha=0.3,
                 patch_widths_min=(1.0,), patch_widths_max=(5.0,), patch_lengths_min=(1.0,), patch_lengths_max=(5.0,),
                 extension_widths=(0.1,), extension_lengths=(0.1,)):
        self.epsilon = float(epsilon)
        self.epsilon_search_runs = int(epsilon_search_runs)
        self.resolution_thresh = float(resolution_thresh)
        self.depth_penalty = float(depth_penalty)
        self.alpha = float(alpha)
        self.patch_widths_min = list(patch_widths_min)
        self.patch_widths_max = list(patch_widths_max)
        self.patch_lengths_min = list(patch_lengths_min)
        self.patch_lengths_max = list(patch_lengths_max)
        self.extension_widths = list(extension_widths)
        self.extension_lengths = list(extension_lengths)

    def get_patch_dimensions(self):
        """-> (patch_widths, patch_lengths) of the initial discretization"""
        return self.patch_widths_max, self.patch_lengths_max


class ResolutionDiscretizationResult(object):
    """fault.py:1990-2044 without the plot"""

    def __init__(self, epsilons=(0,), normalized_rspreads=(1.0,), faults_npatches=(1,)):
        self.epsilons = [float(e) for e in epsilons]
        self.normalized_rspreads = [float(r) for r in normalized_rspreads]
        self.faults_npatches = [int(n) for n in faults_npatches]
        self.optimum = {}

    def derive_optimum_fault_geometry(self):
        data = np.vstack((np.array(self.epsilons), np.array(self.normalized_rspreads))).T
        best_idx, _ = utility.find_elbow(data, rotate_left=True)
        best_idx = int(best_idx)
        self.optimum = {"epsilon": self.epsilons[best_idx], "normalized_rspread": self.normalized_rspreads[best_idx],
                        "npatches": self.faults_npatches[best_idx], "idx": best_idx}

    def dump(self):
        import yaml
        body = dict(epsilons=self.epsilons, normalized_rspreads=self.normalized_rspreads,
                    faults_npatches=self.faults_npatches, optimum=dict(self.optimum))
        return "--- !beat.ffi.ResolutionDiscretizationResult\n" + yaml.safe_dump(body, default_flow_style=False,
                                                                                  sort_keys=False)


# ---------------------------------------------------------------------------------------------- the fault
class DiscretizedFault(object):
    """the part of FaultGeometry (fault.py:97-1100) the discretizer uses: reference subfaults (nsf, 10), their patches
    and, once optimized, the model resolution matrix"""

    def __init__(self, subfaults):
        self.subfaults = np.ascontiguousarray(subfaults, dtype=np.float64).reshape(-1, 10)
        self.patches = PatchSet(np.zeros((0, 10)), np.zeros(0, dtype=np.int64))
        self.subfault_npatches = [0] * self.nsubfaults
        self._model_resolution = None

    nsubfaults = property(lambda self: self.subfaults.shape[0])
    npatches = property(lambda self: int(sum(self.subfault_npatches)))

    @property
    def cum_subfault_npatches(self):
        return np.concatenate([[0], np.cumsum(self.subfault_npatches)]).astype(np.int64)

    def iter_subfaults(self):
        return iter(self.subfaults)

    def set_patches(self, params, subfault_npatches):
        subfault_npatches = [int(n) for n in subfault_npatches]
        self.patches = PatchSet(params, np.repeat(np.arange(len(subfault_npatches)), subfault_npatches))
        self.subfault_npatches = subfault_npatches

    def get_all_patches(self, datatype="geodetic", component=None):
        """(P, 10) rows; with a component: of its unit slip"""
        return self.patches.params if component is None else component_parameters(self.patches.params, component)

    def get_event_relative_patch_centers(self, event=None):
        """fault.py:758-788 -> (P, 3) [km]; no reprojection"""
        return self.patches.centers

    def get_smoothing_operator(self, event=None, correlation_function="nearest_neighbor"):
        """fault.py:790-828 on the host; a resolution-based discretization has no nearest-neighbour operator"""
        from .models.laplacian import get_smoothing_operator
        return get_smoothing_operator(None, self.get_event_relative_patch_centers(event), correlation_function)

    def set_model_resolution(self, model_resolution):
        self._model_resolution = model_resolution

    def get_model_resolution(self):
        """(P, P) host array"""
        R = self._model_resolution
        return R.cpu().numpy() if hasattr(R, "cpu") else R


def _engine_ctx(engine):
    if not isinstance(engine, HalfspaceEngine):
        raise TypeError("engine %r provides no static displacements (HalfspaceEngine does; the "
                        "reference's layered GF-store engine is pyrocko's and out of scope)" % (engine,))
    return engine.ctx


def _data_coords(datasets, event=None):
    """fault.py:1591-1600: (nobs, 2) [km] east, north"""
    es, ns = [], []
    for dataset in datasets:
        n, e = dataset.update_local_coords(event)
        ns.append(n / km)
        es.append(e / km)
    return np.vstack([np.hstack(es), np.hstack(ns)]).T


def optimize_discretization(config, fault, datasets, varnames, crust_ind=0, engine=None, targets=None, event=None,
                            force=False, nworkers=1, method="laplacian", debug=False, history=None):
    """fault.py:1520-1987, same control flow -> (fault, mean_R).  ``fault`` (a DiscretizedFault) is updated in place;
    its model resolution is the device tensor of R_matrix.  ``history`` (a list) receives one dict per generation:
    sf_div_idxs, fixed_idxs, subfault_npatches, R_diag (mean over the components), rating."""
    import torch
    from .ffi import geo_construct_gf_linear_patches

    if method == "svd":
        # fault.py:1778-1800 computes R but never `resolution_matrix`, which :1820 reads: the branch cannot finish in
        # the reference either, and optimize_damping hard-codes "laplacian" (:2130)
        raise NotImplementedError('method "svd" is not built: the reference\'s svd branch leaves resolution_matrix '
                                  'undefined (beat/ffi/fault.py:1778-1820); use "laplacian"')
    if method != "laplacian":
        raise NotImplementedError("Supported methods: laplacian, svd, specified: %s" % method)
    ctx = _engine_ctx(engine)
    data_coords = _data_coords(datasets, event)
    dev = torch.device("cuda:%d" % ctx.device)
    d_data = upload(data_coords, dev)

    # :1602-1627 the initial cut at twice the maximum patch size; the components share one geometry
    patch_widths, patch_lengths = config.get_patch_dimensions()
    rows, counts = [], []
    for index, sf in enumerate(fault.iter_subfaults()):
        npw = get_n_patches(sf[WIDTH], 2 * patch_widths[index])
        npl = get_n_patches(sf[LENGTH], 2 * patch_lengths[index])
        rows.append(cut_patches(sf, npl, npw))
        counts.append(npl * npw)
    fault.set_patches(np.vstack(rows), counts)
    # every component's rows of a generation go through one launch
    gfs_comp = list(geo_construct_gf_linear_patches(
        engine, datasets=datasets,
        patches=np.vstack([fault.get_all_patches("geodetic", c) for c in varnames]),
        device=True).reshape(len(varnames), fault.npatches, -1))

    tobedivided = fault.npatches
    # :1631-1644 the first generation divides every patch of every subfault above the minimum size
    sf_div_idxs = []
    for i, sf in enumerate(fault.iter_subfaults()):
        if not (sf[WIDTH] <= config.patch_widths_min[i] or sf[LENGTH] <= config.patch_lengths_min[i]):
            sf_div_idxs.extend((np.arange(fault.subfault_npatches[i]) + fault.cum_subfault_npatches[i]).tolist())

    generation = 0
    fixed_idxs = set()
    bottom_depths_sf = np.array([bottom_depth(sf) for sf in fault.iter_subfaults()]) * km   # [m], :1905
    while tobedivided:
        subfault_npatches = copy.deepcopy(fault.subfault_npatches)
        # :1676-1748; the mapping and the divided geometry are the same for every component
        old2new, div2new, new_subfault_npatches = get_division_mapping(
            patch_idxs=range(sum(subfault_npatches)), div_idxs=sf_div_idxs, subfault_npatches=subfault_npatches)
        old_params = fault.patches.params
        divided = (np.vstack([divide_patch(old_params[i]) for i in sf_div_idxs]) if len(sf_div_idxs)
                   else np.zeros((0, 10)))
        new_total = int(np.sum(new_subfault_npatches))
        div_set = set(int(j) for j in sf_div_idxs)
        kept_src = np.array([i for i in range(len(old_params)) if i not in div_set], dtype=np.int64)
        # old2new is keyed by the old patch index of the undivided patches (:1424 counts "old" for divided ones too)
        kept_dst = np.array([old2new[int(i)] for i in kept_src], dtype=np.int64)
        div_dst = np.array([div2new[k] for k in range(len(divided))], dtype=np.int64)
        new_params = np.zeros((new_total, 10))
        new_params[kept_dst] = old_params[kept_src]
        new_params[div_dst] = divided
        # only the divided patches get new library rows; the old rows move on the device
        if len(divided):
            new_rows = geo_construct_gf_linear_patches(
                engine, datasets=datasets, patches=np.vstack([component_parameters(divided, c) for c in varnames]),
                device=True).reshape(len(varnames), len(divided), -1)
        t_ks, t_kd = torch.from_numpy(kept_src).to(dev), torch.from_numpy(kept_dst).to(dev)
        t_dd = torch.from_numpy(div_dst).to(dev)
        for gfs_i in range(len(varnames)):
            old_gfs = gfs_comp[gfs_i]
            new_gfs = torch.empty((new_total, old_gfs.shape[1]), dtype=torch.float64, device=dev)
            new_gfs[t_kd] = old_gfs[t_ks]
            if len(divided):
                new_gfs[t_dd] = new_rows[gfs_i]
            gfs_comp[gfs_i] = new_gfs
        fault.set_patches(new_params, new_subfault_npatches)

        # :1751 update fixed indexes
        fixed_idxs = set([old2new[idx] for idx in fixed_idxs])

        # :1773-1831 resolution of every component; L and R stay on the device
        centers = fault.get_event_relative_patch_centers(event)
        d_centers = upload(centers, dev)
        smoothing_op = ctx.smoothing_correlated(d_centers, "gaussian")
        resolution_matrices, R_diags = [], []
        for gfs_i, component in enumerate(varnames):
            resolution_matrix, d_diag = ctx.model_resolution(gfs_comp[gfs_i], smoothing_op, config.epsilon)
            R = d_diag.cpu().numpy()
            R_diags.append(R)
            resolution_matrices.append(resolution_matrix)
            # :1822 sits inside the component loop and is read after it: R_idxs is the LAST component's, while
            # fixed_idxs accumulates over the components (:1831)
            R_idxs = np.argwhere(R > config.resolution_thresh).ravel().tolist()
            fixed_idxs.update(set(np.argwhere(R <= config.resolution_thresh).ravel().tolist()))

        # :1835-1875 size thresholds
        widths, lengths = fault.patches.widths, fault.patches.lengths
        sf_of = fault.patches.subfault
        wmax = np.asarray(config.patch_widths_max, dtype=np.float64)[sf_of]
        lmax = np.asarray(config.patch_lengths_max, dtype=np.float64)[sf_of]
        wmin = np.asarray(config.patch_widths_min, dtype=np.float64)[sf_of]
        lmin = np.asarray(config.patch_lengths_min, dtype=np.float64)[sf_of]
        patch_size_ids = set(np.argwhere((widths <= wmin) | (lengths <= lmin)).ravel().tolist())
        # patches above the maximum size are always candidates, and never fixed (:1867-1875)
        above_size_thresh = set(np.argwhere((widths > wmax) | (lengths > lmax)).ravel().tolist())
        fixed_idxs = fixed_idxs.difference(above_size_thresh)
        unique_ids = set(R_idxs).difference(patch_size_ids, fixed_idxs).union(above_size_thresh)
        ncandidates = len(unique_ids)

        mean_R = np.vstack(R_diags).mean(0).ravel()       # :1884
        rating = None
        if ncandidates:
            # :1886-1929 on the device; the argsort and the alpha cut are O(P) and discrete: host
            d_rating, _ = ctx.division_rating(
                upload(widths, dev), upload(lengths, dev), d_centers, upload(bottom_depths_sf[sf_of], dev), config.depth_penalty,
                d_data, torch.from_numpy(mean_R).to(dev))
            rating = d_rating.cpu().numpy()
            rating_idxs = np.array(rating.argsort()[::-1])
            rated_sel = np.array([ridx for ridx in rating_idxs if ridx in unique_ids])
            n_sel = len(rated_sel)
            idxs = rated_sel[:int(np.ceil(config.alpha * n_sel))]        # :1934
            tobedivided = len(idxs)
            sf_div_idxs = np.sort(copy.deepcopy(idxs))
            generation += 1
        else:
            tobedivided = 0
            sf_div_idxs = np.zeros(0, dtype=np.int64)
        if history is not None:
            history.append(dict(sf_div_idxs=np.array(sf_div_idxs, dtype=np.int64), fixed_idxs=sorted(fixed_idxs),
                                subfault_npatches=list(fault.subfault_npatches), R_diag=mean_R.copy(),
                                rating=None if rating is None else rating.copy()))

    # :1982 R_matrix is the mean over the components
    R_matrix = resolution_matrices[0] if len(resolution_matrices) == 1 else torch.stack(resolution_matrices).mean(0)
    fault.set_model_resolution(R_matrix)
    return fault, mean_R


def optimize_damping(outdir, config, fault, datasets, varnames, crust_ind=0, engine=None, targets=None, event=None,
                     force=False, nworkers=1, method="laplacian", plot=False, figuredir=None, debug=False):
    """fault.py:2057-2206: one discretization per epsilon of logspace(0, 2, runs) * epsilon, the optimum by the elbow of
    the normalized resolution spreads -> (best fault, ResolutionDiscretizationResult).  Files are written only with an
    ``outdir``: <outdir>/discretization/resolution_result_<epsilon>_<runs>.yaml and, per epsilon, the patch table
    fault_geometry_<epsilon>.npz where the reference pickles the fault object.  Plots are out of scope."""
    epsilons = np.logspace(0, 2, config.epsilon_search_runs, endpoint=True) * config.epsilon
    eps0 = config.epsilon
    discr_dir = None
    if outdir:
        discr_dir = os.path.join(outdir, "discretization")
        os.makedirs(discr_dir, exist_ok=True)
    dfaults = []
    try:
        for epsilon in epsilons:
            config.epsilon = float(epsilon)
            dfault, _ = optimize_discretization(config, copy.deepcopy(fault), datasets, varnames, crust_ind, engine,
                                                targets, event, force, nworkers, method="laplacian", debug=False)
            dfaults.append(dfault)
            if discr_dir:
                np.savez(os.path.join(discr_dir, "fault_geometry_%s.npz" % epsilon), params=dfault.patches.params,
                         subfault_npatches=np.array(dfault.subfault_npatches),
                         model_resolution=dfault.get_model_resolution())
    finally:
        config.epsilon = eps0        # :2140 overwrite again with the original value
    result = ResolutionDiscretizationResult(
        epsilons=epsilons.tolist(),
        normalized_rspreads=[utility.normalized_resolution_spread(f.get_model_resolution(), nparams=f.npatches)
                             for f in dfaults],
        faults_npatches=[f.npatches for f in dfaults])
    result.derive_optimum_fault_geometry()
    if discr_dir:
        with open(os.path.join(discr_dir, "resolution_result_%g_%i.yaml" % (eps0, config.epsilon_search_runs)),
                  "w") as f:
            f.write(result.dump())
    return dfaults[result.optimum["idx"]], result
