"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/discretization_reference.npz, tests/golden/discretization_fixture.npz and
profiles/discretization_tolerance.json.

    python tools/gen_golden_discretization.py

discretization_reference.npz: outputs of the REFERENCE's own functions on seeded inputs (needs the reference tree;
oracle/ref_import.py finds it and stubs the packages that are not installed) --
  beat/ffi/fault.py:1386-1433   get_division_mapping
  beat/ffi/fault.py:2047-2054   normalized_resolution_spread
  beat/models/laplacian.py:261-298  get_smoothing_operator_correlated ("gaussian", "exponential")
  beat/utility.py:1695-1723     distances
  beat/utility.py:1622-1655     find_elbow (with get_data_radiant)
The fixture is data: inputs and recorded outputs, none of the reference's text.

discretization_fixture.npz (metadata: "restated"): the fixture problem of tests/discretization_ref.py run through that
module's numpy restatement of optimize_discretization -- RectangularSource.patches needs pyrocko's base class and the
Green's functions pyrocko's engine, so the reference's own loop cannot run here.  Recorded per generation: the division
indexes, the fixed indexes, the patches per subfault, diag(R), the rating; the final patch table, mean_R and R_matrix;
for three epsilons the normalized resolution spreads, patch counts and the optimum index.  The generator ASSERTS the
margins that keep a discrete decision from hiding a rounding difference and fails if they do not hold (then change the
fixture geometry, never the condition):
  * every diag(R) entry of every generation is at least 1e-6 away from resolution_thresh;
  * the ratings at the alpha cut, and any two ratings of candidates, differ by at least 1e-9 relative;
  * at least three generations, some patches fixed and some at minimum size at the end, a final P that is no multiple
    of 16.

discretization_tolerance.json: the spread between two algebraically equal float64 routes to R on the CPU over the
same inputs -- the reference's inv(.).dot(.) and a Cholesky solve -- relative to max|R|, per generation and component
and for a random 130 x 67 G; the device bound is ten times the spread (it sums in a third order, in MFMA blocks) with a
floor of 1e-13.  The same numbers are in the fixture, which is what the tests read.
"""
import importlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402

import discretization_ref as dref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
FLOOR, FACTOR = 1e-13, 10.0


def reference_outputs():
    ref_import.install()
    try:
        import fast_sweep_ext  # noqa: F401  (oracle/_ref)
    except ImportError:
        sys.modules["fast_sweep_ext"] = types.ModuleType("fast_sweep_ext")
        sys.modules["beat.fast_sweeping.fast_sweep_ext"] = sys.modules["fast_sweep_ext"]
    fault_mod = importlib.import_module("beat.ffi.fault")
    util = importlib.import_module("beat.utility")
    lap = importlib.import_module("beat.models.laplacian")
    rng = np.random.RandomState(424242)
    out = {}
    # get_division_mapping: several subfaults, none / some / all divided, first and last patch of a subfault
    cases = [([6, 4], [1, 5, 8]), ([6, 4], []), ([3, 2, 4], list(range(9))), ([5], [0, 4]), ([2, 7, 1], [1, 2, 8, 9])]
    for k, (counts, div) in enumerate(cases):
        o2n, d2n, new = fault_mod.get_division_mapping(range(sum(counts)), div, np.array(counts))
        out["map%d_counts" % k], out["map%d_div" % k] = np.array(counts), np.array(div, dtype=np.int64)
        out["map%d_old2new" % k] = np.array(list(o2n.items()), dtype=np.int64).reshape(-1, 2)
        out["map%d_div2new" % k] = np.array(list(d2n.items()), dtype=np.int64).reshape(-1, 2)
        out["map%d_new" % k] = np.asarray(new)
    out["nmap"] = np.array(len(cases))
    # distances and the operators: 46 and 130 patches (the second past numpy's pairwise block of 128)
    for tag, n in (("a", 46), ("b", 130)):
        coords = rng.uniform(-8.0, 11.0, (n, 3))
        coords[:, 2] = np.abs(coords[:, 2])
        out["coords_" + tag] = coords
        if tag == "a":
            out["dist_" + tag] = util.distances(coords, coords)
        out["gauss_" + tag] = lap.get_smoothing_operator_correlated(coords, "gaussian")
        out["expo_" + tag] = lap.get_smoothing_operator_correlated(coords, "exponential")
    pts, refp = rng.normal(size=(7, 2)), rng.normal(size=(5, 2))
    out["dist2_points"], out["dist2_ref"], out["dist2"] = pts, refp, util.distances(pts, refp)
    # normalized_resolution_spread
    Rm = np.eye(23) * 0.9 + rng.normal(scale=0.02, size=(23, 23))
    out["spread_R"], out["spread"] = Rm, np.array(fault_mod.normalized_resolution_spread(Rm, 23))
    # find_elbow
    eps = np.logspace(0, 2, 7) * 0.01
    spreads = 0.02 + 0.05 / (1 + (eps / 0.05) ** 2) + 0.01 * eps
    data = np.vstack((eps, spreads)).T
    for tag, kw in (("left", dict(rotate_left=True)), ("plain", dict()), ("theta", dict(theta=0.3))):
        idx, rot = util.find_elbow(data, **kw)
        out["elbow_%s_idx" % tag], out["elbow_%s_rot" % tag] = np.array(idx), rot
    out["elbow_data"] = data
    out["radiant"] = np.array(util.get_data_radiant(data))
    out["metadata"] = np.array("outputs of the reference's own functions (beat 2.0.5 tree), numpy %s" % np.__version__)
    return out


def _spread(G, L, eps):
    Ra, Rb = dref.resolution(G, L, eps), dref.resolution_cholesky(G, L, eps)
    return float(np.abs(Ra - Rb).max() / np.abs(Ra).max())


def fixture():
    fp = dref.fixture_problem()
    cfg, thresh = fp["cfg"], fp["cfg"]["resolution_thresh"]
    args = (fp["subfaults"], fp["east"], fp["north"], fp["los"], fp["odw"], fp["nu"], fp["varnames"])
    res = dref.optimize(cfg, *args)
    gens = res["generations"]
    out, tol = {}, {"factor": FACTOR, "floor": FLOOR, "generations": []}
    assert len(gens) >= 3, "fewer than three generations"
    assert gens[-1]["fixed_idxs"] and gens[-1]["at_min"], "no fixed patch or no patch at minimum size at the end"
    assert len(res["params"]) % 16 != 0, "final P is a multiple of 16"
    for g, gen in enumerate(gens):
        margin = np.abs(gen["R_diags"] - thresh).min()
        assert margin >= 1e-6, "generation %d: diag(R) within %.1e of the threshold" % (g, margin)
        if gen["rating"] is not None:
            rt = gen["rating"][gen["rated_sel"]]         # descending
            rel = (rt[:-1] - rt[1:]) / np.abs(rt[:-1]) if len(rt) > 1 else np.array([1.0])
            assert rel.min() >= 1e-9, "generation %d: candidate ratings within %.1e relative" % (g, rel.min())
        spreads = [_spread(gen["gfs"][k].T, gen["L"], cfg["epsilon"]) for k in range(len(fp["varnames"]))]
        tol["generations"].append({"npatches": int(len(gen["params"])), "spread": spreads,
                                   "bound": [max(FACTOR * s, FLOOR) for s in spreads]})
        out["g%d_sf_div_idxs" % g] = gen["sf_div_idxs"]
        out["g%d_fixed_idxs" % g] = np.array(gen["fixed_idxs"], dtype=np.int64)
        out["g%d_subfault_npatches" % g] = np.array(gen["subfault_npatches"], dtype=np.int64)
        out["g%d_mean_R" % g] = gen["mean_R"]
        out["g%d_rating" % g] = gen["rating"] if gen["rating"] is not None else np.zeros(0)
        out["g%d_bound" % g] = np.array(tol["generations"][-1]["bound"])
    out["ngen"] = np.array(len(gens))
    out["params"], out["subfault_npatches"] = res["params"], np.array(res["subfault_npatches"], dtype=np.int64)
    out["mean_R"], out["R_matrix"] = res["mean_R"], res["R_matrix"]
    # a random 130 x 67 G with a correlated operator of random centres
    rng = np.random.RandomState(6730)
    G = rng.normal(size=(130, 67))
    c = rng.uniform(0.0, 9.0, (67, 3))
    L = dref.smoothing_correlated(c, "gaussian")
    s = _spread(G, L, 0.3)
    tol["random_130x67"] = {"spread": s, "bound": max(FACTOR * s, FLOOR)}
    out["rand_G"], out["rand_coords"], out["rand_eps"], out["rand_bound"] = G, c, np.array(0.3), np.array(tol[
        "random_130x67"]["bound"])
    # optimize_damping with three epsilons
    epsilons = np.logspace(0, 2, cfg["epsilon_search_runs"], endpoint=True) * cfg["epsilon"]
    spreads, counts, atols = [], [], []
    for e in epsilons:
        r = dref.optimize(dict(cfg, epsilon=float(e)), *args)
        for gen in r["generations"]:
            assert np.abs(gen["R_diags"] - thresh).min() >= 1e-6, "epsilon %g: diag(R) too close to the threshold" % e
        P = len(r["params"])
        spreads.append(np.linalg.norm(r["R_matrix"] - np.eye(P)) / P)
        counts.append(P)
        # |d spread| <= |dR|_F / P <= max|dR| <= bound * max|R| of the last generation's resolution matrices
        last = r["generations"][-1]
        b = max(max(FACTOR * _spread(last["gfs"][k].T, last["L"], float(e)), FLOOR) for k in range(len(fp["varnames"])))
        atols.append(b * np.abs(r["R_matrix"]).max())
    data = np.vstack((epsilons, np.array(spreads))).T
    theta = 2 * np.pi - np.arctan2(data[:, 1].max() - data[:, 1].min(), data[:, 0].max() - data[:, 0].min())
    rot = data.dot(np.array(((np.cos(theta), -np.sin(theta)), (np.sin(theta), np.cos(theta)))))
    order = np.sort(rot[:, 1])
    assert order[1] - order[0] > 1e-9 * np.abs(rot[:, 1]).max(), "the elbow is a tie"
    out["damp_epsilons"], out["damp_spreads"], out["damp_atol"] = epsilons, np.array(spreads), np.array(atols)
    out["damp_npatches"], out["damp_idx"] = np.array(counts, dtype=np.int64), np.array(int(rot[:, 1].argmin()))
    out["metadata"] = np.array("restated: tests/discretization_ref.py (numpy %s); Green's functions from "
                               "oracle/okada_oracle.py" % np.__version__)
    return out, tol


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    fix, tol = fixture()
    np.savez_compressed(os.path.join(GOLDEN, "discretization_fixture.npz"), **fix)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "discretization_tolerance.json"), "w") as f:
        json.dump(tol, f, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(GOLDEN, "discretization_reference.npz"), **reference_outputs())
    print("generations %d, final P %d, damping optimum %d of %s" % (int(fix["ngen"]), len(fix["params"]),
                                                                  int(fix["damp_idx"]), fix["damp_npatches"].tolist()))
    print(json.dumps(tol["random_130x67"]), max(max(g["spread"]) for g in tol["generations"]))


if __name__ == "__main__":
    main()
