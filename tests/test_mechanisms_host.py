"""Mechanism ensembles without a GPU: the numpy restatement against known points and the 50-digit fixture, csrc/mechanism.hpp
compiled for the host against the same fixture, the focal-sphere grid, the C ABI, the argument rules and the gfx950 compile.

The bounds of the decomposed quantities (BOUND below) are 4 x the worse of the host build of mechanism.hpp and of
``numpy.linalg.eigh`` on tests/golden/mechanisms.npz, floor 8, in units of 2^-53 ||M||_F (eigenvalues, moments, parts) and
of 2^-53 (ratios, (u, v), which carry no scale).  Measured worst cases, host build / numpy:
    eigenvalues 2.68 / 3.93, moments 4.01 / 6.44, parts 3.34 / 5.24, ratios 3.00 / 7.00, (u, v) 3.88 / 6.00."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mechanisms_ref as ref
from conftest import ROOT, load_golden

U = 2.0 ** -53
MEASURED = {"evals": (2.68, 3.93), "moments": (4.01, 6.44), "parts": (3.34, 5.24), "ratios": (3.00, 7.00), "uv": (3.88, 6.00)}
BOUND = dict((k, max(8.0, 4.0 * max(v))) for k, v in MEASURED.items())
SCALED = ("evals", "moments", "parts")      # in units of the tensor's Frobenius norm


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def gold():
    return load_golden("mechanisms")


def frobenius(m6):
    return np.array([np.sqrt(np.sum(ref.symmat6(m) ** 2)) for m in m6])


def units_off(name, got, want, m6):
    """the worst error of every row in the units of BOUND[name]"""
    err = np.abs(np.asarray(got) - np.asarray(want)).reshape(len(m6), -1).max(axis=1) / U
    return err / frobenius(m6) if name in SCALED else err


def restatement(m6):
    out = dict((k, []) for k in MEASURED)
    for m in m6:
        mo, ra, pa = ref.standard_decomposition(m)
        out["evals"].append(np.linalg.eigvalsh(ref.symmat6(m)))
        out["moments"].append(mo)
        out["ratios"].append(ra)
        out["parts"].append(pa)
        out["uv"].append(ref.hudson_of(m))
    return dict((k, np.array(v)) for k, v in out.items())


# ------------------------------------------------------------------------------------------------ the restatement
def test_decomposition_known_points():
    from beat_amd.sources import dc_m6
    dc = dc_m6(30.0, 60.0, -90.0)
    mo, ra, pa = ref.standard_decomposition(dc)
    assert abs(ra[1] - 1.0) < 8 * U and abs(ra[0]) < 8 * U and abs(ra[2]) < 8 * U
    np.testing.assert_allclose(pa[1], dc, rtol=0, atol=8 * U)            # its dc part is the tensor itself
    mo, ra, pa = ref.standard_decomposition([1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    assert ra[0] == 1.0 and ra[1] == 0.0 and ra[3] == 0.0
    mo, ra, pa = ref.standard_decomposition([-1.0, -1.0, 2.0, 0.0, 0.0, 0.0])
    assert abs(ra[2] - 1.0) < 8 * U and abs(ra[1]) < 8 * U and ra[0] == 0.0
    mo, ra, pa = ref.standard_decomposition([1.0, 1.0, 3.0, 0.0, 0.0, 0.0])      # the tensile crack
    np.testing.assert_allclose(ra, [5.0 / 9.0, 0.0, 4.0 / 9.0, 4.0 / 9.0, 1.0], rtol=0, atol=8 * U)
    np.testing.assert_allclose(pa.sum(axis=0) - pa[3] - pa[4], [1.0, 1.0, 3.0, 0.0, 0.0, 0.0], rtol=0, atol=16 * U)


LANDMARKS = [("DC", [1.0, -1.0, 0.0, 0.0, 0.0, 0.0], (0.0, 0.0)),
             ("explosion", [1.0, 1.0, 1.0, 0.0, 0.0, 0.0], (0.0, 1.0)),
             ("implosion", [-1.0, -1.0, -1.0, 0.0, 0.0, 0.0], (0.0, -1.0)),
             ("+CLVD", [-1.0, -1.0, 2.0, 0.0, 0.0, 0.0], (-1.0, 0.0)),
             ("-CLVD", [1.0, 1.0, -2.0, 0.0, 0.0, 0.0], (1.0, 0.0)),
             ("+crack", [1.0, 1.0, 3.0, 0.0, 0.0, 0.0], (-4.0 / 9.0, 5.0 / 9.0)),
             ("+LVD", [1.0, 0.0, 0.0, 0.0, 0.0, 0.0], (-2.0 / 3.0, 1.0 / 3.0))]


def test_hudson_landmarks_and_antisymmetry():
    for name, m, want in LANDMARKS:
        got = ref.hudson_of(m)
        assert max(abs(got[0] - want[0]), abs(got[1] - want[1])) <= 4 * U, (name, got)
    rng = np.random.default_rng(3)
    for m in rng.normal(size=(50, 6)):
        u, v = ref.hudson_of(m)
        u2, v2 = ref.hudson_of(-m)
        assert abs(u + u2) <= 64 * U and abs(v + v2) <= 64 * U
        assert abs(v) <= 1.0 and abs(u) <= 4.0 / 3.0 + 8 * U


def test_restatement_meets_the_fixture(gold):
    m6 = gold["m6"]
    got = restatement(m6)
    for name in MEASURED:
        off = units_off(name, got[name], gold[name], m6)
        i = int(np.argmax(off))
        print("%s: numpy worst %.2f units at row %d (%s)" % (name, off[i], i, gold["labels"][i]))
        assert off[i] <= BOUND[name], (name, off[i], str(gold["labels"][i]))


def test_fixture_holds_the_edges(gold):
    labels = [str(s) for s in gold["labels"]]
    for word in ("random scale 1e-20", "random scale 1", "random scale 1e+20", "dc exact", "dc perturbed 1e-9", "clvd exact",
                 "clvd perturbed 1e-9", "isotropic exact", "isotropic perturbed 1e-9", "two equal eigenvalues", "iso switch",
                 "diagonal"):
        assert any(s.startswith(word) for s in labels), word
    below = [i for i, s in enumerate(labels) if s.startswith("iso switch") and "side -1" in s]
    above = [i for i, s in enumerate(labels) if s.startswith("iso switch") and "side +1" in s]
    assert below and above
    assert np.all(gold["moments"][below, 1] == 0.0) and np.all(gold["moments"][above, 1] > 0.0)     # dc off / on


def test_pixel_counts_and_layout():
    from beat_amd import mechanisms as M
    for res, count in ((3, 5), (4, 4), (65, 3209), (200, 31064)):
        for projection in M.PROJECTIONS:
            amps, takeoff, azimuths, ii_ok, x, y = M.lower_focalsphere_angles(res, projection)
            inside, t, a, xr, yr = ref.focal_grid(res, projection)
            assert ii_ok.sum() == count == takeoff.size == azimuths.size
            assert np.array_equal(ii_ok, inside) and np.array_equal(takeoff, t) and np.array_equal(azimuths, a)
            assert np.all(np.isnan(amps[~ii_ok])) and np.all(amps[ii_ok] == 0.0)
            assert np.all(np.isfinite(takeoff)) and takeoff.max() <= np.pi / 2 + 4 * U and takeoff.min() >= 0.0
            assert np.array_equal(x, np.linspace(-1, 1, res)) and np.array_equal(y, x)
    # resolution 3: the centre pixel looks straight down, the four rim pixels (r^2 == 1) leave horizontally
    _, takeoff, azimuths, ii_ok, x, y = M.lower_focalsphere_angles(3, "lambert")
    assert np.flatnonzero(ii_ok).tolist() == [1, 3, 4, 5, 7] and takeoff[2] == 0.0
    np.testing.assert_allclose(takeoff[[0, 1, 3, 4]], np.pi / 2, rtol=0, atol=2 * U)
    # pixel iy * res + ix is (x[ix], y[iy]); the first coordinate is the east component: azimuth 90 degrees at x = +1
    np.testing.assert_allclose(azimuths, [np.pi, -np.pi / 2, 0.0, np.pi / 2, 0.0], rtol=0, atol=4 * U)
    rw, pix, _, _ = M.focal_sphere(65, "lambert", "any_SH")
    assert rw.shape == (6, 3209) and pix.dtype == np.int64 and np.array_equal(pix, np.flatnonzero(ref.focal_grid(65)[0]))


def test_thin_ensemble_is_the_references():
    from beat_amd import mechanisms as M
    for n, k in ((10, 3), (7, 7), (100000, 1000), (5, 9), (1, 1)):
        assert np.array_equal(M.thin_ensemble(n, k), ref.thin(n, k)) and M.thin_ensemble(n, k).dtype == np.int32
    assert M.thin_ensemble(10, 3).tolist() == [0, 3, 6]


# ------------------------------------------------------------------------------------------------ mechanism.hpp on the host
HOST_MAIN = r"""
#include <cstdio>
#include "mechanism.hpp"
using namespace beatamd;
int main()
{
    double m[6];
    while (scanf("%lf %lf %lf %lf %lf %lf", &m[0], &m[1], &m[2], &m[3], &m[4], &m[5]) == 6) {
        MechDraw r;
        mech_draw(m, r);
        for (int k = 0; k < 3; k++) printf("%.17g ", r.evals[k]);
        for (int k = 0; k < 9; k++) printf("%.17g ", r.evecs[k / 3][k % 3]);
        for (int k = 0; k < 5; k++) printf("%.17g ", r.moments[k]);
        for (int k = 0; k < 5; k++) printf("%.17g ", r.ratios[k]);
        for (int k = 0; k < 30; k++) printf("%.17g ", r.parts[k / 6][k % 6]);
        for (int k = 0; k < 30; k++) printf("%.17g ", r.unit[k / 6][k % 6]);
        printf("%.17g %.17g\n", r.uv[0], r.uv[1]);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("mechanism_host")
    src, exe = d / "main.cpp", d / "mechanism_host"
    src.write_text(HOST_MAIN)
    inc = "-I" + os.path.join(ROOT, "beat_amd", "csrc")
    gxx = shutil.which("g++")
    if gxx:
        cmd = [gxx, "-O2", "-std=c++17", "-ffp-contract=off", inc, str(src), "-o", str(exe)]
    else:
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        cmd = [hipcc, "-x", "c++", "-O2", "-std=c++17", "-ffp-contract=off", inc, str(src), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout

    def run(m6):
        text = "\n".join(" ".join("%.17g" % v for v in row) for row in np.atleast_2d(m6)) + "\n"
        out = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout
        A = np.array([[float(t) for t in line.split()] for line in out.strip().split("\n")])
        return {"evals": A[:, :3], "evecs": A[:, 3:12].reshape(-1, 3, 3), "moments": A[:, 12:17], "ratios": A[:, 17:22],
                "parts": A[:, 22:52].reshape(-1, 5, 6), "unit": A[:, 52:82].reshape(-1, 5, 6), "uv": A[:, 82:84]}
    return run


def test_host_build_meets_the_fixture(gold, host_program):
    m6 = gold["m6"]
    got = host_program(m6)
    for name in MEASURED:
        off = units_off(name, got[name], gold[name], m6)
        i = int(np.argmax(off))
        print("%s: host build worst %.2f units at row %d (%s)" % (name, off[i], i, gold["labels"][i]))
        assert off[i] <= BOUND[name], (name, off[i], str(gold["labels"][i]))


def test_host_build_eigenvectors_units_and_landmarks(gold, host_program):
    m6 = gold["m6"]
    got = host_program(m6)
    fro = frobenius(m6)
    for i, m in enumerate(m6):
        V, w = got["evecs"][i], got["evals"][i]
        assert np.all(np.diff(w) >= 0.0)
        np.testing.assert_allclose(V.T @ V, np.eye(3), rtol=0, atol=32 * U)                       # orthonormal columns
        np.testing.assert_allclose(V @ np.diag(w) @ V.T, ref.symmat6(m), rtol=0, atol=64 * U * fro[i])
        for p in range(5):                                                                     # the unit tensors
            want = ref.unit6(got["parts"][i, p])
            np.testing.assert_allclose(got["unit"][i, p], want, rtol=4 * U, atol=0, equal_nan=True)
    # a diagonal tensor leaves the rotations at once: its eigenvalues are its entries, bit for bit
    d = host_program([[3.0, -1.0, 0.5, 0.0, 0.0, 0.0]])
    assert d["evals"][0].tolist() == [-1.0, 0.5, 3.0]
    assert np.array_equal(np.abs(d["evecs"][0]), np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
    for name, m, want in LANDMARKS:
        uv = host_program([m])["uv"][0]
        assert max(abs(uv[0] - want[0]), abs(uv[1] - want[1])) <= 4 * U, (name, uv)
        uv2 = host_program([[-v for v in m]])["uv"][0]
        assert abs(uv2[0] + uv[0]) <= 4 * U and abs(uv2[1] + uv[1]) <= 4 * U, name


def test_host_build_pure_double_couple(host_program):
    from beat_amd.sources import dc_m6
    m = dc_m6(211.0, 17.0, 143.0)
    got = host_program([m])
    assert abs(got["ratios"][0, 1] - 1.0) <= BOUND["ratios"] * U
    np.testing.assert_allclose(got["parts"][0, 1], m, rtol=0, atol=BOUND["parts"] * U * frobenius([m])[0])


# ------------------------------------------------------------------------------------------------ ABI, argument rules
NEW_ENTRIES = {"beatamd_mt_decompose": 11, "beatamd_fuzzy_amps": 12}


def test_mechanism_entries_are_declared_and_bound():
    from beat_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "beat_amd.h")).read()
    lib = _lib.load()
    for name, arity in NEW_ENTRIES.items():
        m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr)
        assert m, "%s is not declared" % name
        assert len(m.group(1).split(",")) == arity == len(_lib._PROTOS[name]), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for cite in ("beat/plotting/seismic.py:1334-1425", "seismic.py:1664-1850", "seismic.py:2183-2310"):
        assert cite in hdr
    assert lib.beatamd_version() == 120
    mk = open(os.path.join(ROOT, "beat_amd", "csrc", "Makefile")).read()
    assert "mechanisms.hip" in mk and "mechanism.hpp" in mk


def test_argument_rules_need_no_device():
    from beat_amd import mechanisms as M, mechanisms_binding as mb
    mts = np.ones((4, 6))
    for bad in (np.ones(6), np.ones((4, 5)), np.ones((0, 6)), np.ones((2, 3, 6))):
        with pytest.raises(ValueError):
            M.hudson_project(bad)
        with pytest.raises(ValueError):
            M.mts2amps(bad, "lambert", "full", 5)
    with pytest.raises(NotImplementedError, match="top"):
        M.mts2amps(mts, "lambert", "full", 5, view="north")
    with pytest.raises(ValueError, match="mt_type"):
        M.mts2amps(mts, "lambert", "clvd", 5)
    with pytest.raises(ValueError, match="mt_type"):
        M.deco_parts(mts, "iso")
    with pytest.raises(ValueError, match="projection"):
        M.mts2amps(mts, "mercator", "full", 5)
    with pytest.raises(ValueError, match="wavename"):
        M.mts2amps(mts, "lambert", "full", 5, wavename="any_R")
    with pytest.raises(ValueError, match="launch shape"):
        M.mts2amps(mts, "lambert", "full", 5, shape="tall")
    for res in (0, 4097, 2.5):
        with pytest.raises(ValueError, match="grid_resolution"):
            M.mts2amps(mts, "lambert", "full", res)
        with pytest.raises(ValueError, match="grid_resolution"):
            M.decomposition_amps(mts, res)
    with pytest.raises(ValueError):
        M.thin_ensemble(0, 3)
    with pytest.raises(ValueError):
        M.thin_ensemble(5, 0)
    assert mb.check_mts(np.ones((3, 3)))[1:] == (3, mb.KIND_SDR) and mb.check_mts(mts)[1:] == (4, mb.KIND_M6)
    assert (mb.MAX_DRAWS, mb.MAX_RESOLUTION, mb.CHUNK, mb.NPART) == (1 << 24, 4096, 512, 5)
    hpp = open(os.path.join(ROOT, "beat_amd", "csrc", "kernels.hpp")).read()
    assert "MC_CHUNK = 512" in hpp and "MC_MAX_RES = 4096" in hpp and "MC_MAX_N = (int64_t)1 << 24" in hpp


@pytest.mark.skipif(_gpu_present(), reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    from beat_amd import BeatAmdError, mechanisms as M
    mts = np.random.default_rng(7).standard_normal((20, 6))
    calls = [lambda: M.eigensystems(mts), lambda: M.standard_decompositions(mts), lambda: M.deco_parts(mts, "dc"),
             lambda: M.hudson_project(mts), lambda: M.mts2amps(mts, "lambert", "full", 5),
             lambda: M.decomposition_amps(mts, 5)]
    for call in calls:
        with pytest.raises(BeatAmdError):
            call()


KERNELS = ("k_mt_check", "k_mt_decompose", "k_fuzzy_accum", "k_fuzzy_fill", "k_fuzzy_finish")


def test_mechanism_kernels_compile_for_gfx950_without_scratch_or_lds(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "beat_amd", "csrc", "mechanisms.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "mechanisms.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    scratch, lds, name = {}, {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and name:
            lds[name] = int(m.group(1))
    assert len(scratch) == len(KERNELS) + 3, sorted(scratch)      # k_fuzzy_accum: two shapes, count and sum
    for kern in KERNELS:
        hits = [k for k in scratch if kern in k]
        assert hits, "no resource report for %s:\n%s" % (kern, r.stdout[-2000:])
        for k in hits:
            assert scratch[k] == 0 and lds.get(k, 0) == 0, (k, scratch[k], lds.get(k))
