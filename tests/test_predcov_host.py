"""CPU tests of the velocity-model prediction covariance: the numpy restatement of the kernels (tests/predcov_ref.py)
against the reference's numbers (tests/golden/pred_cov.npz, tools/gen_golden_predcov.py) and against numpy.cov, its exact
properties, the C ABI table, no CPU fallback, the compiler's resource report of the three kernels, and the update objects'
rules with stub updates."""
import logging
import os
import re
import shutil
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predcov_ref as pref  # noqa: E402

NEW_ENTRIES = ("beatamd_geo_ensemble_create", "beatamd_geo_ensemble_destroy", "beatamd_geo_ensemble_stack",
               "beatamd_pred_covariance_batch")


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _fraction(got, ref, X):
    return float((np.abs(got - ref) / pref.cov_bound(X)).max())


# ------------------------------------------------------------------------------------------------- P1 restatement vs numpy.cov
def test_p1_restatement_vs_fixture_raw_covariance(golden):
    """the kernels' order against the reference's ``num.cov(crust_synths[i], rowvar=0)`` of the small case, element by
    element within 2 * 8 (K + 3) 2^-53 a_i a_j.  Observed: 0.0013 of ONE bound at the worst element (K = 7, datasets of
    1, 30 and 33 points)."""
    g = golden("pred_cov")
    X, sizes = g["small_X"], [int(n) for n in g["small_sizes"]]
    got = pref.pred_covariance(X, sizes)
    worst, o = 0.0, 0
    for i, n in enumerate(sizes):
        raw = g["small_raw%d" % i]
        assert got[i].shape == raw.shape == (n, n)
        frac = _fraction(got[i], raw, X[:, o:o + n])
        worst = max(worst, frac)
        assert frac <= 2.0, (i, frac)
        o += n
    print("restatement vs the fixture's num.cov: worst |difference| / bound = %.3g" % worst)


@pytest.mark.parametrize("K", [6, 12, 40])
def test_p1_restatement_vs_numpy_cov_at_laquila_sizes(K, golden):
    """seeded unit-normal ensembles of the Laquila scenes' sizes (214 and 205 points) against numpy.cov, the reference's
    estimator, within twice the bound.  Observed fractions of ONE bound at the worst element: K = 6: 0.0205, K = 12: 0.0087,
    K = 40: 0.0023."""
    g = golden("pred_cov")
    sizes = [int(n) for n in g["laquila_sizes"]]
    rng = np.random.default_rng(100 + K)
    X = rng.standard_normal((K, sum(sizes)))
    got = pref.pred_covariance(X, sizes)
    worst, o = 0.0, 0
    for i, n in enumerate(sizes):
        frac = _fraction(got[i], np.cov(X[:, o:o + n], rowvar=0), X[:, o:o + n])
        worst = max(worst, frac)
        assert frac <= 2.0, (i, frac)
        o += n
    print("restatement vs numpy.cov, K = %d: worst |difference| / bound = %.3g" % (K, worst))


def test_p1_base_is_added_last_and_null_base_is_zero(golden):
    g = golden("pred_cov")
    X, sizes = g["small_X"], [int(n) for n in g["small_sizes"]]
    base = [g["small_C0"], None, g["small_C2"]]
    raw, tot = pref.pred_covariance(X, sizes), pref.pred_covariance(X, sizes, base)
    assert np.array_equal(tot[0], g["small_C0"] + raw[0]) and np.array_equal(tot[2], g["small_C2"] + raw[2])
    assert np.array_equal(tot[1], raw[1])


# ------------------------------------------------------------------------------------------------- P2 exact properties
@pytest.mark.parametrize("K", [2, 7, 33])
def test_p2_output_is_exactly_symmetric(K):
    rng = np.random.default_rng(K)
    X = rng.standard_normal((K, 70)) * 10.0 ** rng.uniform(-3, 3, 70)
    b = rng.standard_normal((50, 50))
    out = pref.pred_covariance(X, [20, 50], [None, b + b.T])
    for c in out:
        assert np.array_equal(c, c.T)


def test_p2_two_variants():
    """K = 2: cov = (x0 - x1)(x0 - x1)^T / 2 to rounding; K = 1 is refused"""
    rng = np.random.default_rng(2)
    X = rng.standard_normal((2, 9))
    got = pref.pred_covariance(X, [9])[0]
    d = X[0] - X[1]
    np.testing.assert_allclose(got, np.outer(d, d) / 2.0, rtol=0, atol=2.0 * pref.cov_bound(X).max())
    assert np.all(np.abs(got - np.cov(X, rowvar=0)) <= 2.0 * pref.cov_bound(X))
    with pytest.raises(ValueError):
        pref.pred_covariance(X[:1], [9])


def test_p2_constant_column_gives_exactly_zero_row_and_column():
    """a column that is the same in every variant (its K-fold sum exact, as for these values) is centred to exact zeros:
    its row and column of the sample covariance are exactly zero, and the total there is the base"""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((7, 12))
    X[:, 3], X[:, 8] = 3.0, -0.375
    b = rng.standard_normal((12, 12))
    raw = pref.pred_covariance(X, [12])[0]
    for j in (3, 8):
        assert not raw[j].any() and not raw[:, j].any()
    tot = pref.pred_covariance(X, [12], [b])[0]
    assert np.array_equal(tot[3], b[3]) and np.array_equal(tot[:, 8], b[:, 8])


# ------------------------------------------------------------------------------------------------- P3 ABI
def test_p3_header_entries_are_bound_with_matching_arity():
    from beat_amd import _lib
    with open(os.path.join(ROOT, "include", "beat_amd.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in NEW_ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in include/beat_amd.h" % name
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib._PROTOS and name in _lib.EXPORTS, name
        assert len(_lib._PROTOS[name]) == nargs, (name, nargs, len(_lib._PROTOS[name]))
    lib = os.path.join(ROOT, "beat_amd", "libbeat_amd.so")
    if os.path.exists(lib):
        loaded = _lib.load()
        assert all(hasattr(loaded, n) for n in NEW_ENTRIES)


def test_p3_context_and_models_offer_the_methods():
    from beat_amd import covariance, ffi
    from beat_amd.engine import Context
    from beat_amd.models import LogpForwFunc
    from beat_amd.models.sharded import TargetShardedLogp
    for n in ("geo_ensemble_create", "geo_ensemble_destroy", "geo_ensemble_stack", "pred_covariance_batch"):
        assert callable(getattr(Context, n))
    assert callable(LogpForwFunc.update_geodetic_weights) and callable(TargetShardedLogp.update_geodetic_weights)
    for n in ("stack_all", "load", "init_optimization"):
        assert callable(getattr(ffi.GeodeticGFEnsemble, n))
    assert callable(covariance.VelocityModelCovarianceUpdate.update_weights)
    assert callable(covariance.CovarianceUpdates.update_weights)
    # the sharded model forwards to its local (replicated geodetic composite)
    seen = []
    sh = object.__new__(TargetShardedLogp)
    sh.local = SimpleNamespace(update_geodetic_weights=lambda w, s: seen.append((w, s)))
    sh.update_geodetic_weights([1.0], [2.0])
    assert seen == [([1.0], [2.0])]


def _ensemble(K, P=3, nobs=4, varnames=("uparr", "uperp")):
    from beat_amd.ffi import GeodeticGFEnsemble, GeodeticGFLibrary, GeodeticGFLibraryConfig
    libs = {}
    for ci in range(K):
        libs[ci] = {}
        for v in varnames:
            gf = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=(P, nobs), component=v, crust_ind=ci))
            gf.setup(P, nobs, allocate=True)
            libs[ci][v] = gf
    return GeodeticGFEnsemble(libs, varnames)


def test_p3_ensemble_load_reads_the_reference_file_names(tmp_path):
    from beat_amd.ffi import GeodeticGFEnsemble, GFLibraryError, GeodeticGFLibrary, GeodeticGFLibraryConfig
    ens = _ensemble(3)
    rng = np.random.default_rng(0)
    for ci, libs in ens.libraries.items():
        for v, gf in libs.items():
            gf._gfmatrix[:] = rng.standard_normal(gf._gfmatrix.shape)
            gf.save(str(tmp_path))
            assert os.path.exists(str(tmp_path / ("geodetic_%s_static_%d.traces.npy" % (v, ci))))
    back = GeodeticGFEnsemble.load(str(tmp_path), [2, 0, 1], ["uparr", "uperp"])
    assert back.crust_inds == [0, 1, 2] and back.varnames == ["uparr", "uperp"] and back.n_variations == 3
    assert (back.npatches, back.nsamples) == (3, 4) and back.index(2) == 2
    for ci in ens.crust_inds:
        for v in ens.varnames:
            assert np.array_equal(back.libraries[ci][v].get_all(), ens.libraries[ci][v].get_all())
    odd = GeodeticGFLibrary(GeodeticGFLibraryConfig(dimensions=(3, 5)))
    with pytest.raises(GFLibraryError, match="differ in shape"):
        GeodeticGFEnsemble({0: {"uparr": ens.libraries[0]["uparr"]}, 1: {"uparr": odd}})


# ------------------------------------------------------------------------------------------------- P4 no CPU fallback
@pytest.mark.skipif(_gpu_present(), reason="GPU present")
def test_p4_no_cpu_fallback_without_gpu():
    import beat_amd
    ens = _ensemble(7)
    with pytest.raises(beat_amd.BeatAmdError):
        ens.stack_all(np.zeros((2, 3)))
    with pytest.raises(beat_amd.BeatAmdError):
        beat_amd.get_context(0).pred_covariance_batch(np.zeros((7, 4)), [4])


# ------------------------------------------------------------------------------------------------- P5 resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_p5_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "beat_amd", "csrc", "predcov.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "predcov.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    seen = {}
    name = None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    for kern in ("k_crust_stack", "k_pred_center", "k_pred_cov"):
        hits = [v for k, v in seen.items() if kern in k]
        assert hits, "no resource report for %s:\n%s" % (kern, r.stdout[-2000:])
        assert hits == [0] * len(hits), "%s uses scratch: %s" % (kern, hits)


def test_p5_restatement_states_the_kernel_constants():
    with open(os.path.join(ROOT, "beat_amd", "csrc", "predcov.hip")) as fh:
        m = re.search(r"constexpr int PC_TILE = (\d+), PC_KC = (\d+);", fh.read())
    assert m and (int(m.group(1)), int(m.group(2))) == (pref.PC_TILE, pref.PC_KC)


# ------------------------------------------------------------------------------------------------- P6 the update objects' rules
class _StubModel(object):
    """stands where a compiled model stands: anything that reaches the device fails the test"""

    def __init__(self, sizes, varnames):
        self.problem = SimpleNamespace(geodetic=SimpleNamespace(sizes=list(sizes)), slip_varnames=list(varnames))

    def __getattr__(self, name):
        raise AssertionError("the update reached the model (%s)" % name)


def test_p6_five_variants_or_fewer_install_nothing(caplog):
    """geodetic.py:1151-1152, 1191-1195: thresh = 5, `if len(crust_inds) > thresh`"""
    from beat_amd.covariance import VelocityModelCovarianceUpdate
    from beat_amd.heart import Covariance
    covs = [Covariance(data=np.eye(4))]
    for K in (1, 5):
        upd = VelocityModelCovarianceUpdate(_StubModel([4], ["uparr", "uperp"]), _ensemble(K), covs)
        with caplog.at_level(logging.INFO, logger="beat_amd.covariance"):
            upd.update_weights(np.zeros(6))
        assert upd.n_updates == 1 and upd.n_host_route == 0 and not np.any(covs[0].pred_v)
        assert "number of model variations is too low" in caplog.text
    # six variants pass the rule: the update goes on to the model
    upd = VelocityModelCovarianceUpdate(_StubModel([4], ["uparr", "uperp"]), _ensemble(6), covs)
    with pytest.raises(AssertionError, match="reached the model"):
        upd.update_weights(np.zeros(6))


def test_p6_constructor_checks():
    from beat_amd.covariance import VelocityModelCovarianceUpdate
    from beat_amd.heart import Covariance
    covs = [Covariance(data=np.eye(4))]
    ens = _ensemble(7)
    with pytest.raises(ValueError, match="covariances for"):
        VelocityModelCovarianceUpdate(_StubModel([2, 2], ["uparr", "uperp"]), ens, covs)
    with pytest.raises(ValueError, match="slip variables"):
        VelocityModelCovarianceUpdate(_StubModel([4], ["uparr"]), ens, covs)
    with pytest.raises(ValueError, match="observations"):
        VelocityModelCovarianceUpdate(_StubModel([5], ["uparr", "uperp"]), ens, [Covariance(data=np.eye(5))])
    with pytest.raises(ValueError, match="crust variant"):
        VelocityModelCovarianceUpdate(_StubModel([4], ["uparr", "uperp"]), ens, covs, reference_crust_ind=9)


def test_p6_covariance_updates_call_in_order():
    from beat_amd.covariance import CovarianceUpdates
    calls = []

    class _U(object):
        def __init__(self, name, ms):
            self.name, self.last_ms = name, ms

        def update_weights(self, q):
            calls.append((self.name, float(q[0])))

    both = CovarianceUpdates(_U("seismic", 2.0), _U("geodetic", 3.0))
    both.update_weights(np.array([1.0]))
    both.update_weights(np.array([2.0]))
    assert calls == [("seismic", 1.0), ("geodetic", 1.0), ("seismic", 2.0), ("geodetic", 2.0)]
    assert both.n_updates == 2 and both.last_ms == 5.0

    class _Fails(object):
        def update_weights(self, q):
            raise np.linalg.LinAlgError("dataset 0")

    with pytest.raises(np.linalg.LinAlgError):
        CovarianceUpdates(_U("seismic", 1.0), _Fails(), _U("never", 1.0)).update_weights(np.array([3.0]))
    assert calls[-1] == ("seismic", 3.0)


def test_p6_lazy_pred_v_is_downloaded_when_read():
    """a Covariance term left as a device tensor is fetched on first read and kept as numpy"""
    from beat_amd.heart import Covariance

    class _Dev(object):     # the three members of a torch-cuda tensor that the container touches
        is_cuda, fetched = True, 0

        def detach(self):
            return self

        def cpu(self):
            type(self).fetched += 1
            return self

        def numpy(self):
            return 0.5 * np.eye(3)

    cov = Covariance(data=np.eye(3))
    cov.pred_v = _Dev()
    assert _Dev.fetched == 0
    assert np.array_equal(cov.pred_v, 0.5 * np.eye(3)) and isinstance(cov._terms["pred_v"], np.ndarray)
    np.testing.assert_allclose(cov.c_total, 1.5 * np.eye(3))
    assert _Dev.fetched == 1
