"""CPU tests of the posterior diagnostics: the numpy restatement (tests/summary_ref.py) against numbers of the reference's
own Covariance arithmetic (tests/golden/summary.npz, tools/gen_golden_summary.py), the ensemble-index rule, the Welford
recurrence (cut into calls anywhere: the same bits; close to a two-pass in extended precision), the C ABI table, no CPU
fallback, and the compiler's resource report of the new kernels."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import summary_ref as sref  # noqa: E402

NEW_ENTRIES = ("beatamd_wset_quad_batch", "beatamd_ffi_obs_quads", "beatamd_ffi_variance_reductions_batch",
               "beatamd_ffi_geo_residuals_batch", "beatamd_standardize_batch", "beatamd_ensemble_moments_update",
               "beatamd_ensemble_moments_finish")


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


# ------------------------------------------------------------------------------------------------- S1 twin vs the reference
def test_s1_variance_reduction_through_chol_inverse_vs_reference(golden):
    """1 - |W r|^2 / |W d|^2 with W = chol_inverse against the reference's 1 - r.icov.r / d.icov.d at three hyper-parameter
    values (exp(2h) cancels): absolute 1e-9 * max(1, nom / denom), the project's composition tolerance"""
    g = golden("summary")
    worst = 0.0
    for key, n in sref.fixture_cases(g):
        W, r, d = g[key + "_chol_inverse"], g[key + "_r"], g[key + "_d"]
        nom, denom, vr = sref.variance_reduction(W, r, d)
        for i, hp in enumerate(g["hps"]):
            ratio = g[key + "_nom"][i] / g[key + "_denom"][i]
            tol = 1e-9 * max(1.0, ratio)
            dev = abs(vr - g[key + "_vr"][i])
            worst = max(worst, dev / tol)
            assert dev <= tol, (key, hp, vr, g[key + "_vr"][i])
            # the quadratic forms themselves, the hyper-parameter scale put back
            np.testing.assert_allclose(nom * np.exp(-2.0 * hp), g[key + "_nom"][i], rtol=1e-9)
            np.testing.assert_allclose(denom * np.exp(-2.0 * hp), g[key + "_denom"][i], rtol=1e-9)
    print("variance reduction, twin vs reference: worst |difference| / tolerance = %.3g" % worst)


def test_s1_standardized_residuals_vs_reference(golden):
    """exp(-h) * inv(cov.chol()) . r against the reference's inv(cov.chol(exp(2h))) . r: 1e-9 of the largest element"""
    from beat_amd.models.problem import _standardizing_operators
    g = golden("summary")
    worst = 0.0
    for key, n in sref.fixture_cases(g):
        S = _standardizing_operators([sref.fixture_covariance(g, key)], n)[0]
        assert np.abs(np.triu(S, 1)).max(initial=0.0) <= 1e-12 * np.abs(S).max()    # lower triangular (to inv's rounding)
        for i, hp in enumerate(g["hps"]):
            z, ref = sref.standardize(S, g[key + "_r"], hp), g[key + "_z_%d" % i]
            tol = 1e-9 * np.abs(ref).max()
            worst = max(worst, float(np.abs(z - ref).max() / tol))
            assert np.all(np.abs(z - ref) <= tol), (key, hp)
    print("standardized residuals, twin vs reference: worst |difference| / tolerance = %.3g" % worst)


def test_s1_standardizing_is_not_whitening(golden):
    """inv(chol(C)) (lower) and chol(inv(C)).T (upper) give products of one norm and different elements: why the engine's
    weight sets cannot serve get_standardized_residuals"""
    g = golden("summary")
    key = "toeplitz_64"
    S = np.linalg.inv(sref.fixture_covariance(g, key).chol())
    W, r = g[key + "_chol_inverse"], g[key + "_r"]
    np.testing.assert_allclose(np.linalg.norm(S @ r), np.linalg.norm(W @ r), rtol=1e-12)
    assert np.abs(S @ r - W @ r).max() > 0.1


def test_s1_scalar_variances_give_scalar_operators():
    from beat_amd.models.problem import _standardizing_operators
    S = _standardizing_operators([4.0, 0.25], 7)
    assert S.shape == (2,) and np.array_equal(S, [0.5, 2.0])


# ------------------------------------------------------------------------------------------------- S2 ensemble indices
def test_s2_ensemble_indices_follow_the_reference_rule(golden):
    from beat_amd.summary import ensemble_indices
    g = golden("summary")
    assert {tuple(c) for c in g["ens_cases"]} == {(10, 4), (530, 7), (5, 5), (3, 5), (4096, 100)}
    for n, e in g["ens_cases"]:
        raw = g["ens_%d_%d" % (n, e)]
        got = ensemble_indices(n, e)
        assert got.dtype == np.int32 and np.array_equal(got, raw[raw < n]), (n, e)
    # the overshoot the docstring speaks of is in the fixture
    assert g["ens_530_7"][-1] == 530 and ensemble_indices(530, 7)[-1] < 530 and ensemble_indices(530, 7).size == 7
    assert ensemble_indices(0, 5).size == 0 and ensemble_indices(5, 0).size == 0


# ------------------------------------------------------------------------------------------------- S3 Welford
def _moment_cases(C, rng):
    M = 37
    return {"unit": rng.standard_normal((C, M)),
            "offset": 1e6 + 1e-3 * rng.standard_normal((C, M)),
            "mixed": rng.standard_normal((C, M)) * 10.0 ** rng.uniform(-3, 3, M)}


@pytest.mark.parametrize("C", [1, 2, 65, 530, 1100])
def test_s3_welford_any_split_is_bitwise_and_close_to_two_pass(C):
    rng = np.random.default_rng(C)
    worst = 0.0
    for name, X in _moment_cases(C, rng).items():
        one, n = sref.welford_update(X)
        assert n == C
        cuts = sorted(set([0, 1, C // 3, C // 2, C - 1, C]) | set(rng.integers(0, C + 1, 3).tolist()))
        state, seen = None, 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            state, seen = sref.welford_update(X[a:b], state, seen)
        assert seen == C and np.array_equal(state, one), name
        mean, std, mn, mx = sref.welford_finish(one, C)
        assert np.array_equal(mn, X.min(0)) and np.array_equal(mx, X.max(0))
        rmean, rstd = sref.two_pass(X)
        bound = sref.moments_bound(X)
        worst = max(worst, float((np.abs(mean - rmean) / bound).max()), float((np.abs(std - rstd) / bound).max()))
        assert np.all(np.abs(mean - rmean) <= bound) and np.all(np.abs(std - rstd) <= bound), name
    print("Welford twin, C = %d: worst |difference| / (C 2^-52 max|x|) = %.3g" % (C, worst))


def test_s3_nan_poisons_mean_and_std_of_its_column_only():
    X = np.random.default_rng(0).standard_normal((9, 4))
    X[3, 2] = np.nan
    mean, std, _, _ = sref.welford_finish(sref.welford_update(X)[0], 9)
    assert np.isnan(mean[2]) and np.isnan(std[2]) and np.isfinite(np.delete(mean, 2)).all()


# ------------------------------------------------------------------------------------------------- S4 ABI
def test_s4_header_entries_are_bound_with_matching_arity():
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


def test_s4_context_and_model_offer_the_methods():
    from beat_amd.engine import Context
    from beat_amd.models import LogpForwFunc
    from beat_amd.models.sharded import TargetShardedLogp
    for n in ("wset_quad_batch", "ffi_obs_quads", "ffi_variance_reductions_batch", "ffi_geo_residuals_batch",
              "standardize_batch", "ensemble_moments_update", "ensemble_moments_finish"):
        assert callable(getattr(Context, n))
    for n in ("obs_quads", "variance_reductions", "geodetic_residuals", "standardized_residuals"):
        assert callable(getattr(LogpForwFunc, n))
        with pytest.raises(NotImplementedError, match="target-sharded"):
            args = {"obs_quads": (), "variance_reductions": (None,), "geodetic_residuals": (None,),
                    "standardized_residuals": (None, None)}[n]
            getattr(TargetShardedLogp, n)(object.__new__(TargetShardedLogp), *args)


# ------------------------------------------------------------------------------------------------- S5 no CPU fallback
@pytest.mark.skipif(_gpu_present(), reason="GPU present")
def test_s5_no_cpu_fallback_without_gpu():
    import beat_amd
    from beat_amd import summary
    from beat_amd.synthetic import SyntheticSpec, build_problem

    class _F(object):       # a compiled model cannot exist without a GPU: the entries fail before they ask it anything
        ndata = 2

        def variance_reductions(self, Q, out=None):
            raise AssertionError("reached the model without a device")

        synthetics = variance_reductions

    pop = np.zeros((5, 3))
    with pytest.raises(beat_amd.BeatAmdError):
        summary.posterior_variance_reductions(_F(), pop)
    with pytest.raises(beat_amd.BeatAmdError):
        summary.result_ensemble(_F(), pop, pop[0], 2)
    with pytest.raises(beat_amd.BeatAmdError):
        beat_amd.get_context(0)
    spec = SyntheticSpec((3,), (3,), (1.0,), T=2, N=8, D=2, S=30, covariance="scalar", geodetic_nobs=(4,))
    prob, _ = build_problem(spec)
    with pytest.raises(beat_amd.BeatAmdError):
        prob.compile()


# ------------------------------------------------------------------------------------------------- S6 resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_s6_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "beat_amd", "csrc", "summary.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "summary.o")],
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
    for kern in ("k_variance_reduction", "k_standardize", "k_ensemble_moments", "k_moments_finish"):
        hits = [v for k, v in seen.items() if kern in k]
        assert hits, "no resource report for %s:\n%s" % (kern, r.stdout[-2000:])
        assert hits == [0] * len(hits), "%s uses scratch: %s" % (kern, hits)
