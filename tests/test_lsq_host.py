"""CPU tests of the least-squares start: the numpy restatement (tests/lsq_ref.py) of the design matrix and of the active
set against the reference's numbers (tests/golden/lsq.npz, tools/gen_golden_lsq.py), the C ABI table, no CPU fallback, the
compiler's resource report of the kernels, the error texts with stub models, and the samplers' ``start`` argument."""
import inspect
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
import lsq_ref  # noqa: E402

NEW_ENTRIES = ("beatamd_ffi_model_set_lsq_variables", "beatamd_ffi_lsq_normal_batch", "beatamd_nnls_batch",
               "beatamd_ffi_lsq_solution_batch")
CASES = ("s2x3", "joint3x4", "ml5x7", "s1x17", "two_sub", "geo40", "zero", "positive")


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _chains(golden):
    g = golden("lsq")
    assert tuple(str(n) for n in g["cases"]) == CASES
    for name in CASES:
        case = lsq_ref.load_case(g, name)
        for c in range(case["Q"].shape[0]):
            yield name, case, c


# ------------------------------------------------------------------------------------------------- L1 design matrix
def test_l1_restated_design_matrix_equals_the_reference(golden):
    """nearest neighbour: bit for bit; multilinear: to 1e-12 max|A| (observed: bit for bit, too)"""
    n_ml = 0
    for name, case, c in _chains(golden):
        A, d = lsq_ref.design(case, c)
        ml = any(int(case["wm%d_ml" % w]) for w in range(int(case["nwm"])))
        n_ml += ml
        assert A.shape == case["A"][c].shape
        assert np.array_equal(d, case["d"][c]), (name, c)
        if ml:
            assert np.abs(A - case["A"][c]).max() <= 1e-12 * np.abs(case["A"][c]).max(), (name, c)
        else:
            assert np.array_equal(A, case["A"][c]), (name, c)
    assert n_ml >= 3


def test_l1_fixture_covers_the_shapes(golden):
    g = golden("lsq")
    seen_T, seen_N, hs = set(), set(), []
    for name in CASES:
        case = lsq_ref.load_case(g, name)
        hs += list(case["h"])
        for w in range(int(case["nwm"])):
            T, P, D, S, N = case["wm%d_G" % w].shape
            seen_T.add(T)
            seen_N.add(N)
    assert {1, 3, 4} <= seen_T and {1, 5, 16, 24} <= seen_N
    assert min(hs) <= 0.1 and max(hs) >= 1.5
    assert sorted(int(lsq_ref.load_case(g, n)["P"]) for n in ("s2x3", "joint3x4", "ml5x7", "s1x17")) == [6, 12, 17, 35]
    assert int(lsq_ref.load_case(g, "two_sub")["grids"].shape[0]) == 2 and int(lsq_ref.load_case(g, "two_sub")["nwm"]) == 2
    assert [int(n) for n in lsq_ref.load_case(g, "geo40")["geo_sizes"]] == [20, 20]
    assert not lsq_ref.load_case(g, "zero")["m_ref"].any() and (lsq_ref.load_case(g, "positive")["m_ref"] > 0).all()


# ------------------------------------------------------------------------------------------------- L2 active set
def test_l2_restated_active_set_against_scipy(golden):
    """same support; |m - m_ref|_inf <= 10^3 2^-52 cond_2(A_P)^2 |m_ref|_inf (the normal equations square the condition
    number, 10^3 is the margin); objective within 1e-12 relative of scipy's.  Observed: deviations of at most 4e-14 where
    the bound is 1e-12 to 2e-10."""
    removed_cases = set()
    for name, case, c in _chains(golden):
        A, d, m_ref = case["A"][c], case["d"][c], case["m_ref"][c]
        x, iters, status, removed = lsq_ref.nnls_normal(A.T @ A, A.T @ d)
        assert status == 0 and iters <= 3 * m_ref.size
        assert np.array_equal(x != 0, m_ref != 0), (name, c)
        assert np.abs(x - m_ref).max() <= lsq_ref.solution_bound(A, m_ref), (name, c)
        rn = np.linalg.norm(A @ x - d)
        assert abs(rn - case["rnorm"][c]) <= 1e-12 * case["rnorm"][c], (name, c)
        if removed:
            removed_cases.add(name)
        if name == "zero":
            assert iters == 0 and not x.any()
        if name == "positive":
            ref = np.linalg.solve(A.T @ A, A.T @ d)
            assert (x > 0).all() and np.abs(x - ref).max() <= lsq_ref.solution_bound(A, m_ref)
    assert len(removed_cases) >= 2, removed_cases


def test_l2_restated_active_set_status_words():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((30, 8))
    d = A @ rng.uniform(0.5, 2.0, 8)
    Nm, b = A.T @ A, A.T @ d
    x, iters, status, _ = lsq_ref.nnls_normal(Nm, b, maxiter=2)
    assert status == 1 and iters == 2
    bad = Nm.copy()
    bad[2, 3] = np.nan
    x, iters, status, _ = lsq_ref.nnls_normal(bad, b)
    assert status == 2 and np.isnan(x).all()


# ------------------------------------------------------------------------------------------------- L3 ABI
def test_l3_header_entries_are_bound_with_matching_arity():
    from beat_amd import _lib
    with open(os.path.join(ROOT, "include", "beat_amd.h")) as fh:
        raw = fh.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define BEATAMD_VERSION 120\b", raw) and _lib.ABI_VERSION == 120
    for name in NEW_ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in include/beat_amd.h" % name
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib._PROTOS and name in _lib.EXPORTS, name
        assert len(_lib._PROTOS[name]) == nargs, (name, nargs, len(_lib._PROTOS[name]))
    declared = set(re.findall(r"\b(beatamd_\w+)\s*\(", text))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    # every entry cites the reference lines it restates
    doc = raw[raw.index("replaces: DistributionOptimizer.lsq_solution"):]
    for cite in ("problems.py:753-873", "seismic.py:1351-1507", "base.py:663-709", "geodetic.py:411-427", "problems.py:845-848"):
        assert cite in doc, cite
    lib = os.path.join(ROOT, "beat_amd", "libbeat_amd.so")
    if os.path.exists(lib):
        loaded = _lib.load()
        assert all(hasattr(loaded, n) for n in NEW_ENTRIES)


def test_l3_context_and_models_offer_the_methods():
    from beat_amd.engine import Context
    from beat_amd.models import LogpForwFunc, lsq
    from beat_amd.models.sharded import TargetShardedLogp
    from beat_amd.sampler import SMC, pt_sample, smc_sample
    for n in ("ffi_model_set_lsq_variables", "ffi_lsq_normal_batch", "nnls_batch", "ffi_lsq_solution_batch"):
        assert callable(getattr(Context, n))
    assert callable(LogpForwFunc.lsq_normal_equations) and callable(LogpForwFunc.lsq_solution)
    assert callable(lsq.lsq_start_population)
    for fn in (smc_sample, pt_sample, SMC.initialize_population):
        assert inspect.signature(fn).parameters["start"].default is None
    sh = object.__new__(TargetShardedLogp)
    for call in (lambda: sh.lsq_solution(np.zeros((1, 3))), lambda: sh.lsq_normal_equations(np.zeros((1, 3)))):
        with pytest.raises(NotImplementedError, match="target-sharded"):
            call()


@pytest.mark.skipif(_gpu_present(), reason="GPU present")
def test_l3_no_cpu_fallback_without_gpu():
    import beat_amd
    with pytest.raises(beat_amd.BeatAmdError):
        beat_amd.get_context(0).nnls_batch(np.eye(3)[None], np.ones((1, 3)))


# ------------------------------------------------------------------------------------------------- L4 resources
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_l4_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "beat_amd", "csrc", "lsq.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "lsq.o")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    seen, name = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            seen[name] = int(m.group(1))
    for kern in ("k_lsq_gram", "k_lsq_rhs", "k_nnls"):
        hits = [v for k, v in seen.items() if kern in k]
        assert hits, "no resource report for %s:\n%s" % (kern, r.stdout[-2000:])
        assert hits == [0] * len(hits), "%s uses scratch: %s" % (kern, hits)
    with open(src) as fh:
        assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in fh.read()


# ------------------------------------------------------------------------------------------------- L5 error texts
class _StubCtx(object):
    def __init__(self, status=0):
        self.status, self.calls = status, []

    def ffi_model_set_lsq_variables(self, model_id, inverted, zeroed):
        self.calls.append(("set", inverted, zeroed))

    def ffi_lsq_solution_batch(self, model_id, Q):
        n = Q.shape[0]
        return Q.copy(), np.zeros(n, dtype=np.int32), np.full(n, self.status, dtype=np.int32)


def _stub_model(slip_varnames=("uparr", "uperp"), laplacian=True, prewhitened=False, status=0):
    from beat_amd.models import LogpForwFunc
    f = object.__new__(LogpForwFunc)
    f.ctx, f.model_id, f.nparams, f._dirty = _StubCtx(status), 0, 4, None
    f.problem = SimpleNamespace(laplacian=(np.eye(2), 0.0) if laplacian else None, slip_varnames=list(slip_varnames),
                                wavemaps=[SimpleNamespace(is_prewhitened=prewhitened, name="any_P_0")])
    return f


def test_l5_error_texts():
    Q = np.zeros((2, 4))
    with pytest.raises(ValueError, match="Least-squares- solution for distributed slip is only available with laplacian "
                                         "regularization!"):
        _stub_model(laplacian=False).lsq_solution(Q)
    with pytest.raises(ValueError, match="exactly one of uparr, utens"):
        _stub_model(("uperp",)).lsq_solution(Q)
    with pytest.raises(ValueError, match="exactly one of uparr, utens"):
        _stub_model(("uparr", "utens")).lsq_normal_equations(Q)
    with pytest.raises(ValueError, match="pre-whitened"):
        _stub_model(prewhitened=True).lsq_solution(Q)
    with pytest.raises(RuntimeError, match=r"^Maximum number of iterations reached\.$"):
        _stub_model(status=1).lsq_solution(Q)
    with pytest.raises(ValueError, match="expected 4 parameters"):
        _stub_model().lsq_solution(np.zeros((2, 5)))
    f = _stub_model(("uperp", "utens"))
    out = f.lsq_solution(Q)
    assert np.array_equal(out, Q) and f.ctx.calls == [("set", 1, 0)]
    f.lsq_solution(Q)
    assert f.ctx.calls == [("set", 1, 0)]          # the model is told once


def test_l5_lsq_start_population_draws_the_prior_like_smc():
    from beat_amd.models.lsq import prior_population
    lower, upper = np.array([0.0, -1.0, 2.0]), np.array([5.0, 1.0, 2.5])
    rng = np.random.RandomState(42)
    want = lower + (upper - lower) * rng.random_sample((7, 3))
    assert np.array_equal(prior_population(lower, upper, 7, 42), want)


# ------------------------------------------------------------------------------------------------- L6 start=
def test_l6_start_length_check():
    from beat_amd.sampler.smc import check_start
    with pytest.raises(TypeError, match=r"Argument `start` should have dicts equal the number of chains \(step.N-chains\)"):
        check_start(np.zeros((3, 4)), 5, 4)
    with pytest.raises(ValueError, match="start must be"):
        check_start(np.zeros((5, 3)), 5, 4)
    s = check_start([[1, 2], [3, 4]], 2, 2)
    assert s.dtype == np.float64 and s.flags["C_CONTIGUOUS"] and s.shape == (2, 2)
