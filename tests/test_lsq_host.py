"""CPU tests of the least-squares start: the numpy restatement (tests/lsq_ref.py) of the design matrix and of the active
set against the reference's numbers (tests/golden/lsq.npz, tools/gen_golden_lsq.py), the systems of 63 to 1024 unknowns,
the exact tie systems and their hand-written expectations that tests/test_gpu_nnls_edges.py runs on the device, with the
margins of every decision in long double (printed per system), the C ABI table, no CPU fallback, the
compiler's resource report of the kernels, the error texts with stub models, and the samplers' ``start`` argument."""
import functools
import inspect
import os
import re
import shutil
import subprocess
import sys
from collections import OrderedDict
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


# ------------------------------------------------------------------------------------------------- L2 beyond one wavefront
# The systems tests/test_gpu_nnls_edges.py hands to k_nnls (one 64-lane wavefront per chain, every loop strided by 64), each
# checked here on the CPU for the feature it exists for.  name -> (n, seed, rho, frac, noise, rows, feature); the seeds
# are fixed: a seed whose margins missed decision_floor would be replaced, never the floor.
EDGE_SYSTEMS = OrderedDict(
    [("n%d" % n, (n, 1000 + n, 0.0, 0.5, 0.3, None, "support > 64" if n >= 127 else None))
     for n in (63, 64, 65, 127, 128, 129, 200, 400)]
    + [("n65_corr", (65, 2078, 0.45, 0.5, 1.0, None, "removal")),
       ("n129_corr", (129, 2139, 0.45, 0.5, 1.0, None, "removal > 64")),
       ("n200_corr", (200, 2200, 0.45, 0.7, 2.0, None, "removal > 64")),
       ("n400_corr", (400, 2400, 0.45, 0.7, 2.0, None, "removal > 64")),
       ("n1024", (1024, 3000, 0.3, 0.08, 0.5, 1200, "support > 64")),
       # further systems of the chunked launches (the boundary chains hold different systems)
       ("n1024_b", (1024, 4001, 0.3, 0.03, 0.02, 1200, "support > 64")),
       ("n400_b", (400, 5001, 0.45, 0.1, 0.5, None, "removal > 64")),
       ("n400_c", (400, 5002, 0.45, 0.1, 0.5, None, "removal > 64"))])
LANE_STRIDE = tuple("n%d" % n for n in (63, 64, 65, 127, 128, 129, 200, 400)) + ("n65_corr", "n129_corr", "n200_corr",
                                                                                 "n400_corr")
KINDS = ("arg", "tol", "neg", "alpha", "keep")


@functools.lru_cache(maxsize=None)
def edge_system(name):
    """a system of EDGE_SYSTEMS with its three references, computed once per process and left unchanged"""
    from scipy.optimize import nnls
    n, seed, rho, frac, noise, rows, feature = EDGE_SYSTEMS[name]
    A, d = lsq_ref.nnls_system(n, seed, rho, frac, noise, rows)
    Nm, b = A.T @ A, A.T @ d
    x_scipy = nnls(A, d, maxiter=10 * n)[0]
    x_nn, iters, status, removed = lsq_ref.nnls_normal(Nm, b)
    ref = lsq_ref.nnls_margins(Nm, b)
    s = SimpleNamespace(name=name, n=n, A=A, d=d, N=Nm, b=b, x_scipy=x_scipy, x_nn=x_nn, iters=iters, status=status,
                        removed=removed, ref=ref, x_ld=ref["x"], feature=feature, bound=lsq_ref.solution_bound(A, x_scipy),
                        floor=lsq_ref.decision_floor(A, x_scipy), cond=lsq_ref.passive_cond(A, x_scipy))
    for a in (A, d, Nm, b, x_scipy, x_nn, s.x_ld):
        a.setflags(write=False)
    return s


def margin_line(name, ref, floor, cond=float("nan")):
    mg = ref["margins"]
    return ("%-10s iters %4d removed %3d support %4d cond %5.1f | " % (name, ref["iters"], ref["removed"],
                                                                       int((ref["x"] != 0).sum()), cond)
            + " ".join("%s %.1e" % (k, mg[k]) for k in KINDS) + " | floor %.1e solve %.1e" % (floor, ref["solve_err"]))


def check_margins(name, ref, floor):
    """the precondition of a decision-exact comparison: every margin at least decision_floor, and the long-double run's
    own solves accurate to 1e-3 of the smallest margin"""
    smallest = min(ref["margins"].values())
    assert smallest >= floor, (name, ref["margins"], floor)
    assert ref["solve_err"] <= 1e-3 * smallest, (name, ref["solve_err"], smallest)
    return smallest


@pytest.mark.parametrize("name", list(EDGE_SYSTEMS))
def test_l2_edge_systems_hold_their_edges(name):
    """the restatement, scipy's nnls and the long-double run agree on the support, the restatement and the long-double
    run on iters and removals (scipy 1.15 does not report its iterations); both solutions within solution_bound of scipy's;
    every margin above decision_floor; the feature of the case is there.  Measured: margins 2e-7 .. 2e-4 (the smallest
    always `arg` or `tol`) over floors of at most 6e-11, solve errors below 1e-10."""
    s = edge_system(name)
    ref = s.ref
    print(margin_line(name, ref, s.floor, s.cond))
    sup = s.x_scipy != 0
    assert s.status == 0 and ref["status"] == 0
    assert np.array_equal(s.x_nn != 0, sup) and np.array_equal(s.x_ld != 0, sup)
    assert s.iters == ref["iters"] and s.removed == ref["removed"] and s.iters <= 3 * s.n
    assert np.abs(s.x_nn - s.x_scipy).max() <= s.bound and np.abs(s.x_ld - s.x_scipy).max() <= s.bound
    check_margins(name, ref, s.floor)
    assert s.cond < 20.0
    big = sum(k for m, k in ref["events"] if m > 64)
    if s.feature == "support > 64":
        assert sup.sum() > 64 and max(len(ref["entered"]), 0) > 64
    if s.feature == "removal":
        assert s.removed >= 1
    if s.feature == "removal > 64":
        assert s.removed >= 3 and big >= 3, ref["events"]
    if s.n > 64:
        assert max(ref["entered"]) >= 64 and s.iters > 1          # a second trip of the lane-strided loops


def test_l2_generator_is_seeded_and_shaped():
    A, d = lsq_ref.nnls_system(65, 9, 0.45, 0.5, 1.0)
    A2, d2 = lsq_ref.nnls_system(65, 9, 0.45, 0.5, 1.0)
    assert A.shape == (130, 65) and np.array_equal(A, A2) and np.array_equal(d, d2)
    B, _ = lsq_ref.nnls_system(65, 9, 0.0, 0.5, 1.0)
    assert np.array_equal(B * 64, np.round(B * 64)) and np.abs(B).max() <= 127 / 64
    want = B.copy()
    want[:, :-1] += 0.45 * B[:, 1:]
    want[:, 1:] += 0.45 * B[:, :-1]
    assert np.abs(A - want).max() <= 4 * lsq_ref.EPS
    assert lsq_ref.nnls_system(1024, 1, 0.3, 0.08, 0.5, 1200)[0].shape == (1200, 1024)


# first of equals: N = 4 I of size 130 and dyadic b, every operation exact.  kind -> (b, the variables in the order the
# active set must enter them, written down by hand: descending b, the lower index first among equals)
TIE_N = 130


def tie_system(kind):
    n = TIE_N
    if kind == "all_equal":
        b = np.full(n, 1.5)
        order = list(range(n))
    else:
        # distinct multiples of 1/256 in [1, 1.51): 37 is coprime to 130; b[10] = 0 and b[100] < 0 never enter
        b = 1.0 + ((37 * np.arange(n)) % n) / 256.0
        b[10], b[100] = 0.0, -0.5
        top = {"same_lane": (5, 69), "other_lane": (6, 69), "three_trips": (0, 64, 128)}[kind]
        b[list(top)] = 2.0
        rest = [i for i in range(n) if i not in top and i not in (10, 100)]
        order = sorted(top) + sorted(rest, key=lambda i: -b[i])
    return 4.0 * np.eye(n), b, order


TIE_KINDS = ("same_lane", "other_lane", "three_trips", "all_equal")
TIE_HEAD = {"same_lane": [5, 69], "other_lane": [6, 69], "three_trips": [0, 64, 128], "all_equal": [0, 1, 2]}


@pytest.mark.parametrize("kind", TIE_KINDS)
def test_l2_first_of_equals_by_hand(kind):
    """the equal maxima enter in ascending index; under a cap of k solves the support is the first k entered variables
    (the k-th solve still lands in x: the cap is met when variable k + 1 asks for a solve); uncapped x = b / 4 exactly"""
    Nm, b, order = tie_system(kind)
    assert order[:len(TIE_HEAD[kind])] == TIE_HEAD[kind]
    if kind != "all_equal":
        rest = b[order[len(TIE_HEAD[kind]):]]
        assert (b[TIE_HEAD[kind]] == 2.0).all() and (np.diff(rest) < 0).all() and rest[0] < 2.0 and len(order) == 128
    ref = lsq_ref.nnls_margins(Nm, b)
    assert ref["entered"] == order and ref["margins"]["arg"] == 0.0 and ref["removed"] == 0
    for k in (1, 2, 3):
        x, iters, status, removed = lsq_ref.nnls_normal(Nm, b, maxiter=k)
        assert status == 1 and iters == k and sorted(np.nonzero(x)[0]) == sorted(order[:k])
        assert np.array_equal(x[order[:k]], b[order[:k]] / 4.0)
    x, iters, status, removed = lsq_ref.nnls_normal(Nm, b)
    tol = 10.0 * TIE_N * lsq_ref.EPS * np.abs(b).max()
    assert status == 0 and iters == len(order) == int((b > tol).sum()) and removed == 0
    assert np.array_equal(x, np.where(b > tol, b / 4.0, 0.0)) and np.array_equal(ref["x"], x)


# x on the tolerance, exact: a removal step in which two variables leave at once.  Random systems have none (no step of
# the 1200 seeds 2065 .. 2464, 2129 .. 2528 and 2200 .. 2599 of the correlated generator at n = 65, 129 and 200 removes
# two), so this one is built by hand.  n = 130, b[64] = -2^44 sets tol = 1300 2^-52 2^44 = 325 / 64.  Variables p, q, r =
# 70, 5, 129 are coupled through N_PP = U^T U, U = [[2, 0, 3], [0, 2, -12], [0, 0, 4]], b_P = U^T (75, 74, 200) = (150,
# 148, 137); variable k = 3 stands alone with N_kk = 256, b_k = 256 tol = 1300.  Every quantity is a short dyadic number:
#   k enters (w = 1300), x_k = tol; p enters (150), x_p = 37.5; q (148), x_q = 37; r (w_r = 800): s = (tol, -37.5, 337, 50)
#   alpha = 37.5 / 75 = 1/2: x_p = 0, x_k = tol/2 + tol/2 = tol (not above it): both leave; x_q = 187, x_r = 25 stay
#   {q, r} factored again (2, -12; 5): s = (283, 41); w_p = 150 - 6 * 41 = -96; w_k = 1300: k enters again, x_k = tol.
# Six solves, one step that removes two variables, x = (tol, 283, 41) at (3, 5, 129).
def on_tolerance_system():
    n, k, p, q, r = TIE_N, 3, 70, 5, 129
    Nm, b = 4.0 * np.eye(n), np.zeros(n)
    U = np.array([[2.0, 0.0, 3.0], [0.0, 2.0, -12.0], [0.0, 0.0, 4.0]])
    Nm[np.ix_([p, q, r], [p, q, r])] = U.T @ U
    b[[p, q, r]] = U.T @ np.array([75.0, 74.0, 200.0])
    tol = 325.0 / 64.0
    Nm[k, k], b[k], b[64] = 256.0, 256.0 * tol, -2.0 ** 44
    x = np.zeros(n)
    x[[k, q, r]] = tol, 283.0, 41.0
    return Nm, b, x, 6, [k, p, q, r, k]


def test_l2_two_variables_leave_in_one_step_by_hand():
    Nm, b, x_want, iters_want, entered = on_tolerance_system()
    assert 10.0 * TIE_N * lsq_ref.EPS * np.abs(b).max() == 325.0 / 64.0
    assert list(b[[70, 5, 129]]) == [150.0, 148.0, 137.0]
    x, iters, status, removed = lsq_ref.nnls_normal(Nm, b)
    assert status == 0 and iters == iters_want and removed == 2
    assert np.array_equal(x != 0, x_want != 0) and np.abs(x - x_want).max() <= 64 * lsq_ref.EPS * 283.0   # (LAPACK's order)
    ref = lsq_ref.nnls_margins(Nm, b)
    assert ref["events"] == [(4, 2)] and ref["entered"] == entered and ref["iters"] == iters_want
    assert np.array_equal(ref["x"], x_want) and ref["margins"]["keep"] > 1.0 / 337.0


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
