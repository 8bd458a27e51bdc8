"""k_nnls (csrc/lsq.hip) beyond one wavefront of unknowns.  The kernel runs Lawson & Hanson's active set with one 64-lane
wavefront per chain and every loop strided by 64; here it meets 63 .. 1024 unknowns: the second and further trips of
those loops, the argmax over more than 64 candidates and its first-of-equals rule, removals from a passive set of more
than 64 variables, the launches NNLS_SCRATCH_BYTES splits a batch into, the passes of lsq_solution, and the limits.

Every system comes from tests/test_lsq_host.py, which checks on the CPU that it holds the edge it is meant to hold and
that every decision of the active set (entry, stop, sign, step length, removal) has a margin of at least
lsq_ref.decision_floor in a long-double run; so iters and the support are compared exactly, the solution against scipy's
nnls and the long-double run within lsq_ref.solution_bound.  The tie systems are exact in float64 and compared bit for bit."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsq_ref  # noqa: E402
import test_lsq_host as cases  # noqa: E402

pytestmark = pytest.mark.gpu

_ALONE = {}


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


def alone(ctx, name):
    """(x, iters, status) of a system of cases.EDGE_SYSTEMS in a batch of one, solved once"""
    if name not in _ALONE:
        s = cases.edge_system(name)
        x, it, st = ctx.nnls_batch(s.N[None], s.b[None])
        _ALONE[name] = (x[0].copy(), int(it[0]), int(st[0]))
    return _ALONE[name]


def check_against_references(s, x, iters, status):
    """status 0, the restatement's iters, scipy's support, within solution_bound of scipy's and the long-double x"""
    assert status == 0 and iters == s.iters, (s.name, status, iters, s.iters)
    assert np.array_equal(x != 0, s.x_scipy != 0), s.name
    worst = max(np.abs(x - s.x_scipy).max(), np.abs(x - s.x_ld).max()) / s.bound
    smallest = min(s.ref["margins"].values())
    print("%s: largest error / bound %.3g, smallest margin / floor %.3g" % (s.name, worst, smallest / s.floor))
    assert worst <= 1.0, (s.name, worst)
    return worst


# ------------------------------------------------------------------------------------------------- lane-stride edges
@pytest.mark.parametrize("name", cases.LANE_STRIDE)
def test_lane_stride_edges(ctx, name):
    """n = 63 .. 400 uncorrelated (no removals: the entering path alone) and n = 65 .. 400 with correlated neighbours
    (removals, from more than 64 passive variables at n >= 129)"""
    check_against_references(cases.edge_system(name), *alone(ctx, name))


# ------------------------------------------------------------------------------------------------- the limits
def test_1024_unknowns(ctx):
    """NNLS_MAX_N: 57344 B of LDS, sixteen trips of every lane-strided loop"""
    check_against_references(cases.edge_system("n1024"), *alone(ctx, "n1024"))


def test_1025_unknowns_are_refused_and_the_context_stays_usable(ctx):
    s = cases.edge_system("n129_corr")
    x0, it0, st0 = ctx.nnls_batch(s.N[None], s.b[None])
    with pytest.raises(ValueError, match="1025 unknowns"):
        ctx.nnls_batch(np.eye(1025)[None], np.ones((1, 1025)))
    x1, it1, st1 = ctx.nnls_batch(s.N[None], s.b[None])
    assert np.array_equal(x1, x0) and np.array_equal(it1, it0) and np.array_equal(st1, st0) and st1[0] == 0


# ------------------------------------------------------------------------------------------------- first of equals, exact
@pytest.mark.parametrize("kind", cases.TIE_KINDS)
def test_first_of_equals(ctx, kind, monkeypatch):
    """N = 4 I (130), dyadic b with equal maxima in one lane (5, 69), across lanes with the lower index in the higher lane
    (69, 6), in three trips of one lane (0, 64, 128) and everywhere: under a cap of k solves the support is the first k
    variables of the order written down in test_lsq_host.py; uncapped x = b / 4 bit for bit"""
    Nm, b, order = cases.tie_system(kind)
    for k in (1, 2, 3):
        monkeypatch.setenv("BEATAMD_NNLS_MAXITER", str(k))
        x, it, st = ctx.nnls_batch(Nm[None], b[None])
        xr, itr, str_, _ = lsq_ref.nnls_normal(Nm, b, maxiter=k)
        assert st[0] == 1 and str_ == 1 and it[0] == k == itr
        assert np.nonzero(x[0])[0].tolist() == sorted(order[:k]), (kind, k, np.nonzero(x[0])[0], order[:k])
        assert np.array_equal(x[0], xr)
    monkeypatch.delenv("BEATAMD_NNLS_MAXITER")
    x, it, st = ctx.nnls_batch(Nm[None], b[None])
    tol = 10.0 * b.size * lsq_ref.EPS * np.abs(b).max()
    assert st[0] == 0 and it[0] == int((b > tol).sum()) == len(order)
    assert np.array_equal(x[0], np.where(b > tol, b / 4.0, 0.0))


def test_two_variables_leave_in_one_step(ctx):
    """the hand-built exact system of test_lsq_host.py: an interpolated x that lands on the tolerance leaves (x <= tol)
    together with the variable that set the step; it enters again, which the count of solves shows"""
    Nm, b, x_want, iters_want, _ = cases.on_tolerance_system()
    x, it, st = ctx.nnls_batch(Nm[None], b[None])
    assert st[0] == 0 and it[0] == iters_want, (st[0], it[0])
    assert np.array_equal(x[0], x_want), np.nonzero(x[0] != x_want)


# ------------------------------------------------------------------------------------------------- chunked launches
def _stacked(ctx, names, C):
    systems = [cases.edge_system(n) for n in names]
    pick = [c % len(names) for c in range(C)]
    Nm = np.stack([systems[i].N for i in pick])
    b = np.stack([systems[i].b for i in pick])
    return Nm, b, [names[i] for i in pick]


def _check_chains_equal_alone(ctx, x, it, st, which, skip=()):
    for c, name in enumerate(which):
        if c in skip:
            continue
        xa, ita, sta = alone(ctx, name)
        assert it[c] == ita and st[c] == sta and np.array_equal(x[c], xa), (c, name, it[c], ita, st[c], sta)


@pytest.mark.parametrize("C", (32, 33, 65))
def test_chunked_launches_at_1024_unknowns(ctx, C):
    """32 chains per launch at n = 1024: one, two and three launches; the chains on either side of a boundary hold
    different systems; every chain bit for bit what it is alone"""
    names = ("n1024", "n1024_b")
    for name in names[1:]:
        check_against_references(cases.edge_system(name), *alone(ctx, name))
    Nm, b, which = _stacked(ctx, names, C)
    assert C <= 32 or which[31] != which[32]
    x, it, st = ctx.nnls_batch(Nm, b)
    _check_chains_equal_alone(ctx, x, it, st, which)


def test_chunked_launches_at_400_unknowns_and_a_nan_chain_in_the_second(ctx):
    """209 chains per launch at n = 400: C = 210 puts one chain into a second launch; then the same batch with a NaN in
    chain 209 (the second launch): flagged 2 alone"""
    names = ("n400_corr", "n400_b", "n400_c")
    for name in names[1:]:
        check_against_references(cases.edge_system(name), *alone(ctx, name))
    Nm, b, which = _stacked(ctx, names, 210)
    assert which[208] != which[209]
    x, it, st = ctx.nnls_batch(Nm, b)
    _check_chains_equal_alone(ctx, x, it, st, which)
    Nm[209, 7, 300] = np.nan
    x, it, st = ctx.nnls_batch(Nm, b)
    assert st[209] == 2 and np.isnan(x[209]).all() and not st[:209].any()
    _check_chains_equal_alone(ctx, x, it, st, which, skip=(209,))


# ------------------------------------------------------------------------------------------------- the model's path
def _check_chain_against_scipy(case, c, m, what):
    """precondition first: every margin of the long-double run on numpy's normal equations above decision_floor; then
    scipy's support and |m - m_scipy| <= solution_bound"""
    from scipy.optimize import nnls
    A, d = lsq_ref.design(case, c)
    m_scipy = nnls(A, d, maxiter=10 * A.shape[1])[0]
    ref = lsq_ref.nnls_margins(A.T @ A, A.T @ d)
    floor = lsq_ref.decision_floor(A, m_scipy)
    print(cases.margin_line("%s[%d]" % (what, c), ref, floor, lsq_ref.passive_cond(A, m_scipy)))
    cases.check_margins((what, c), ref, floor)
    assert np.array_equal(ref["x"] != 0, m_scipy != 0), (what, c)
    bound = lsq_ref.solution_bound(A, m_scipy)
    assert np.array_equal(m != 0, m_scipy != 0), (what, c)
    err = np.abs(m - m_scipy).max()
    print("%s[%d]: error / bound %.3g" % (what, c, err / bound))
    assert err <= bound, (what, c, err, bound)
    return ref


@pytest.mark.parametrize("shape", [((5, 13, 0.5), "nearest_neighbor"), ((10, 13, 0.5), "multilinear")],
                         ids=["P65_nn", "P130_ml"])
def test_model_path_past_64_patches(ctx, shape):
    grid, interp = shape
    P = grid[0] * grid[1]
    case = lsq_ref.synthetic_case(grid, 2, 64, interp, 3, seed=300 + P)
    prob, lay = lsq_ref.build_problem(case)
    f = prob.compile(ctx)
    try:
        Q = case["Q"]
        out, it, st = f.lsq_solution(Q, return_info=True)
        x, it2, st2 = ctx.nnls_batch(*f.lsq_normal_equations(Q))
        sl, up = lay.offsets["uparr"], lay.offsets["uperp"]
        assert not st.any() and np.array_equal(it, it2) and np.array_equal(st, st2)
        assert np.array_equal(out[:, sl:sl + P], x)
        rest = np.ones(Q.shape[1], dtype=bool)
        rest[sl:sl + P] = rest[up:up + P] = False
        assert np.array_equal(out[:, rest], Q[:, rest]) and not out[:, up:up + P].any()
        case["st0"] = f.start_times(Q)
        for c in range(Q.shape[0]):
            ref = _check_chain_against_scipy(case, c, out[c, sl:sl + P], "P%d" % P)
            assert it[c] == ref["iters"], (c, it[c], ref["iters"])
    finally:
        f.release()


def test_pass_boundary_of_lsq_solution(ctx):
    """a pass of lsq_solution holds floor(2^30 / (8 P^2)) chains: 7941 at P = 130.  C = 7945 (T = 1, N = 5): chain 0, the
    last chain of the first pass (7940), the first of the second (7941) and the chains 7942, 7943 and 7944 equal their
    solutions alone bit for bit and scipy's within the bound.  Measured on the MI355X: 0.29 s for the 7945 chains, 0.8 s
    for the test, so the shape stays."""
    grid, P, C = (10, 13, 0.5), 130, 7945
    per_pass = (1 << 30) // (8 * P * P)
    assert per_pass == 7941
    case = lsq_ref.synthetic_case(grid, 1, 5, "nearest_neighbor", C, seed=777)
    prob, lay = lsq_ref.build_problem(case)
    f = prob.compile(ctx)
    try:
        Q = case["Q"]
        t0 = time.perf_counter()
        out, it, st = f.lsq_solution(Q, return_info=True)
        print("lsq_solution of %d chains at P = %d: %.2f s" % (C, P, time.perf_counter() - t0))
        assert not st.any()
        sl = lay.offsets["uparr"]
        case["st0"] = f.start_times(Q)
        for c in (0, per_pass - 1, per_pass, 7942, 7943, 7944):
            o1, it1, st1 = f.lsq_solution(Q[c:c + 1], return_info=True)
            assert np.array_equal(o1[0], out[c]) and it1[0] == it[c] and st1[0] == 0, c
            ref = _check_chain_against_scipy(case, c, out[c, sl:sl + P], "pass")
            assert it[c] == ref["iters"], (c, it[c], ref["iters"])
    finally:
        f.release()
