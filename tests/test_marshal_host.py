"""
How ``Context`` marshals its array arguments, pinned on the host with no library and no GPU: a stub library records what
every entry point receives (``ptr`` is the identity here, so it receives the arrays themselves), and every public method
that takes an array is called with the smallest host inputs that are not yet in canonical form (float32, Fortran-ordered
or strided, Python lists, None for the optional ones).  The cases were written against the binding as it stood before
``beat_amd._marshal`` and hold unchanged after it; ``gf_chain_groups`` (it uploads its keys) is a device-only path and
lives in test_gpu_marshal.py.
"""
import ctypes as C

import numpy as np
import pytest

from beat_amd import _lib, engine

f8, i4, i8 = np.float64, np.int32, np.int64
H = "h"          # the context handle the stub library receives


class ANY(object):
    """a ctypes reference or address"""


class A(object):
    """the entry point receives a C-contiguous ``dt`` array with the values (and, unless given, the shape) of ``x``"""

    def __init__(self, x, dt=f8, shape=None):
        self.want = np.asarray(x, dtype=dt) if shape is None else np.asarray(x, dtype=dt).reshape(shape)

    def check(self, got):
        assert isinstance(got, np.ndarray) and got.dtype == self.want.dtype and got.flags.c_contiguous
        assert got.shape == self.want.shape
        np.testing.assert_array_equal(got, self.want)


class O(object):
    """the entry point receives a new C-contiguous host array of this shape and dtype (``zero``: zeroed)"""

    def __init__(self, shape, dt=f8, zero=False):
        self.shape, self.dt, self.zero = tuple(shape), np.dtype(dt), zero

    def check(self, got):
        assert isinstance(got, np.ndarray) and got.dtype == self.dt and got.flags.c_contiguous
        assert got.shape == self.shape and got.flags.writeable
        assert not self.zero or not got.any()


class SAME(object):
    """the entry point receives this very object"""

    def __init__(self, obj):
        self.obj = obj

    def check(self, got):
        assert got is self.obj


def F(*shape, **kw):
    """distinct float32 values in a layout that is not C-contiguous: Fortran order, or a strided view in one dimension"""
    dt = kw.get("dt", np.float32)
    n = int(np.prod(shape))
    if len(shape) == 1:
        a = (np.arange(2 * n) * 0.25 + 1).astype(dt)[::2]
    else:
        a = np.asfortranarray((np.arange(n) * 0.5 + 1).reshape(shape).astype(dt))
    assert n < 2 or not a.flags.c_contiguous or min(shape) == 1
    return a


def K(*shape, **kw):
    """a canonical (C-contiguous float64) array, as the in-place arguments need"""
    return (np.arange(int(np.prod(shape)), dtype=kw.get("dt", f8)) + 2).reshape(shape)


class _Stub(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def ctx(monkeypatch):
    monkeypatch.setattr(engine, "ptr", lambda a: a)
    c = engine.Context.__new__(engine.Context)
    c._lib, c._h, c.device = _Stub(), H, 0
    return c


def _match(got, want):
    if want is ANY:
        return
    if hasattr(want, "check"):
        want.check(got)
    else:
        assert type(got) is type(want) and got == want, (got, want)


def run(ctx, method, args, kwargs, entry, want, ret=None):
    """call, compare the one recorded library call with ``want``; ``ret``: indexes of the call's arguments the method
    returns (one index: that object, a tuple: a tuple of them), or a function that checks the result"""
    ctx._lib.calls[:] = []
    res = getattr(ctx, method)(*args, **kwargs)
    calls = [c for c in ctx._lib.calls if c[0] != "beatamd_ffi_model_nterm"]
    assert [c[0] for c in calls] == [entry]
    got = calls[0][1]
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        _match(g, w)
    if isinstance(ret, int):
        assert res is got[ret]
    elif isinstance(ret, tuple):
        assert isinstance(res, tuple) and len(res) == len(ret)
        for r, i in zip(res, ret):
            assert r is got[i]
    elif ret is not None:
        ret(res, got)
    else:
        assert res is None
    return res, got


def _is(obj):
    return lambda res, got: res is obj or pytest.fail("returned another object")


def _eq(val):
    return lambda res, got: (type(res) is type(val) and res == val) or pytest.fail("returned %r" % (res,))


def _cases():
    """(id, method, args, kwargs, entry, expected arguments, returned)"""
    c = []

    def add(name, method, args, kwargs, entry, want, ret=None):
        c.append(pytest.param(method, args, kwargs, "beatamd_" + entry, want, ret, id=name))

    # -- sweep, libraries, stacking
    s = F(3, 6)
    add("fast_sweep", "fast_sweep_batch", (s, 2, [1, 2, 0], (0, 1, 1), 2, 3), {}, "fast_sweep_batch",
        [H, A(s), 2.0, A([1, 2, 0], i4), A([0, 1, 1], i4), 2, 3, 3, O((3, 6))], 8)
    s1 = F(6)
    add("fast_sweep_1d", "fast_sweep_batch", (s1, 2.5, np.array([1.0]), np.array([0], dtype=i8), 2, 3), {}, "fast_sweep_batch",
        [H, A(s1, shape=(1, 6)), 2.5, A([1], i4), A([0], i4), 2, 3, 1, O((1, 6))], 8)
    g = F(2, 3)
    add("seis_gflib_upload", "seis_gflib_upload", (7, g), {"offset": 5}, "seis_gflib_upload", [H, 7, A(g), 5, 6])
    k = K(2, 3)
    add("seis_gflib_adopt", "seis_gflib_adopt", (7, k), {}, "seis_gflib_adopt", [H, 7, SAME(k)])
    du, st, sl = F(3, 4), F(3, 2, 4), [[1, 2, 3, 4]] * 3
    add("seis_stack_all", "seis_stack_all_batch", (7, (2, 4, 1, 1, 5), du, st, sl), {"interpolation": "multilinear"},
        "seis_stack_all_batch", [H, 7, 3, A(du), A(st), A(sl), 1, O((3, 2, 5))], 7)
    add("geo_gflib_create", "geo_gflib_create", (g,), {}, "geo_gflib_create", [H, 2, 3, A(g), ANY], _eq(0))
    add("geo_stack_all", "geo_stack_all_batch", (7, 5, du), {}, "geo_stack_all_batch", [H, 7, 3, A(du), 0, O((3, 5))], 5)
    o = F(3, 5)      # a caller's out is handed on as it is
    add("geo_stack_all_out", "geo_stack_all_batch", (7, 5, du), {"out": o}, "geo_stack_all_batch", [H, 7, 3, A(du), 1, SAME(o)], 5)
    add("geo_ensemble_create", "geo_ensemble_create", ([[1, 2], [3, 4], [5, 6]], 3, 2), {}, "geo_ensemble_create",
        [H, A([1, 2, 3, 4, 5, 6], i4), 3, 2, ANY], _eq(0))
    v = F(4)
    add("geo_ensemble_stack", "geo_ensemble_stack", (3, 2, 5, v), {}, "geo_ensemble_stack", [H, 3, A(v), O((2, 5))], 3)
    x = F(3, 5)

    # -- weights, priors, noise
    w, lp = F(2, 1), [0.5, 1.5]
    add("weights_create_scalar", "weights_create_scalar", (w, lp, 4), {}, "weights_create",
        [H, 0, 2, 4, A(w, shape=(2,)), A(lp), ANY], _eq(0))
    W = F(2, 3, 3)
    add("weights_create_dense", "weights_create_dense", (W, lp), {}, "weights_create", [H, 1, 2, 3, A(W), A(lp), ANY], _eq(0))
    W2 = F(3, 3)
    add("weights_create_dense_2d", "weights_create_dense", (W2, 0.5), {}, "weights_create",
        [H, 1, 1, 3, A(W2, shape=(1, 3, 3)), A([0.5]), ANY], _eq(0))
    add("weights_update_dense", "weights_update", (4, W, lp), {}, "weights_update", [H, 4, 1, 18, A(W), A(lp)])
    add("weights_update_scalar", "weights_update", (4, [1, 2], lp), {}, "weights_update", [H, 4, 0, 2, A([1, 2]), A(lp)])
    r, hp = F(3, 2, 5), F(3, 2)
    add("mvn_chol_logp", "mvn_chol_logp_batch", (4, r, hp), {}, "mvn_chol_logp_batch", [H, 4, 3, A(r), A(hp), O((3, 2))], 5)
    add("laplacian_create", "laplacian_create", (W2, 2), {}, "laplacian_create", [H, 3, A(W2), 2.0, ANY], _eq(0))
    add("laplacian_logp", "laplacian_logp_batch", (1, du, [1, 2, 3]), {}, "laplacian_logp_batch",
        [H, 1, 3, 4, A(du), A([1, 2, 3]), O((3,))], 6)
    add("autocovariance", "autocovariance_batch", (x,), {}, "autocovariance_batch",
        [H, 3, 5, A(x), A(np.asarray(x, f8).mean(axis=1)), O((3, 5))], 5)
    co, sd = F(2, 4), F(2)
    add("scaled_toeplitz", "scaled_toeplitz_batch", (co, sd), {}, "scaled_toeplitz_batch", [H, 2, 4, A(co), A(sd), O((2, 4, 4))], 5)
    xy, d5 = F(5, 2), F(5)
    add("ball_rms", "ball_rms_batch", (xy, d5, [2, 3], 5), {}, "ball_rms_batch",
        [H, 2, A([2, 3], i8), A(xy), A(d5), 5.0, O((2,)), O((5,), i4), O((5,))], (6, 7, 8))

    # -- the fused model: construction
    lay = _lib.FfiLayout()
    add("ffi_model_create", "ffi_model_create", (lay, [2.0, 3.0], (4, 5), F(2)), {}, "ffi_model_create",
        [H, ANY, 2, A([2, 3], i4), A([4, 5], i4), A(F(2)), ANY], _eq(0))
    add("ffi_model_create_empty", "ffi_model_create", (lay, [], [], []), {}, "ffi_model_create", [H, ANY, 0, None, None, None, ANY],
        _eq(0))
    dat = F(2, 5)
    add("add_wavemap", "ffi_model_add_wavemap", (1, [3.0, 4.0], dat, 2, [5, 6]), {}, "ffi_model_add_wavemap",
        [H, 1, A([3, 4], i4), A(dat), 2, A([5, 6], i8), None, 0])
    add("add_wavemap_shifts", "ffi_model_add_wavemap", (1, [3, 4], dat, 2, [5, 6]),
        {"shift_off": np.array([7, 8], dtype=i4), "interpolation": "multilinear"}, "ffi_model_add_wavemap",
        [H, 1, A([3, 4], i4), A(dat), 2, A([5, 6], i8), A([7, 8], i8), 1])
    sp = F(2, 3)
    add("add_wavemap_spectrum", "ffi_model_add_wavemap_spectrum", (1, [3, 4], sp, 2, [5, 6], 8, (1, 4)), {},
        "ffi_model_add_wavemap_spectrum", [H, 1, A([3, 4], i4), A(sp), 2, A([5, 6], i8), None, 0, 8, 1, 4])
    add("amp_spectrum", "amp_spectrum_batch", (x, 8, (1, 4)), {}, "amp_spectrum_batch",
        [H, 3, 5, 8, 1, 4, A(x), None, 0, O((3, 3))], 9)
    ds, o33 = [[1, 2, 3], [4, 5, 6]], K(3, 3)
    add("amp_spectrum_residual", "amp_spectrum_batch", (x, 8, [1, 4]), {"data_spec": ds, "out": o33}, "amp_spectrum_batch",
        [H, 3, 5, 8, 1, 4, A(x), A(ds), 2, SAME(o33)], 9)
    add("amp_spectrum_residual_f32", "amp_spectrum_batch", (x, 8, [1, 4]), {"data_spec": sp}, "amp_spectrum_batch",
        [H, 3, 5, 8, 1, 4, A(x), A(sp), 2, O((3, 3))], 9)
    d7, w7 = F(7), F(7)
    add("add_geodetic", "ffi_model_add_geodetic", (1, [3, 4], d7, w7, [3.0, 4.0], (5, 6), [0, 1]), {}, "ffi_model_add_geodetic",
        [H, 1, A([3, 4], i4), A(d7), A(w7), 2, A([3, 4], i8), A([5, 6], i4), A([0, 1], i8)])
    po, pf, los = [[0, -1]], F(1, 10), F(7, 3)
    add("add_geodetic_geometry", "ffi_model_add_geodetic_geometry",
        (1, [0], po, pf, d7, w7, los, 0.25, d7, w7, [3, 4], [5, 6], [0, 1]), {}, "ffi_model_add_geodetic_geometry",
        [H, 1, 1, A([0], i4), A(po, i8), A(pf), 7, A(d7), A(w7), A(los), 0.25, A(d7), A(w7), 2, A([3, 4], i8), A([5, 6], i4),
         A([0, 1], i8)])
    B0, B1 = F(4, 2), F(3, 3)
    off = [[0, -1, -1, -1], [2, 3, 4, -1]]
    fix = [[0, 0.5, 0, 0], [0, 0, 0, 0]]
    flat = np.concatenate([np.asarray(B0, f8).ravel(order="F"), np.asarray(B1, f8).ravel(order="F")])
    add("add_corrections", "ffi_model_add_geodetic_corrections", (1, [0, 1], [2, 3], [B0, B1], [[0, -1], [2, 3, 4]],
                                                                 [[0, 0.5], [0, 0, 0]]), {},
        "ffi_model_add_geodetic_corrections", [H, 1, 2, A([0, 1], i4), A([2, 3], i4), A(flat), A(off, i8), A(fix)])
    ea = [[6371e3, 6378e3, 0.003]] * 2
    add("add_corrections_kinds", "ffi_model_add_geodetic_corrections", (1, [0, 1], [2, 3], [B0, B1], [[0, -1], [2, 3, 4]],
                                                                       [[0, 0.5], [0, 0, 0]]),
        {"kind": [0, 1], "earth": np.ravel(ea)}, "ffi_model_add_geodetic_corrections_kinds",
        [H, 1, 2, A([0, 1], i4), A([2, 3], i4), A(flat), A(off, i8), A(fix), A([0, 1], i4), A(ea)])

    # -- the fused model: evaluation
    Q = F(3, 4)
    add("ffi_logp", "ffi_logp_batch", (1, Q, 5), {}, "ffi_logp_batch", [H, 1, 3, A(Q), O((3, 5))], 4)
    add("ffi_logp_out", "ffi_logp_batch", (1, Q, 5), {"out": o}, "ffi_logp_batch", [H, 1, 3, A(Q), SAME(o)], 4)
    add("ffi_synthetics", "ffi_synthetics_batch", (1, 0, Q, 2, 5), {"residuals": 1}, "ffi_synthetics_batch",
        [H, 1, 0, 3, A(Q), 1, O((3, 2, 5))], 6)
    bad = F(3)       # handed on as it is
    add("ffi_start_times", "ffi_start_times_batch", (1, Q, 5), {"chain_bad": bad}, "ffi_start_times_batch",
        [H, 1, 3, A(Q), O((3, 5)), SAME(bad)], 4)
    add("ffi_start_times_out", "ffi_start_times_batch", (1, Q, 5), {"out": o}, "ffi_start_times_batch",
        [H, 1, 3, A(Q), SAME(o), None], 4)
    mps = F(5)
    add("ffi_magnitudes", "ffi_magnitudes_batch", (1, Q, mps, 5), {}, "ffi_magnitudes_batch",
        [H, 1, 3, A(Q), A(mps), None, 0, O((3,)), O((3,))], (7, 8))
    add("ffi_magnitudes_comp", "ffi_magnitudes_batch", (1, Q, [1, 2, 3, 4, 5], 5), {"comp_off": [0.0, 2.0]}, "ffi_magnitudes_batch",
        [H, 1, 3, A(Q), A([1, 2, 3, 4, 5]), A([0, 2], i8), 2, O((3,)), O((3,))], (7, 8))
    add("moment_rate_spans", "ffi_moment_rate_spans_batch", (1, Q, 2, 5, 0.5), {}, "ffi_moment_rate_spans_batch",
        [H, 1, 3, A(Q), None, None, 0.5, O((3, 3, 2), i8)], 7)
    stt, spans = F(3, 5), K(3, 3, 2, dt=i8)
    add("moment_rate_spans_given", "ffi_moment_rate_spans_batch", (1, Q, 2, 5, 1),
        {"start_times": stt, "chain_bad": [0.0, 1.0, 0.0], "out": spans}, "ffi_moment_rate_spans_batch",
        [H, 1, 3, A(Q), A(stt), A([0, 1, 0], i4), 1.0, SAME(spans)], 7)
    add("moment_rates", "ffi_moment_rates_batch", (1, Q, mps, 2, 5, 0.5, -1, 4), {}, "ffi_moment_rates_batch",
        [H, 1, 3, A(Q), A(mps), None, 0, None, None, 0.5, 0, -1, 4, O((3, 3, 4)), None], 13)
    rates = K(3, 3, 4)
    add("moment_rates_given", "ffi_moment_rates_batch", (1, Q, mps, 2, 5, 0.5, -1, 4),
        {"comp_off": (0, 2), "start_times": stt, "chain_bad": np.array([0, 1, 0]), "out": rates, "spans": spans},
        "ffi_moment_rates_batch",
        [H, 1, 3, A(Q), A(mps), A([0, 2], i8), 2, A(stt), A([0, 1, 0], i4), 0.5, 0, -1, 4, SAME(rates), SAME(spans)], 13)

    # -- Metropolis steps
    Q0, L0, acc = K(3, 4), K(3, 5), K(3, dt=i4)
    de, sc, lo, up, lu = F(3, 4), F(3), F(4), [9, 9, 9, 9], F(3)
    add("ffi_astep", "ffi_astep_batch", (1, Q0, L0, de, sc, lo, up, lu, 1), {}, "ffi_astep_batch",
        [H, 1, 3, SAME(Q0), SAME(L0), A(de), A(sc), A(lo), A(up), A(lu), 1.0, O((3,), i4)], 11)
    be = F(3)
    add("ffi_astep_betas", "ffi_astep_batch", (1, Q0, L0, de, sc, lo, up, lu, be), {"accepted": acc}, "ffi_astep_batch_betas",
        [H, 1, 3, SAME(Q0), SAME(L0), A(de), A(sc), A(lo), A(up), A(lu), A(be), SAME(acc)], 11)
    fa = F(2, 4)
    add("ffi_mstep", "ffi_mstep_batch", (1, Q0, L0, fa, None, 0, -1, 2 ** 32 + 5, 0, sc, lo, up, 0.5, acc), {}, "ffi_mstep_batch",
        [H, 1, 3, SAME(Q0), SAME(L0), A(fa), 2, -1, 0, 2 ** 64 - 1, 5, 0, A(sc), A(lo), A(up), 0.5, None, SAME(acc), None, None],
        17)
    asum, nacc = K(1, dt=i8), K(1, dt=i8)
    add("ffi_mstep_univariate", "ffi_mstep_batch", (1, Q0, L0, lo, 2, 3, 7, 1, 4, sc, lo, up, be, acc),
        {"accepted_sum": asum, "n_accepted": nacc}, "ffi_mstep_batch",
        [H, 1, 3, SAME(Q0), SAME(L0), A(lo), 0, 2, 3, 7, 1, 4, A(sc), A(lo), A(up), 1.0, A(be), SAME(acc), SAME(asum), SAME(nacc)],
        17)
    fg = F(3, 2, 4)
    add("ffi_mstep_grouped", "ffi_mstep_batch_grouped", (1, Q0, L0, fg, 0, 7, 1, 4, sc, lo, up, 0.5, acc), {},
        "ffi_mstep_batch_grouped",
        [H, 1, 3, 3, SAME(Q0), SAME(L0), A(fg), 2, 0, 7, 1, 4, A(sc), A(lo), A(up), 0.5, None, SAME(acc), None, None], 17)
    add("ffi_mstep_grouped_betas", "ffi_mstep_batch_grouped", (1, Q0, L0, fg, 0, 7, 1, 4, sc, lo, up, be, acc),
        {"accepted_sum": asum, "n_accepted": nacc}, "ffi_mstep_batch_grouped",
        [H, 1, 3, 3, SAME(Q0), SAME(L0), A(fg), 2, 0, 7, 1, 4, A(sc), A(lo), A(up), 1.0, A(be), SAME(acc), SAME(asum), SAME(nacc)],
        17)
    Qp, inb = K(3, 4), K(3, dt=i4)
    add("metropolis_propose", "metropolis_propose", (Q0, de, sc, lo, up, Qp, inb), {}, "metropolis_propose",
        [H, 3, 4, SAME(Q0), A(de), A(sc), A(lo), A(up), SAME(Qp), SAME(inb)])
    Lp = K(3, 5)
    add("metropolis_accept", "metropolis_accept", (Q0, L0, Qp, Lp, inb, lu, 0.5, acc), {}, "metropolis_accept",
        [H, 3, 4, 5, SAME(Q0), SAME(L0), SAME(Qp), SAME(Lp), SAME(inb), A(lu), 0.5, None, SAME(acc)])
    add("metropolis_tune", "metropolis_tune", (Q0[:, 0], acc, 50), {}, "metropolis_tune", [H, 3, ANY, SAME(acc), 50])

    # -- sampler steps
    lk = F(6)
    add("smc_calc_beta", "smc_calc_beta", (lk, 0.25, 1), {}, "smc_calc_beta", [H, 6, A(lk), 1, 0.25, 1.0, ANY, O((6,))],
        lambda res, got: (res[0] == 0.0 and res[1] is got[7]) or pytest.fail("(beta, weights)"))
    add("smc_calc_beta_strided", "smc_calc_beta", (lk, 0.25, 1), {"stride": 2, "n": 3}, "smc_calc_beta",
        [H, 3, A(lk), 2, 0.25, 1.0, ANY, O((3,))], lambda res, got: res[1] is got[7] or pytest.fail("weights"))
    add("smc_stage_weights", "smc_stage_weights", (lk, 1), {}, "smc_stage_weights", [H, 6, A(lk), 1, 1.0, O((6,))], 5)
    add("smc_resample", "smc_resample", (lk, 1), {}, "smc_resample", [H, 6, A(lk), 1.0, O((6,), i4)], 4)
    add("smc_population_factor", "smc_population_factor", (Q, sc), {}, "smc_population_factor",
        [H, 3, 4, A(Q), A(sc), O((3, 4))], 5)
    add("proposal_draw", "proposal_draw", (fa, 3, -1, 2 ** 32 + 5), {}, "proposal_draw",
        [H, 3, 2, 4, A(fa), 2 ** 64 - 1, 5, 0, 0, O((3, 4)), O((3,))], (9, 10))
    add("proposal_draw_given", "proposal_draw", (fa, 3, 7, 1), {"delta": Qp, "want_log_u": False, "df": 2, "first_chain": 1},
        "proposal_draw", [H, 3, 2, 4, A(fa), 7, 1, 1, 2, SAME(Qp), None], (9, 10))
    add("proposal_draw_grouped", "proposal_draw_grouped", (fg, 3, 7, 1), {}, "proposal_draw_grouped",
        [H, 3, 3, 2, 4, A(fg), 7, 1, 0, 0, O((3, 4)), O((3,))], (10, 11))
    add("proposal_draw_univariate", "proposal_draw_univariate", (1, lo, 3, 7, 1), {}, "proposal_draw_univariate",
        [H, 3, 4, 1, A(lo), 7, 1, 0, O((3, 4)), O((3,))], (8, 9))
    S2 = K(2, 8 + 2 + 4)
    add("group_moments_reset", "group_moments_reset", (S2, 2), {}, "group_moments_reset", [H, 2, 2, SAME(S2), 0, None, None],
        _is(S2))
    Q62, rf = F(6, 2), K(2, 2)
    add("group_moments_reset_ref", "group_moments_reset", (S2, 2), {"Q": Q62, "ref": rf}, "group_moments_reset",
        [H, 2, 2, SAME(S2), 3, A(Q62), SAME(rf)], _is(S2))
    rf32 = F(2, 2)
    add("group_moments_update", "group_moments_update", (S2, Q62, lk, rf32), {"like_stride": 2}, "group_moments_update",
        [H, 2, 3, 2, A(Q62), A(lk), 2, A(rf32), SAME(S2)], _is(S2))
    fac = K(2, 2, 2)
    add("group_moments_factor", "group_moments_factor", (S2, 2, fac), {}, "group_moments_factor",
        [H, 2, 2, SAME(S2), SAME(fac), None, O((2,), i4)],
        lambda res, got: (res[0] is fac and res[1] is None and res[2] is got[6]) or pytest.fail("(factor, cov, flags)"))
    add("group_moments_factor_cov", "group_moments_factor", (S2, 2, fac), {"want_cov": True}, "group_moments_factor",
        [H, 2, 2, SAME(S2), SAME(fac), O((2, 2, 2)), O((2,), i4)],
        lambda res, got: (res[0] is fac and res[1] is got[5] and res[2] is got[6]) or pytest.fail("(factor, cov, flags)"))
    add("gather_rows", "gather_rows", (Q, [2.0, 0.0]), {}, "gather_rows", [H, 2, 4, A(Q), 3, A([2, 0], i4), O((2, 4))], 6)
    add("gather_rows_out", "gather_rows", (Q, np.array([2, 0, 1, 1])), {"out": o}, "gather_rows",
        [H, 4, 4, A(Q), 3, A([2, 0, 1, 1], i4), SAME(o)], 6)

    # -- least-squares start, hyper-parameters
    add("ffi_lsq_normal", "ffi_lsq_normal_batch", (1, Q, 5), {"chain_bad": bad}, "ffi_lsq_normal_batch",
        [H, 1, 3, A(Q), O((3, 5, 5)), O((3, 5)), SAME(bad)], (4, 5))
    N3, b3 = F(3, 2, 2), F(3, 2)
    add("nnls", "nnls_batch", (N3, b3), {}, "nnls_batch", [H, 3, 2, A(N3), A(b3), O((3, 2)), O((3,), i4), O((3,), i4)], (5, 6, 7))
    add("ffi_lsq_solution", "ffi_lsq_solution_batch", (1, Q), {}, "ffi_lsq_solution_batch",
        [H, 1, 3, A(Q), O((3, 4)), O((3,), i4), O((3,), i4)], (4, 5, 6))
    add("ffi_llks", "ffi_llks_batch", (1, Q), {}, "ffi_llks_batch", [H, 1, 3, A(Q), O((3, 0))], 4)
    add("ffi_llks_out", "ffi_llks_batch", (1, Q), {"out": o}, "ffi_llks_batch", [H, 1, 3, A(Q), SAME(o)], 4)
    add("hyper_model_create", "hyper_model_create", (2, [5.0, 6.0], [1, 2], [0, 1], [0, 1], [2]), {}, "hyper_model_create",
        [H, 2, 2, ANY, ANY, ANY, ANY, 1, ANY, ANY], _eq(0))
    Hh, ll = F(3, 2), F(3, 4)
    add("hyper_logp", "hyper_logp_batch", (1, Hh, ll), {}, "hyper_logp_batch", [H, 1, 3, A(Hh), A(ll), O((3, 5))], 5)
    add("hyper_logp_out", "hyper_logp_batch", (1, Hh, ll), {"out": o}, "hyper_logp_batch", [H, 1, 3, A(Hh), A(ll), SAME(o)], 5)
    Hc, LLc, scc, llc, loc, upc, scl = K(3, 2), K(3, 5), K(3), K(3, 4), K(2), K(2), K(2)
    add("hyper_chain", "hyper_chain_batch", (1, 10, Hc, LLc, scc, acc, llc, loc, upc, 0, scl, -1, 2 ** 32 + 5, 0, 50, 50), {},
        "hyper_chain_batch", [H, 1, 3, 10, SAME(Hc), SAME(LLc), SAME(scc), SAME(acc), SAME(llc), SAME(loc), SAME(upc), 0, SAME(scl),
                              2 ** 64 - 1, 5, 0, 50, 50, 1, None, None])
    add("hyper_chain_trace", "hyper_chain_batch", (1, 10, Hc, LLc, scc, acc, llc, loc, upc, 0, scl, 7, 1, 0, 50, 50),
        {"buffer_thinning": 2, "trace": o, "n_accepted": nacc}, "hyper_chain_batch",
        [H, 1, 3, 10, SAME(Hc), SAME(LLc), SAME(scc), SAME(acc), SAME(llc), SAME(loc), SAME(upc), 0, SAME(scl), 7, 1, 0, 50, 50, 2,
         SAME(o), SAME(nacc)])

    # -- posterior diagnostics
    add("wset_quad", "wset_quad_batch", (4, r), {}, "wset_quad_batch", [H, 4, 3, A(r), O((3, 2))], 4)
    add("wset_quad_out", "wset_quad_batch", (4, r), {"out": o}, "wset_quad_batch", [H, 4, 3, A(r), SAME(o)], 4)
    add("ffi_obs_quads", "ffi_obs_quads", (1, 4), {}, "ffi_obs_quads", [H, 1, O((4,))], 2)
    add("ffi_obs_quads_out", "ffi_obs_quads", (1, 4), {"out": o}, "ffi_obs_quads", [H, 1, SAME(o)], 2)
    add("variance_reductions", "ffi_variance_reductions_batch", (1, Q, 2), {}, "ffi_variance_reductions_batch",
        [H, 1, 3, A(Q), O((3, 2))], 4)
    add("variance_reductions_out", "ffi_variance_reductions_batch", (1, Q, 2), {"out": o}, "ffi_variance_reductions_batch",
        [H, 1, 3, A(Q), SAME(o)], 4)
    add("geo_residuals", "ffi_geo_residuals_batch", (1, Q, 7), {}, "ffi_geo_residuals_batch", [H, 1, 3, A(Q), 1, O((3, 7))], 5)
    add("geo_residuals_out", "ffi_geo_residuals_batch", (1, Q, 7), {"residuals": False, "out": o}, "ffi_geo_residuals_batch",
        [H, 1, 3, A(Q), 0, SAME(o)], 5)
    St, Sd = F(2), F(2, 5, 5)
    add("standardize_scalar", "standardize_batch", (St, r), {}, "standardize_batch",
        [H, 0, A(St), 2, 5, 3, A(r), None, O((3, 2, 5))], 8)
    add("standardize_dense", "standardize_batch", (Sd, r), {"hp": hp, "out": o}, "standardize_batch",
        [H, 1, A(Sd), 2, 5, 3, A(r), A(hp), SAME(o)], 8)
    vo, vf, vea = [[0, 1, -1], [2, -1, 3]], F(2, 3), np.ravel(ea)
    add("pole_coefficients", "pole_coefficients_batch", (Q, vo, vf, vea), {}, "pole_coefficients_batch",
        [H, 3, 4, A(Q), 2, A(vo, i8), A(vf), A(ea), O((3, 2, 4))], 8)
    add("pole_coefficients_out", "pole_coefficients_batch", (Q, np.ravel(vo), vf, vea), {"out": o}, "pole_coefficients_batch",
        [H, 3, 4, A(Q), 2, A(vo, i8), A(vf), A(ea), SAME(o)], 8)
    Bp = F(5, 3)
    add("pole_coupling", "pole_coupling_batch", (Q, [0, 1, -1], F(3), ea[0], Bp, 1), {}, "pole_coupling_batch",
        [H, 3, 4, A(Q), A([0, 1, -1], i8), A(F(3)), A(ea[0]), 5, A(Bp), 1, O((3, 5)), O((3, 5))], (10, 11))
    add("ensemble_moments_update", "ensemble_moments_update", (x,), {}, "ensemble_moments_update", [H, 3, 5, A(x), O((5, 5)), 0],
        lambda res, got: (res[0] is got[4] and res[1] == 3) or pytest.fail("(state, rows seen)"))
    st5 = K(5, 5)
    add("ensemble_moments_update_state", "ensemble_moments_update", (x,), {"state": st5, "n_seen": 4}, "ensemble_moments_update",
        [H, 3, 5, A(x), SAME(st5), 4], lambda res, got: (res[0] is st5 and res[1] == 7) or pytest.fail("(state, rows seen)"))
    s55 = F(5, 5)
    add("ensemble_moments_finish", "ensemble_moments_finish", (s55, 7), {}, "ensemble_moments_finish",
        [H, 5, A(s55), 7, O((5,)), O((5,)), O((5,)), O((5,))], (4, 5, 6, 7))

    # -- density grids: a scalar tmin and one extent for every target are broadcast
    Y, ext = F(3, 2, 4), [0, 2, -1.0, 1]
    add("trace_density", "trace_density_update", (Y, 0.5, 0.1, ext), {"grid_size": (6, 5)}, "trace_density_update",
        [H, 3, 2, 4, A(Y), A([0.5, 0.5]), 0.1, A([ext, ext]), 6, 5, 7.0, O((2, 6, 5), zero=True)], 11)
    grid, tm2, ext2 = K(2, 6, 5), F(2), F(2, 4)
    add("trace_density_grid", "trace_density_update", (Y, tm2, 1, ext2), {"grid_size": [6, 5], "linewidth": 3, "grid": grid},
        "trace_density_update", [H, 3, 2, 4, A(Y), A(tm2), 1.0, A(ext2), 6, 5, 3.0, SAME(grid)], 11)
    rg = F(3, 2, 2)
    add("trace_density_ranges", "trace_density_update_ranges", (Y, 0.5, 0.1, np.float32(ext), rg), {"grid_size": (6, 5)},
        "trace_density_update_ranges",
        [H, 3, 2, 4, A(Y), A([0.5, 0.5]), 0.1, A([ext, ext]), A(rg, i8), 6, 5, 7.0, O((2, 6, 5), zero=True)], 12)
    add("trace_density_ranges_none", "trace_density_update_ranges", (Y, 0.5, 0.1, ext, None), {"grid_size": (6, 5)},
        "trace_density_update", [H, 3, 2, 4, A(Y), A([0.5, 0.5]), 0.1, A([ext, ext]), 6, 5, 7.0, O((2, 6, 5), zero=True)], 11)

    # -- geodetic libraries, discretization
    prm, e3, n3 = F(3, 2, 10), F(3), [1, 2, 3]
    add("halfspace_displacements", "halfspace_displacements_batch", ([0.0, 1.0], prm, e3, n3), {}, "halfspace_displacements_batch",
        [H, 3, 2, A([0, 1], i4), A(prm), 3, A(e3), A(n3), 0.25, O((3, 2, 3, 3))], 9)
    p2, lo3, od = F(2, 10), F(3, 3), F(3)
    add("geo_gf_library", "geo_gf_library", (p2, e3, n3, lo3, od), {"nu": 0.3}, "geo_gf_library",
        [H, 2, A(p2), 3, A(e3), A(n3), A(lo3), A(od), 0.3, O((2, 3))], 9)
    pc = F(4, 3)
    add("smoothing_correlated", "smoothing_correlated", (pc,), {"correlation_function": "exponential"}, "smoothing_correlated",
        [H, 4, A(pc), 1, O((4, 4))], 4)
    gfs, L4 = F(4, 3), F(4, 4)
    add("model_resolution", "model_resolution", (gfs, L4, 2), {}, "model_resolution",
        [H, 4, 3, A(gfs), A(L4), 2.0, O((4, 4)), O((4,))], (6, 7))
    w4, dc = F(4), F(3, 2)
    add("division_rating", "division_rating", (w4, w4, pc, w4, 2, dc, w4), {}, "division_rating",
        [H, 4, 3, A(w4), A(w4), A(pc), A(w4), 2.0, A(dc), A(w4), O((4,)), O((4,))], (10, 11))

    # -- covariance operators
    add("chol_inverse", "chol_inverse_batch", (W,), {}, "chol_inverse_batch", [H, 2, 3, A(W), O((2, 3, 3)), O((2,))], (4, 5))
    add("chol_inverse_flags", "chol_inverse_batch_flags", (W,), {}, "chol_inverse_batch_flags",
        [H, 2, 3, A(W), O((2, 3, 3)), O((2,)), O((2,), i4)], (4, 5, 6))
    add("factor_compact", "factor_compact", (F(5, 3),), {}, "factor_compact", [H, 5, 3, A(F(5, 3)), O((3, 3))], 4)
    add("whitening_ratio", "whitening_ratio_batch", (W, W[::-1]), {}, "whitening_ratio_batch",
        [H, 2, 3, A(W), A(W[::-1]), O((2, 3, 3))], 5)
    X23 = K(2, 3)
    add("unwhiten_traces", "unwhiten_traces", (W, X23), {}, "unwhiten_traces", [H, 2, 3, A(W), SAME(X23)], 4)
    add("ffi_model_update_data", "ffi_model_update_data", (1.0, 2.0, dat), {}, "ffi_model_update_data", [H, 1, 2, A(dat)])
    return c


@pytest.mark.parametrize("method,args,kwargs,entry,want,ret", _cases())
def test_host_call(ctx, method, args, kwargs, entry, want, ret):
    run(ctx, method, args, kwargs, entry, want, ret)


def test_every_array_method_is_covered():
    """every public method of Context whose body hands an array over appears above or in one of the tests below"""
    import inspect
    import re
    covered = {p.values[0] for p in _cases()} | {
        "check_correction_kinds", "pred_covariance_batch", "like_assemble", "whiten_rows", "whiten_rows_batch", "set_step_counter",
        "gf_chain_groups"}     # (the last: device only, test_gpu_marshal.py)
    takes_arrays = {name for name, fn in inspect.getmembers(engine.Context, inspect.isfunction)
                    if not name.startswith("_") and re.search(r"\bptr\(", inspect.getsource(fn))}
    assert takes_arrays <= covered, sorted(takes_arrays - covered)


def test_check_correction_kinds():
    kd, ea = engine.Context.check_correction_kinds([2.0, 3.0], (0, 1), [1, 1, 0, 6371e3, 6378e3, 0.003])
    A([0, 1], i4).check(kd)
    A([[1, 1, 0], [6371e3, 6378e3, 0.003]]).check(ea)
    for args, msg in ((([2, 3], [0], [1] * 6), "correction kinds: 1 for 2 terms"),
                      (([2, 3], [0, 1], [1] * 5), "5 values for 2 terms"),
                      (([2, 3], [0, 2], [1] * 6), "unknown kind 2"),
                      (([2, 2], [0, 1], [1] * 6), "has 2 basis columns, not 3"),
                      (([2, 3], [0, 1], [1, 1, 0, 1, -1, 0]), "correction term 1: earth")):
        with pytest.raises(ValueError, match=msg):
            engine.Context.check_correction_kinds(*args)


def test_pred_covariance_pointer_tables(ctx, monkeypatch):
    """the one call that hands over tables of pointers: with the real ``ptr``, read back while the call runs"""
    monkeypatch.setattr(engine, "ptr", _lib.ptr)
    seen = []

    def entry(h, K, nobs, x, nd, n, pb, po):
        tables = [list((C.c_void_p * nd).from_address(p)) for p in (pb, po)]
        seen.append((h, K, nobs, x, nd, list((C.c_int64 * nd).from_address(n)), tables))
        return 0
    ctx._lib.beatamd_pred_covariance_batch = entry
    x = F(3, 5)
    out = ctx.pred_covariance_batch(x, [2.0, 3.0])
    assert isinstance(out, list) and [o.shape for o in out] == [(2, 2), (3, 3)]
    assert all(isinstance(o, np.ndarray) and o.dtype == f8 and o.flags.c_contiguous for o in out)
    assert seen[0][:3] == (H, 3, 5) and seen[0][4:6] == (2, [2, 3])
    assert seen[0][6] == [[None, None], [o.ctypes.data for o in out]]
    b0, o0, o1 = K(2, 2), K(2, 2), K(3, 3)
    res = ctx.pred_covariance_batch(x, (2, 3), base=[b0, None], out=(o0, o1))
    assert isinstance(res, list) and res[0] is o0 and res[1] is o1
    assert seen[1][6] == [[b0.ctypes.data, None], [o0.ctypes.data, o1.ctypes.data]]


def test_tensor_only_methods(ctx):
    """the methods that ask their tensors for ``is_contiguous`` / ``dim``: host tensors stand in for device ones"""
    torch = pytest.importorskip("torch")
    gathered, LL, local = (torch.zeros(shape, dtype=torch.float64) for shape in ((2, 3), (3, 4), (3, 6)))
    _, got = run(ctx, "like_assemble", (gathered, [0.0, -1.0], local, 2, 1, 3, [2, 4], LL), {}, "beatamd_like_assemble",
                 [H, 3, 4, 2, SAME(gathered), ANY, SAME(local), 6, 2, 1, 3, 2, ANY, SAME(LL)], _is(LL))
    run(ctx, "like_assemble", (gathered, [0, 1], None, 0, 0, 0, [2], LL), {}, "beatamd_like_assemble",
        [H, 3, 4, 2, SAME(gathered), ANY, None, 0, 0, 0, 0, 1, ANY, SAME(LL)], _is(LL))
    with pytest.raises(ValueError, match="like_assemble: gathered must be a contiguous"):
        ctx.like_assemble(gathered.t(), [0, 1, 2], None, 0, 0, 0, [2], LL)
    rows, Wb = torch.zeros(2, 3, 4, dtype=torch.float64), F(2, 4, 4)
    run(ctx, "whiten_rows_batch", (rows, Wb), {}, "beatamd_whiten_rows_batch", [H, SAME(rows), 2, 3, 4, A(Wb)], _is(rows))
    with pytest.raises(ValueError, match="rows must be a contiguous"):
        ctx.whiten_rows_batch(rows.transpose(1, 2), Wb)
    with pytest.raises(ValueError, match=r"W must be \(2, 4, 4\)"):
        ctx.whiten_rows_batch(rows, Wb[:1])
    run(ctx, "whiten_rows", (rows[0], Wb[0]), {}, "beatamd_whiten_rows", [H, ANY, 3, 4, A(Wb[0])],
        lambda res, got: tuple(res.shape) == (3, 4) or pytest.fail("rows"))
    cnt = torch.zeros(1, dtype=torch.int32)
    run(ctx, "set_step_counter", (cnt,), {}, "beatamd_ctx_set_step_counter", [H, SAME(cnt)])
    run(ctx, "set_step_counter", (None,), {}, "beatamd_ctx_set_step_counter", [H, None])
    # a host tensor takes the tensor branch of the input rule: handed on as it is, or refused -- never converted
    Qt = torch.zeros(3, 4, dtype=torch.float64)
    run(ctx, "ffi_logp_batch", (1, Qt, 5), {}, "beatamd_ffi_logp_batch", [H, 1, 3, SAME(Qt), O((3, 5))], 4)
    with pytest.raises(ValueError, match="device tensors must be contiguous float64"):
        ctx.ffi_logp_batch(1, Qt.float(), 5)
    with pytest.raises(ValueError, match="device tensors must be contiguous float64"):
        ctx.ffi_logp_batch(1, Qt.t(), 5)


def _errors():
    """(id, method, args, kwargs, exception, message fragment)"""
    Q, S2 = F(3, 4), K(2, 14)
    Y, W = F(3, 2, 4), F(2, 3, 3)
    r = F(3, 2, 5)
    e = [
        ("slowness", "fast_sweep_batch", (F(3, 5), 2, [1], [0], 2, 3), {}, ValueError, "slowness has 5 entries per chain, grid has 6"),
        ("stack_shapes", "seis_stack_all_batch", (7, (2, 4, 1, 1, 5), F(3, 4), F(3, 2, 3), F(3, 4)), {}, ValueError,
         r"stack_all_batch: expected durations/slips \(C,4\) and starttimes \(C,2,4\)"),
        ("interpolation", "seis_stack_all_batch", (7, (2, 4, 1, 1, 5), F(3, 4), F(3, 2, 4), F(3, 4)), {"interpolation": "cubic"},
         NotImplementedError, "Interpolation scheme cubic not implemented!"),
        ("interpolation_wavemap", "ffi_model_add_wavemap", (1, [3], F(1, 5), 2, [5]), {"interpolation": "cubic"},
         NotImplementedError, "Interpolation scheme cubic not implemented!"),
        ("ensemble_ids", "geo_ensemble_create", ([1, 2, 3], 2, 2), {}, ValueError, "3 library ids for 2 variants of 2 variables"),
        ("predcov_X", "pred_covariance_batch", (F(5), [5]), {}, ValueError, r"X must be \(K, Nobs\)"),
        ("predcov_count", "pred_covariance_batch", (F(3, 5), [2, 3]), {"base": [None]}, ValueError, "2 sizes, 1 base and 2 output"),
        ("predcov_base", "pred_covariance_batch", (F(3, 5), [2, 3]), {"base": [F(2, 2), None]}, ValueError,
         r"base\[0\] must be a contiguous float64 \(2, 2\) array"),
        ("predcov_out_shape", "pred_covariance_batch", (F(3, 5), [2, 3]), {"out": [K(2, 2), K(2, 3)]}, ValueError,
         r"out\[1\] must be a contiguous float64 \(3, 3\) array"),
        ("predcov_out_none", "pred_covariance_batch", (F(3, 5), [2, 3]), {"out": [K(2, 2), None]}, ValueError,
         "every dataset needs an output matrix"),
        ("weights_square", "weights_create_dense", (F(2, 3, 4), [0, 0]), {}, ValueError, "weights must be square"),
        ("ball_shapes", "ball_rms_batch", (F(5, 2), F(4), [2, 3], 5), {}, ValueError, r"expected \(5, 2\) and \(5,\)"),
        ("data_spec_add", "ffi_model_add_wavemap_spectrum", (1, [3, 4], F(2, 4), 2, [5, 6], 8, (1, 4)), {}, ValueError,
         r"data_spec must be \(T, 3\)"),
        ("amp_X", "amp_spectrum_batch", (F(5), 8, (1, 4)), {}, ValueError, r"amp_spectrum: X must be \(R, N\)"),
        ("amp_data_spec", "amp_spectrum_batch", (F(3, 5), 8, (1, 4)), {"data_spec": F(2, 4)}, ValueError,
         r"data_spec must be \(2, 3\), got \(2, 4\)"),
        ("amp_out", "amp_spectrum_batch", (F(3, 5), 8, (1, 4)), {"out": F(3, 3)}, ValueError,
         r"out must be a contiguous float64 \(3, 3\) array on Q's side"),
        ("basis", "ffi_model_add_geodetic_corrections", (1, [0], [2], [F(4, 3)], [[0, 1]], [[0, 0]]), {}, ValueError,
         r"correction term 0: basis of shape \(4, 3\), expected \(n, 2\)"),
        ("moment_per_slip", "ffi_magnitudes_batch", (1, Q, F(4), 5), {}, ValueError, r"moment_per_slip must be \(5,\), got \(4,\)"),
        ("moment_per_slip_rates", "ffi_moment_rates_batch", (1, Q, F(4), 2, 5, 0.5, 0, 4), {}, ValueError,
         r"moment_per_slip must be \(5,\), got \(4,\)"),
        ("start_times", "ffi_moment_rate_spans_batch", (1, Q, 2, 5, 0.5), {"start_times": F(3, 4)}, ValueError,
         r"start_times must be \(3, 5\), got \(3, 4\)"),
        ("start_times_rates", "ffi_moment_rates_batch", (1, Q, F(5), 2, 5, 0.5, 0, 4), {"start_times": F(2, 5)}, ValueError,
         r"start_times must be \(3, 5\), got \(2, 5\)"),
        ("chain_bad", "ffi_moment_rate_spans_batch", (1, Q, 2, 5, 0.5), {"chain_bad": [0, 1]}, ValueError,
         r"chain_bad must be \(3,\), got \(2,\)"),
        ("chain_bad_rates", "ffi_moment_rates_batch", (1, Q, F(5), 2, 5, 0.5, 0, 4), {"chain_bad": [0, 1]}, ValueError,
         r"chain_bad must be \(3,\), got \(2,\)"),
        ("spans_shape", "ffi_moment_rate_spans_batch", (1, Q, 2, 5, 0.5), {"out": K(3, 2, 2, dt=i8)}, ValueError,
         r"spans must be a contiguous int64 \(3, 3, 2\) array on Q's side"),
        ("spans_dtype", "ffi_moment_rate_spans_batch", (1, Q, 2, 5, 0.5), {"out": K(3, 3, 2, dt=i4)}, ValueError,
         r"spans must be a contiguous int64 \(3, 3, 2\) array on Q's side"),
        ("spans_layout", "ffi_moment_rates_batch", (1, Q, F(5), 2, 5, 0.5, 0, 4), {"spans": F(3, 3, 2, dt=i8)}, ValueError,
         r"spans must be a contiguous int64 \(3, 3, 2\) array on Q's side"),
        ("rates", "ffi_moment_rates_batch", (1, Q, F(5), 2, 5, 0.5, 0, 4), {"out": K(3, 3, 5)}, ValueError,
         r"rates must be a contiguous float64 \(3, 3, 4\) array on Q's side"),
        ("astep_Q0", "ffi_astep_batch", (1, F(3, 4, dt=f8), K(3, 5), F(3, 4), F(3), F(4), F(4), F(3), 1), {}, ValueError,
         r"Q0 / L0 must be C-contiguous float64 \(updated in place\)"),
        ("astep_L0", "ffi_astep_batch", (1, K(3, 4), K(3, 5).astype(np.float32), F(3, 4), F(3), F(4), F(4), F(3), 1), {}, ValueError,
         r"Q0 / L0 must be C-contiguous float64 \(updated in place\)"),
        ("grouped_factors", "ffi_mstep_batch_grouped", (1, K(3, 4), K(3, 5), F(2, 4), 0, 7, 1, 0, F(3), F(4), F(4), 0.5, K(3, dt=i4)),
         {}, ValueError, r"factors must be \(groups, K, nparams\)"),
        ("draw_grouped_factors", "proposal_draw_grouped", (F(2, 4), 3, 7, 1), {}, ValueError, r"factors must be \(groups, K, nparams\)"),
        ("state_layout", "group_moments_reset", (F(2, 14, dt=f8), 2), {}, ValueError, "group moments: state must be C-contiguous float64"),
        ("state_dtype", "group_moments_update", (F(2, 14), F(6, 2), F(6), K(2, 2)), {}, ValueError,
         "group moments: state must be C-contiguous float64"),
        ("state_shape", "group_moments_factor", (K(2, 13), 2, K(2, 2, 2)), {}, ValueError,
         r"state must be C-contiguous float64 \(groups, 8 \+ nparams \+ nparams\^2\)"),
        ("reset_ref", "group_moments_reset", (S2, 2), {"Q": F(6, 2), "ref": F(2, 2)}, ValueError,
         r"ref must be C-contiguous float64 \(written in place\)"),
        ("reset_Q", "group_moments_reset", (S2, 2), {"Q": F(5, 2), "ref": K(2, 2)}, ValueError,
         r"group_moments_reset: Q \(G \* R, nparams\), ref \(G, nparams\)"),
        ("update_ref", "group_moments_update", (S2, F(6, 2), F(6), K(3, 2)), {}, ValueError,
         r"group_moments_update: Q \(G \* R, nparams\), ref \(G, nparams\)"),
        ("factor_layout", "group_moments_factor", (S2, 2, F(2, 2, 2)), {}, ValueError,
         r"factor must be C-contiguous float64 \(written in place\)"),
        ("factor_shape", "group_moments_factor", (S2, 2, K(2, 2, 3)), {}, ValueError, r"factor must be \(groups, nparams, nparams\)"),
        ("nnls", "nnls_batch", (F(3, 2, 3), F(3, 2)), {}, ValueError, r"nnls_batch: N \(3, 2, 3\) does not match b \(3, 2\)"),
        ("hyper_terms", "hyper_model_create", (2, [5, 6], [1, 2], [0], [0, 1], [2]), {}, ValueError, "one entry per term"),
        ("standardize_r", "standardize_batch", (F(2), F(3, 5)), {}, ValueError, r"residuals must be \(C, T, N\)"),
        ("standardize_S", "standardize_batch", (F(3), r), {}, ValueError, r"S must be \(2,\) or \(2, 5, 5\)"),
        ("standardize_hp", "standardize_batch", (F(2), r), {"hp": F(2, 3)}, ValueError, r"hp must be \(3, 2\)"),
        ("pole_shapes", "pole_coefficients_batch", (Q, [0, 1, 2], F(2, 3), F(3)), {}, ValueError,
         "offsets, fixed values and earth constants differ in shape"),
        ("pole_basis", "pole_coupling_batch", (Q, [0, 1, 2], F(3), F(3), F(5, 2), 1), {}, ValueError,
         r"basis must be \(P, 3\) on Q's side"),
        ("moments_X", "ensemble_moments_update", (F(5),), {}, ValueError, r"X must be \(C, M\)"),
        ("moments_seen", "ensemble_moments_update", (F(3, 5),), {"n_seen": 2}, ValueError, "2 rows seen but no state given"),
        ("moments_state_shape", "ensemble_moments_update", (F(3, 5),), {"state": K(4, 5)}, ValueError,
         r"state must be a contiguous float64 \(5, 5\) array on X's side"),
        ("moments_state_dtype", "ensemble_moments_update", (F(3, 5),), {"state": F(5, 5)}, ValueError,
         r"state must be a contiguous float64 \(5, 5\) array on X's side"),
        ("density_Y", "trace_density_update", (F(3, 4), 0.5, 0.1, [0, 1, 0, 1]), {}, ValueError, r"Y must be \(E, T, N\)"),
        ("density_tmin", "trace_density_update", (Y, [1, 2, 3], 0.1, [0, 1, 0, 1]), {"grid_size": (6, 5)}, ValueError, "broadcast"),
        ("density_grid_shape", "trace_density_update", (Y, 0.5, 0.1, [0, 1, 0, 1]), {"grid_size": (6, 5), "grid": K(2, 5, 6)},
         ValueError, r"grid must be a contiguous float64 \(2, 6, 5\) array on Y's side"),
        ("density_grid_layout", "trace_density_update_ranges", (Y, 0.5, 0.1, [0, 1, 0, 1], F(3, 2, 2)),
         {"grid_size": (6, 5), "grid": F(2, 6, 5)}, ValueError, r"grid must be a contiguous float64 \(2, 6, 5\) array on Y's side"),
        ("density_ranges", "trace_density_update_ranges", (Y, 0.5, 0.1, [0, 1, 0, 1], F(3, 2, 3)), {"grid_size": (6, 5)},
         ValueError, r"trace_density_update: ranges must be \(3, 2, 2\), got \(3, 2, 3\)"),
        ("halfspace_params", "halfspace_displacements_batch", ([0, 1], F(3, 2, 9), F(3), F(3)), {}, ValueError,
         r"params must be \(C, 2, 10\)"),
        ("geolib_params", "geo_gf_library", (F(2, 9), F(3), F(3), F(3, 3), F(3)), {}, ValueError,
         r"params must be \(2, 10\), got \(2, 9\)"),
        ("geolib_los", "geo_gf_library", (F(2, 10), F(3), F(3), F(3, 2), F(3)), {}, ValueError, r"los must be \(3, 3\), got \(3, 2\)"),
        ("correlation", "smoothing_correlated", (F(4, 3),), {"correlation_function": "nearest_neighbor"}, ValueError,
         'does not support "nearest_neighbor" correlation function'),
        ("coords", "smoothing_correlated", (F(4, 2),), {}, ValueError, r"patches_coords must be \(4, 3\), got \(4, 2\)"),
        ("resolution_L", "model_resolution", (F(4, 3), F(4, 3), 2), {}, ValueError, r"L must be \(4, 4\), got \(4, 3\)"),
        ("rating_centers", "division_rating", (F(4), F(4), F(4, 2), F(4), 2, F(3, 2), F(4)), {}, ValueError,
         r"centers must be \(4, 3\), got \(4, 2\)"),
        ("ratio_shapes", "whitening_ratio_batch", (W, F(2, 3, 4)), {}, ValueError, r"W_new and W_old must both be \(nd, n, n\)"),
        ("unwhiten_shapes", "unwhiten_traces", (W, K(2, 4)), {}, ValueError, r"W must be \(nd, n, n\) and X \(nd, n\)"),
        ("unwhiten_dtype", "unwhiten_traces", (W, F(2, 3)), {}, ValueError,
         r"X must be a contiguous float64 array / tensor \(updated in place\)"),
        ("unwhiten_layout", "unwhiten_traces", (W, F(2, 3, dt=f8)), {}, ValueError,
         r"X must be a contiguous float64 array / tensor \(updated in place\)"),
    ]
    return [pytest.param(*row[1:], id=row[0]) for row in e]


@pytest.mark.parametrize("method,args,kwargs,exc,fragment", _errors())
def test_host_refusal(ctx, method, args, kwargs, exc, fragment):
    with pytest.raises(exc, match=fragment):
        getattr(ctx, method)(*args, **kwargs)
    assert ctx._lib.calls == []      # refused before anything reaches the library


# ------------------------------------------------------------------------------------------ beat_amd._marshal itself
def test_marshal_imports_without_torch():
    import os
    import subprocess
    import sys
    code = ("import sys; sys.modules['torch'] = None; import numpy as np; from beat_amd import _marshal as m; "
            "a = m.as_input([[1, 2]], np.int32); assert a.dtype == np.int32 and not m.is_dev(a); "
            "assert m.new(a, (2,), np.int64, zero=True).tolist() == [0, 0]; "
            "assert m.on_side(1, a, np.float64, (2,), 'x', broadcast=True).tolist() == [1.0, 1.0]; "
            "assert m.checked(None, a, (1,), np.float64, 'x').shape == (1,) and m.is_canonical(a, np.int32)")
    subprocess.check_call([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_marshal_as_input_host():
    from beat_amd import _marshal as m
    assert m.as_input(None) is None and m.as_input(None, i4) is None
    k = K(3, 4)
    assert m.as_input(k) is k                                   # canonical: the array itself, no copy
    for dt in (f8, i4, i8):
        src = F(3, 4)
        A(src, dt).check(m.as_input(src, dt))
        A([[1, 2], [3, 4]], dt).check(m.as_input([[1, 2], [3, 4]], dt))
    A([2.5], f8).check(m.as_input(2.5))                         # (numpy.ascontiguousarray gives at least one dimension)
    assert not m.is_dev(k) and not m.is_dev([1.0]) and not m.is_dev(None)


def test_marshal_on_side_host():
    from beat_amd import _marshal as m
    src, ref = F(3, 4), K(2)
    for side in (ref, (False, 0)):
        A(src).check(m.on_side(src, side, f8, (3, 4), "a"))
        A([0, 1, 0], i4).check(m.on_side([0.0, 1.0, 0.0], side, i4, (3,), "a"))
        A([0.5] * 3).check(m.on_side(0.5, side, f8, (3,), "a", broadcast=True))
        A([[1, 2, 3, 4]] * 3).check(m.on_side([1, 2, 3, 4], side, f8, (3, 4), "a", broadcast=True))
        assert m.on_side(None, side, f8, (3,), "a") is None
        with pytest.raises(ValueError, match=r"^a: b must be \(4, 3\), got \(3, 4\)$"):
            m.on_side(src, side, f8, (4, 3), "a: b")
        with pytest.raises(ValueError, match=r"must be \(3,\), got \(1,\)"):
            m.on_side(0.5, side, f8, (3,), "a")                  # no broadcast unless asked for
        with pytest.raises(ValueError, match="broadcast"):
            m.on_side([1, 2], side, f8, (3,), "a", broadcast=True)
    k = K(3, 4)
    assert m.on_side(k, ref, f8, (3, 4), "a") is k


def test_marshal_new_and_checked_host():
    from beat_amd import _marshal as m
    ref = K(2)
    for side in (ref, (False, 0)):
        for dt in (f8, i4, i8):
            O((3, 4), dt).check(m.new(side, (3, 4), dt))
            O((3, 4), dt, zero=True).check(m.new(side, (3, 4), dt, zero=True))
        O((0,)).check(m.new(side, (0,)))
    O((3, 4), i8).check(m.checked(None, ref, (3, 4), i8, "out"))
    O((3, 4), zero=True).check(m.checked(None, ref, (3, 4), f8, "out", zero=True))
    k = K(3, 4)
    assert m.checked(k, ref, (3, 4), f8, "out") is k
    assert m.is_canonical(k) and m.is_canonical(k, f8, (3, 4), ref) and m.is_canonical(K(3, dt=i8), i8)
    for bad in (F(3, 4), F(3, 4, dt=f8), K(4, 3), K(3, 4, dt=i8), k[:, ::2], k.tolist(), None):
        assert not m.is_canonical(bad, f8, (3, 4), ref)
        if bad is not None:
            with pytest.raises(ValueError, match=r"^g: out must be a contiguous float64 \(3, 4\) array on Y's side$"):
                m.checked(bad, ref, (3, 4), f8, "g: out", of="Y")
    with pytest.raises(ValueError, match=r"spans must be a contiguous int64 \(3, 4\) array on Q's side"):
        m.checked(k, ref, (3, 4), i8, "spans")                  # float64 is no int64


def test_marshal_host_tensors():
    """a torch tensor on the host takes the tensor branch of the input rule (handed on or refused, never converted), and
    is host data wherever a side is asked for"""
    torch = pytest.importorskip("torch")
    from beat_amd import _marshal as m
    assert m.torch_dtype(f8) is torch.float64 and m.torch_dtype(i4) is torch.int32 and m.torch_dtype(i8) is torch.int64
    t = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    assert not m.is_dev(t) and m.as_input(t) is t and m.as_input(t.int(), i4).dtype == torch.int32
    for bad, dt in ((t.float(), f8), (t.t(), f8), (t, i4), (t.int(), i8)):
        with pytest.raises(ValueError, match="device tensors must be contiguous %s" % np.dtype(dt).name):
            m.as_input(bad, dt)
    A(t.numpy()).check(m.on_side(t.float().t().contiguous().t(), K(2), f8, (3, 4), "a"))     # converted like any host data
    O((3,)).check(m.new(t, (3,)))                                                          # the host side
    assert m.is_canonical(t) and m.is_canonical(t, f8, (3, 4), K(2)) and not m.is_canonical(t.t()) and not m.is_canonical(t, i8)
    assert m.checked(t, K(2), (3, 4), f8, "out") is t
    up = m.upload(F(3, 4), "cpu")
    assert up.dtype == torch.float32 and up.is_contiguous() and np.array_equal(up.numpy(), F(3, 4))
    up = m.upload(F(3, 4), "cpu", f8)
    assert up.dtype == torch.float64 and np.array_equal(up.numpy(), F(3, 4))
    assert m.upload([1, 2], torch.device("cpu"), i4).dtype == torch.int32
