"""The paths the model evaluator's shared builders take (csrc/model.cpp): which stacking kernel the synthetics entry and
the likelihood launch for the smoke problem, and that the entry points which evaluate a part of the model -- residuals of a
wavemap, geodetic residuals, the Laplacian -- give bit for bit what the likelihood makes of the same part."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C = 64   # one candidate chain-group size: nothing is chosen by timing

# ctx.last_kernel() and ctx.gf_plan()["plan"] after f.synthetics(Q) and after f.batch(Q), recorded by running `_observe`
# below on the commit before the evaluator moved out of capi.cpp (f13a94f) on an MI355X: the synthetics entry builds its
# index tables per target and reads float64 rows, the likelihood shares tables between the targets of a station.  The
# context is this module's own: the likelihood's row buffers are sized from the launch before it (the synthetics call)
EXPECTED = {
    "synthetics": ("k_gfstack_dma<1,1,0,64,1>",
                   "lane <-> chain kernel with 64-chain groups (small batch): row buffers of 64 slots"),
    "batch": ("k_gfstack_dma<1,1,2,64,1>",
              "lane <-> chain kernel with 64-chain groups (small batch): row buffers of 64 slots sized by the previous "
              "launch's distinct-row count"),
}


@pytest.fixture(scope="module")
def ctx():
    from beat_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model(ctx):
    """the smoke problem (``__graft_entry__.smoke``), compiled once; Q [64, nparams], its likelihood vectors LL"""
    from beat_amd.synthetic import SyntheticSpec, build_problem, draw_population
    spec = SyntheticSpec((6,), (5,), (1.0,), T=4, N=128, D=3, S=25, covariance="toeplitz", station_shifts=True,
                         geodetic_nobs=(12,), laplacian=True)
    prob, host = build_problem(spec)
    f = prob.compile(ctx)
    Q = draw_population(spec, host["layout"], host["lower"], host["upper"], C)
    seen = _observe(ctx, f, Q)
    yield dict(spec=spec, prob=prob, host=host, f=f, Q=Q, seen=seen, LL=np.asarray(f.batch(Q)))
    f.release()


def _observe(ctx, f, Q):
    seen = {}
    f.synthetics(Q)
    seen["synthetics"] = (ctx.last_kernel(), ctx.gf_plan()["plan"])
    f.batch(Q)
    seen["batch"] = (ctx.last_kernel(), ctx.gf_plan()["plan"])
    return seen


def test_a_kernels_and_plans_are_the_recorded_ones(model):
    for k, v in model["seen"].items():
        print("%s: last_kernel %r\n    plan %r" % (k, v[0], v[1]))
    assert model["seen"] == EXPECTED


def test_b_wavemap_residuals_are_data_minus_synthetics(model):
    f, Q = model["f"], model["Q"]
    syn, res = f.synthetics(Q), f.synthetics(Q, residuals=True)
    assert syn.shape == (C, 4, 128)
    assert np.array_equal(res, model["prob"].wavemaps[0].data[None] - syn)


def test_c_geodetic_columns_from_the_residual_entry(ctx, model):
    """f.geodetic_residuals -> wset_quad_batch / the MVN epilogue per dataset = the geodetic columns of f.batch and of
    f.update_llks"""
    f, Q, prob = model["f"], model["Q"], model["prob"]
    g, lay = prob.geodetic, prob.layout
    res = f.geodetic_residuals(Q, residuals=True)
    assert np.array_equal(res, (g.data[None] - f.geodetic_residuals(Q, residuals=False)) * g.odws[None])
    T, llks, o = prob.wavemaps[0].n_t, f.update_llks(Q), 0
    for d, n in enumerate(g.sizes):
        r = np.ascontiguousarray(res[:, o:o + n]).reshape(C, 1, n)
        hp = np.ascontiguousarray(Q[:, lay.offset(*g.hypers[d])]).reshape(C, 1)
        assert np.array_equal(ctx.wset_quad_batch(f._geo_wsets[d], r)[:, 0], llks[:, T + d]), d
        assert np.array_equal(ctx.mvn_chol_logp_batch(f._geo_wsets[d], r, hp)[:, 0], model["LL"][:, T + d]), d
        o += n


def test_d_laplacian_column_from_the_laplacian_entry(ctx, model):
    from beat_amd.models.problem import hyper_name_laplacian
    f, Q, prob = model["f"], model["Q"], model["prob"]
    lay, P = prob.layout, prob.npatches
    slips = np.stack([Q[:, lay.offset(v):lay.offset(v) + P] for v in prob.slip_varnames], axis=1)
    hp = np.ascontiguousarray(Q[:, lay.offset(hyper_name_laplacian)])
    col = prob.wavemaps[0].n_t + len(prob.geodetic.sizes)
    assert np.array_equal(ctx.laplacian_logp_batch(prob._lap, np.ascontiguousarray(slips), hp), model["LL"][:, col])
