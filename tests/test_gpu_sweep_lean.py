"""The lean diagonal loop of the rupture-time sweep (sweep.hip sweep_diag64: slowness terms once per grid, one clamped cell
index per lane, v_min_f64 minima, three diagonals per trip, the unscaled sqrt where SWEEP_PLAIN holds) against the first
version (BEATAMD_SWEEP_V1=1, sweep_wave's LDS loop) in one process.  Same operands, operations and order per cell, so
every comparison is np.array_equal on the float64 times: no tolerance.

The model path (mode 1 of the kernel: slowness = 1 / velocities, hypocentre index from the nucleation position, + time)
is read through CompiledModel.start_times."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sweep_ref import host_sweep  # noqa: E402  (the numpy restatement of the reference's loops: counts iterations here)

pytestmark = pytest.mark.gpu

# no interior (every neighbour clamps); rows and columns swapped; the bench grid; 64 rows (the limit, all lanes live);
# diagonal counts ni + nj - 1 of every residue of the three-diagonal trip, odd and even; 65 rows: the first version
GRIDS = [(1, 1), (1, 2), (2, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (20, 20), (64, 2), (64, 64), (63, 33), (63, 34),
         (65, 3)]
H = 1.3


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


def _hypocentres(ni, nj):
    """the four corners, an edge midpoint and the centre"""
    return [(0, 0), (0, nj - 1), (ni - 1, 0), (ni - 1, nj - 1), (0, nj // 2), (ni // 2, nj // 2)]


def _fields(ni, nj, rng):
    n = ni * nj
    uniform = np.full(n, 1.0 / 3.0)
    random = rng.uniform(1.0 / 4.0, 1.0 / 2.5, n)
    holes = random.copy().reshape(ni, nj)
    if n > 4:
        holes.ravel()[rng.choice(n, 3, replace=False)] = np.inf       # isolated infinitely slow patches
    if ni >= 3:
        holes[ni // 2, :] = np.inf                                    # a row that cuts the grid
    elif nj >= 3:
        holes[:, nj // 2] = np.inf
    ii, jj = np.meshgrid(np.arange(ni), np.arange(nj), indexing="ij")
    checker = np.where((ii + jj) % 2 == 0, 0.25, 1e3).ravel()
    # (1e-200: 2*f*f*h*h underflows to 0, the sqrt argument is -(a-b)^2 or 0; 1e+150: arguments near 1e299)
    return [("uniform", uniform), ("random", random), ("inf", holes.ravel()), ("tiny", random * 1e-200),
            ("huge", random * 1e150), ("checker", checker)]


@functools.lru_cache(maxsize=None)
def _case(ni, nj):
    """every field x every hypocentre of one grid as one batch"""
    rng = np.random.default_rng(100 * ni + nj)
    slow, hi, hj, names = [], [], [], []
    for fname, f in _fields(ni, nj, rng):
        for (a, b) in _hypocentres(ni, nj):
            slow.append(f)
            hi.append(a)
            hj.append(b)
            names.append("%s@%d,%d" % (fname, a, b))
    return np.array(slow), np.array(hi, dtype=np.int32), np.array(hj, dtype=np.int32), names


def _both(ctx, monkeypatch, call):
    monkeypatch.delenv("BEATAMD_SWEEP_V1", raising=False)
    new = call()
    monkeypatch.setenv("BEATAMD_SWEEP_V1", "1")
    old = call()
    monkeypatch.delenv("BEATAMD_SWEEP_V1", raising=False)
    return new, old


@pytest.mark.parametrize("ni,nj", GRIDS)
def test_lean_sweep_is_bitwise_the_first_version(ctx, monkeypatch, ni, nj):
    slow, hi, hj, names = _case(ni, nj)
    new, old = _both(ctx, monkeypatch, lambda: ctx.fast_sweep_batch(slow, H, hi, hj, ni, nj))
    for c, name in enumerate(names):
        assert np.array_equal(new[c], old[c], equal_nan=True), (ni, nj, name)
    # the fields are what they are meant to be: reached cells finite, the hypocentre at 0
    assert np.all(new[np.arange(len(hi)), hi * nj + hj] == 0.0)
    assert not np.isnan(new).any()


# ---------------------------------------------------------------------------------------------- the bench population
def _spec():
    from beat_amd.synthetic import SyntheticSpec
    # the bench fault (one 20 x 20 subfault of 1 km patches; velocities U(2.5, 4)) and a second, oblong subfault with
    # another patch size; a small library: only the rupture times are computed.  time > 0: the + time store.
    return SyntheticSpec((20, 3), (20, 5), (1.0, 0.7), T=1, N=32, D=1, S=2, st_dt=13.0, time_bounds=(0.25, 1.0))


@functools.lru_cache(maxsize=None)
def _population():
    """chains 1000 + c, c < 513, of the bench's draw; subfault 0 as explicit sweep inputs; its outer iterations"""
    from beat_amd.synthetic import _layout_and_bounds, draw_population
    spec = _spec()
    layout, lower, upper = _layout_and_bounds(spec)
    Q = draw_population(spec, layout, lower, upper, 513)
    v0 = layout.offset("velocities")
    slow = 1.0 / Q[:, v0:v0 + 400]
    h = 1.0
    hi = np.rint((Q[:, layout.offset("nucleation_dip")] - h / 2.0) / h).astype(np.int32)
    hj = np.rint((Q[:, layout.offset("nucleation_strike")] - h / 2.0) / h).astype(np.int32)
    _, iters = host_sweep(slow, h, hi, hj, 20, 20)
    return spec, layout, Q, slow, hi, hj, iters


def test_population_holds_two_and_three_iteration_grids():
    iters = _population()[-1]
    assert (iters == 2).any() and (iters >= 3).any(), np.bincount(iters)


@pytest.mark.parametrize("C", [1, 4, 5, 513])
def test_lean_sweep_chain_counts_explicit(ctx, monkeypatch, C):
    """the edges of the four-wave workgroup; the first chains of the population and, so that every count sweeps grids
    of two and of three outer iterations, one of each in front"""
    _, _, _, slow, hi, hj, iters = _population()
    first = [int(np.flatnonzero(iters >= 3)[0]), int(np.flatnonzero(iters == 2)[0])]
    sel = (first + [c for c in range(513) if c not in first])[:C] if C >= 4 else first[:C]
    new, old = _both(ctx, monkeypatch, lambda: ctx.fast_sweep_batch(slow[sel], 1.0, hi[sel], hj[sel], 20, 20))
    assert np.array_equal(new, old)
    assert np.isfinite(new).all()


@pytest.fixture(scope="module")
def model(ctx):
    from beat_amd.synthetic import build_problem
    prob, host = build_problem(_spec())
    f = prob.compile(ctx)
    yield f
    f.release()


@pytest.mark.parametrize("C", [1, 4, 5, 513])
def test_lean_sweep_chain_counts_model_path(ctx, monkeypatch, model, C):
    spec, layout, Q, slow, hi, hj, _ = _population()
    new, old = _both(ctx, monkeypatch, lambda: model.start_times(Q[:C]))
    assert new.shape == (C, spec.P)
    assert np.array_equal(new, old)
    # subfault 0 of the model path is the explicit sweep of the same slowness and hypocentre, plus the nucleation time
    explicit = ctx.fast_sweep_batch(slow[:C], 1.0, hi[:C], hj[:C], 20, 20)
    tadd = Q[:C, layout.offset("time")]
    assert tadd.min() > 0.0
    assert np.array_equal(new[:, :400], explicit + tadd[:, None])
    assert np.isfinite(new).all()


def test_hypocentre_outside_the_grid_raises_and_flags_the_chain(ctx, model):
    _, layout, Q, *_ = _population()
    q = Q[:6].copy()
    q[2, layout.offset("nucleation_dip")] = 20.7          # index 20 of a 20-row subfault
    q[4, layout.offset("nucleation_strike", 1)] = -0.9    # index -2 of the second subfault
    bad = np.full(6, -1, dtype=np.int32)
    with pytest.raises(ValueError, match="nucleation index outside the patch grid"):
        model.start_times(q, chain_bad=bad)
    assert bad.tolist() == [0, 0, 1, 0, 1, 0]
    # the status word was cleared by the raise: the next call is clean
    assert np.isfinite(model.start_times(Q[:6])).all()
