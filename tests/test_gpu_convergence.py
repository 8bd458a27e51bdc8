"""GPU tests of the convergence summary (beat_amd/diagnostics.py, csrc/convergence.hip) against the numpy restatement
(tests/convergence_ref.py): the lagged products and the whole table bit for bit, the rank transform against scipy and
multi-precision values, and ``summary.txt`` of sampled stages."""
import os
from collections import OrderedDict

import numpy as np
import pytest

import convergence_ref as ref

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -53
KEYS = ("mean", "sd", "hdi_3%", "hdi_97%", "mcse_mean", "mcse_sd", "ess_bulk", "ess_tail", "r_hat", "ess_mean", "ess_sd")
EXACT = [0, 1, 2, 3, 6, 7, 8, 9, 10]      # device columns; 4 and 5 (the MCSE) are formed on the host by numpy


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _arr(table, keys=KEYS):
    return np.array([np.asarray(table[k].cpu().numpy() if hasattr(table[k], "cpu") else table[k]) for k in keys]).T


def _device_z(A):
    from beat_amd import diagnostics as d
    return d.rank_normalize(np.asarray(A, dtype=np.float64))


def _check(got, want, what):
    """device columns bit for bit (NaN = NaN); the host-formed MCSE within 4 units of 2^-53"""
    np.testing.assert_array_equal(got[:, EXACT], want[:, EXACT], err_msg=str(what))
    for c in (4, 5):
        g, w = got[:, c], want[:, c]
        assert np.array_equal(np.isnan(g), np.isnan(w)), (what, c)
        ok = ~np.isnan(w)
        assert np.all(np.abs(g[ok] - w[ok]) <= 4 * UNIT * np.abs(w[ok])), (what, c, g, w)


# ------------------------------------------------------------------------------------------------ autocov
ACOV_N = [2, 3, 63, 64, 65, ref.TILE - 1, ref.TILE, ref.TILE + 1, ref.CHUNK - 1, ref.CHUNK, ref.CHUNK + 1]


@pytest.mark.parametrize("n", ACOV_N)
def test_autocov_is_the_fixed_order_restatement(n):
    from beat_amd import diagnostics as d
    rng = np.random.default_rng(n)
    Y = ref.ar1(rng, 2, n, 0.6) * 3.0 + 1.5
    for lag0 in (0, 64, 65):
        for nlags in (1, 63, 64, 65, n):
            want = ref.acov_fixed(Y, lag0, nlags)
            got = d.autocov(Y, nlags, lag0)
            assert isinstance(got, np.ndarray) and np.array_equal(got, want), (n, lag0, nlags)
            if lag0 == 0 and nlags >= min(n, 3):
                fft = ref.acov_fft(Y)[:, :min(n, nlags)]
                assert np.abs(got[:, :fft.shape[1]] - fft).max() <= 1e-12 * fft[:, 0].max()
    got = d.autocov(_dev(Y), 65, 64)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), ref.acov_fixed(Y, 64, 65))
    one = d.autocov(Y[0], 5)
    assert one.shape == (5,) and np.array_equal(one, ref.acov_fixed(Y[:1], 0, 5)[0])


def test_autocov_rows_and_lag_ranges_split():
    from beat_amd import diagnostics as d
    rng = np.random.default_rng(11)
    for R, n in ((1, 65), (2, 700), (130, 65)):
        Y = ref.ar1(rng, R, n, 0.5)
        whole = d.autocov(Y, n)
        assert np.array_equal(whole, ref.acov_fixed(Y, 0, n))
        k = R // 2
        if k:
            assert np.array_equal(np.concatenate([d.autocov(Y[:k], n), d.autocov(Y[k:], n)]), whole)      # over rows
        parts = [d.autocov(Y, b - a, a) for a, b in ((0, 2), (2, 64), (64, 65), (65, n))]                  # over lag ranges
        assert np.array_equal(np.concatenate(parts, axis=1), whole)


def test_autocov_lag_ranges_of_a_large_batch():
    """4200 rows x 2 chunks x 8192 lags of chunk sums exceed the 256 MiB the launcher keeps: the lags go in ranges.  The
    rows of the large call are bitwise those of a small call (one range) and of the restatement"""
    import torch
    from beat_amd import diagnostics as d
    n = 2 * ref.CHUNK
    g = torch.Generator(device="cuda").manual_seed(5)
    Y = torch.randn((4200, n), dtype=torch.float64, device="cuda", generator=g)
    whole = d.autocov(Y, n)
    few = d.autocov(Y[[0, 1, 4199]].contiguous(), n)
    assert torch.equal(whole[[0, 1, 4199]], few)
    Yh = Y[[0, 4199]].cpu().numpy()
    for lag0 in (0, 3839, 3840, 8000):
        assert np.array_equal(few[[0, 2], lag0:lag0 + 70].cpu().numpy(), ref.acov_fixed(Yh, lag0, 70))


# ------------------------------------------------------------------------------------------------ rank normalisation
def _mp_ppf(p):
    import mpmath as mp
    mp.mp.dps = 50
    return [mp.sqrt(2) * mp.erfinv(2 * mp.mpf(float(q)) - 1) for q in p]


@pytest.mark.parametrize("S", [4, 5, 16385, 3 * 16384 + 1])
def test_rank_normalize_ranks_and_z(S):
    """ranks = scipy's rankdata; z within 16 x scipy's own distance from 50-digit values, at least 8 units of
    2^-53 max(1, |z|) (the rule of kde2d), on the 64 smallest, the 64 largest and 128 random ranks of every size"""
    import mpmath as mp
    from scipy import stats
    from beat_amd import diagnostics as d
    rng = np.random.default_rng(S)
    a = rng.standard_normal(S)
    z, r = d.rank_normalize(a, want_ranks=True)
    assert np.array_equal(r, stats.rankdata(a, "average"))
    rk = np.unique(np.concatenate([np.arange(1, min(S, 64) + 1), np.arange(max(1, S - 63), S + 1), rng.integers(1, S + 1, 128)]))
    p = (rk.astype(float) - 0.375) / (S + 0.25)
    zs, zm = stats.norm.ppf(p), _mp_ppf(p)
    pos = np.argsort(np.argsort(a))      # rank - 1 of every element (no ties here)
    where = dict((int(pos[i]) + 1, i) for i in range(S))
    for k, zsk, zmk in zip(rk, zs, zm):
        unit = UNIT * max(1.0, abs(float(zmk)))
        bound = max(16.0 * abs(float(mp.mpf(float(zsk)) - zmk)), 8.0 * unit)
        got = z[where[int(k)]]
        assert abs(float(mp.mpf(float(got)) - zmk)) <= bound, (S, k, got, float(zmk), bound / unit)
    zd = d.rank_normalize(_dev(a.reshape(1, -1)))
    assert zd.is_cuda and tuple(zd.shape) == (1, S) and np.array_equal(zd.cpu().numpy()[0], z)


def test_rank_normalize_ties():
    from scipy import stats
    from beat_amd import diagnostics as d
    rng = np.random.default_rng(3)
    S = 3 * 16384 + 1
    cases = [np.full(5, 2.5), np.full(16385, -1.0), np.round(rng.standard_normal(S), 1),
             np.where(rng.random(4097) < 0.5, 0.0, -0.0), np.array([0.0, -0.0, 1.0, -1.0, 0.0])]
    run = rng.standard_normal(S)
    run[16380:16390] = 0.25            # a run of ties across the edge of the first sort tile
    run[2 * 16384 - 1:2 * 16384 + 1] = 0.25
    cases.append(run)
    for a in cases:
        z, r = d.rank_normalize(a, want_ranks=True)
        want = stats.rankdata(a, "average")
        assert np.array_equal(r, want)
        assert np.array_equal(z[np.argsort(want, kind="stable")], np.sort(z))      # z is monotone in the rank
        for v in np.unique(a)[:3]:
            assert np.unique(z[a == v]).size == 1                                  # ties share their z
    assert d.rank_normalize(np.full(7, 2.5))[0] == 0.0
    with pytest.raises(ValueError, match="non-finite"):
        d.rank_normalize(np.array([1.0, np.nan, 2.0]))


# ------------------------------------------------------------------------------------------------ summary
@pytest.mark.parametrize("V", ref.GRID_V)
@pytest.mark.parametrize("D", ref.GRID_D)
@pytest.mark.parametrize("C", ref.GRID_C)
def test_summary_grid_is_the_restatement_on_the_device_z(C, D, V):
    from beat_amd import diagnostics as d
    X = ref.grid_input(C, D, V)
    t = d.summary(X)
    assert not t["flags"].any() and t["names"] == ["x%d" % i for i in range(V)]
    _check(_arr(t), ref.summary(X, z=_device_z), (C, D, V))


@pytest.mark.parametrize("D", [1, 3])
def test_fewer_than_four_draws_give_nan_diagnostics(D):
    from beat_amd import diagnostics as d
    X = ref.ar1(np.random.default_rng(D), 3, D, 0.0, 2)
    got, want = _arr(d.summary(X)), ref.summary(X)
    _check(got, want, D)
    assert np.all(np.isnan(got[:, 4:])) and not np.any(np.isnan(got[:, [0, 2, 3]]))


def test_constant_and_nan_columns():
    from beat_amd import diagnostics as d
    sp = ref.special_inputs()
    X = sp["constant"]
    t = _arr(d.summary(X))
    _check(t, ref.summary(X, z=_device_z), "constant")
    assert np.all(t[1, [6, 7, 9, 10]] == X.shape[0] * X.shape[1]) and np.isnan(t[1, 8]) and t[1, 1] == 0.0
    X = sp["nan"]
    tab = d.summary(X)
    assert tab["flags"].tolist() == [0, 0, 1] and np.all(np.isnan(_arr(tab)[2]))
    np.testing.assert_array_equal(_arr(tab)[:2], _arr(d.summary(X[:, :, :2])))      # the other columns keep their bits
    _check(_arr(tab), ref.summary(X, z=_device_z), "nan")


def test_slow_chains_take_several_rounds_and_no_schedule_changes_a_bit():
    from beat_amd import diagnostics as d
    X = ref.special_inputs()["ar99"]
    info = {}
    want = ref.summary(X, z=_device_z, info=info)
    assert info["max_t"] > 128
    base = d.summary(X)
    assert base["rounds"] >= 3                       # 64, 256 and 1024 lags
    _check(_arr(base), want, "ar99")
    for first in (2, 64, 256):
        t = d.summary(X, first_lags=first)
        np.testing.assert_array_equal(_arr(t), _arr(base), err_msg="first_lags %d" % first)
    assert d.summary(X, first_lags=2)["rounds"] > base["rounds"]
    X = np.concatenate([ref.grid_input(3, 129, 65)[:, :, :10], ref.ar1(np.random.default_rng(5), 3, 129, 0.95, 2)], axis=2)
    base = _arr(d.summary(X))
    for batch in (1, 7, X.shape[2]):
        for first in (2, 64, 256):
            np.testing.assert_array_equal(_arr(d.summary(X, var_batch=batch, first_lags=first)), base,
                                          err_msg="batch %d first %d" % (batch, first))
    cols = [11, 3, 3, 0]
    sub = d.summary(X, cols=cols, var_names=["v%d" % i for i in range(12)])
    assert sub["names"] == ["v11", "v3", "v3", "v0"]
    np.testing.assert_array_equal(_arr(sub), base[cols])


def test_device_trace_gives_tensors_and_single_variable_calls():
    import torch
    from beat_amd import diagnostics as d
    X = ref.grid_input(3, 129, 3)
    host = d.summary(X)
    dev = d.summary(_dev(X))
    for k in KEYS + ("flags",):
        assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda and isinstance(host[k], np.ndarray)
    np.testing.assert_array_equal(_arr(dev), _arr(host))
    np.testing.assert_array_equal(_arr(d.summary(X[0])), _arr(d.summary(X[:1])))       # (D, V) is one chain
    x, row = X[:, :, 1], _arr(host)[1]
    assert [d.ess(x, "bulk"), d.ess(x, "tail"), d.ess(x, "mean"), d.ess(x, "sd"), d.rhat(x)] == [row[6], row[7], row[9],
                                                                                                 row[10], row[8]]
    assert d.mcse(x, "mean") == row[4] and d.mcse(x, "sd") == row[5] and d.hdi(x).tolist() == [row[2], row[3]]
    lo, hi = d.hdi(x, 0.5)
    assert (lo, hi) == ref.hdi(x, 0.5)
    assert float(d.ess(_dev(x), "bulk")) == row[6] and d.hdi(_dev(x)).is_cuda


E2E_TOL_ESS, E2E_TOL_RHAT = 16 * 3.1e-15, 16 * 6.8e-16


@pytest.mark.parametrize("case", [(1, 37), (3, 129), (8, 130), "ar99"])
def test_end_to_end_against_the_all_host_restatement(case):
    """scipy's z in the restatement: mean, sd, the interval, ess_tail, ess_mean, ess_sd and the MCSE do not see z and are
    equal.  ess_bulk and r_hat: scipy's z was perturbed on the CPU by +- its admitted bound (64 units of 2^-53 max(1, |z|) =
    16 x scipy's measured distance of 4 units from 50-digit values) 100 times for the inputs (1, 37), (3, 129), (8, 130)
    and ar99; the largest relative change was 3.1e-15 (ess_bulk) and 6.8e-16 (r_hat); the tolerances are 16 x those."""
    from beat_amd import diagnostics as d
    X = ref.special_inputs()["ar99"] if case == "ar99" else ref.grid_input(case[0], case[1], 3)
    got, want = _arr(d.summary(X)), ref.summary(X)
    np.testing.assert_array_equal(got[:, [0, 1, 2, 3, 7, 9, 10]], want[:, [0, 1, 2, 3, 7, 9, 10]])
    for c in (4, 5):
        assert np.all(np.abs(got[:, c] - want[:, c]) <= 4 * UNIT * np.abs(want[:, c]))
    print(case, np.abs(got[:, 6] / want[:, 6] - 1).max(), np.abs(got[:, 8] / want[:, 8] - 1).max())
    assert np.all(np.abs(got[:, 6] - want[:, 6]) <= E2E_TOL_ESS * want[:, 6])
    assert np.all(np.abs(got[:, 8] - want[:, 8]) <= E2E_TOL_RHAT * want[:, 8])


# ------------------------------------------------------------------------------------------------ stages
def test_summarize_stage_of_smc_and_pt_toys(tmp_path):
    from test_samplers_cpu import _two_gaussians
    from beat_amd import diagnostics as d
    from beat_amd.backend import stage_path, write_population
    from beat_amd.models import ParameterLayout
    from beat_amd.sampler import SMC, smc_sample
    from beat_amd.sampler.hosttarget import HostTarget
    from beat_amd.sampler.pt import pt_sample
    f, n = _two_gaussians()
    lay = ParameterLayout(OrderedDict([("x", n)]))
    step = SMC(HostTarget(f, n), -2 * np.ones(n), 2 * np.ones(n), n_chains=64, tune_interval=10, random_seed=3)
    home = str(tmp_path / "smc")
    smc_sample(20, step, homepath=home, layout=lay, out_names=["like"], buffer_thinning=2, max_stages=3)
    final = stage_path(home, -1)
    table, text = d.summarize_stage(final, lay, ["like"], "SMC")
    names = ["x[%d]" % i for i in range(n)] + ["like"] if n > 1 else ["x", "like"]
    lines = open(os.path.join(home, "summary.txt")).read().splitlines()
    assert table["names"] == names and [ln.split()[0] for ln in lines[1:]] == names
    assert lines[0].split() == list(KEYS[:9]) and "\n".join(lines) == text
    vals, rows = d.read_stage(final, lay, ["like"])
    from beat_amd.backend import thinned_draws
    assert rows == names and vals.shape == (64, len(thinned_draws(20, 2)), n + 1)      # draws 0, 2, ..., 18 and the last
    one = d.summary(vals.reshape(1, -1, n + 1))                      # chain after chain as ONE chain (backend.py:1401-1415)
    np.testing.assert_array_equal(_arr(table), _arr(one))
    for ln, row in zip(lines[1:], _arr(one)):
        np.testing.assert_array_equal([float(v) for v in ln.split()[1:]], [float("%.4f" % v) for v in row[:9]])
    # an intermediate stage contributes the last draw of every chain
    mid, _ = d.summarize_stage(stage_path(home, 1), lay, ["like"], "SMC", final=False, summary_file=False)
    v1, _ = d.read_stage(stage_path(home, 1), lay, ["like"])
    np.testing.assert_array_equal(_arr(mid), _arr(d.summary(v1[:, -1:].reshape(1, -1, n + 1))))
    # PT: the kept draws of chain 0, the chains kept apart
    s, ls, _ = pt_sample(HostTarget(f, n), -2 * np.ones(n), 2 * np.ones(n), n_chains_posterior=2, n_chains_tempered=6,
                         n_replicas=8, n_samples=400, swap_interval=(20, 40), beta_tune_interval=5,
                         proposal_cov=np.eye(n) * 0.02, random_seed=5)
    homept = str(tmp_path / "pt")
    write_population(homept, -1, lay, ["like"], s[:, None, :], np.asarray(ls).reshape(s.shape[0], 1, -1)[:, :, :1])
    tpt, _ = d.summarize_stage(stage_path(homept, -1), lay, ["like"], "PT", burn=0.25, thin=2, per_chain=True)
    vpt, _ = d.read_stage(stage_path(homept, -1), lay, ["like"])
    np.testing.assert_array_equal(_arr(tpt), _arr(d.summary(vpt[:1, 100::2])))
    assert os.path.exists(os.path.join(homept, "summary.txt"))
