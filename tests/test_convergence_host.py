"""CPU tests of the convergence summary (beat_amd/diagnostics.py, csrc/convergence.hip): the numpy restatement of the kernels
(tests/convergence_ref.py) is pinned to numpy / scipy primitives and to AR(1) processes whose autocorrelation time is known
in closed form; the inputs of the GPU tests are checked for stopping lags that no rounding can move; the prototypes, the
argument rules and the kernels' resources."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import convergence_ref as ref
import marginals_ref
from conftest import ROOT


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


# ------------------------------------------------------------------------------------------------ restatement vs libraries
ROUTE_CASES = [(1, 4, 0.0), (1, 5, 0.0), (2, 37, 0.5), (3, 129, 0.3), (2, 20001, 0.5), (4, 4000, 0.9), (8, 130, 0.0),
               (2, 2400, 0.99)]
ROUTE_TOL = 16 * 3.6e-15


def test_autocovariance_routes_agree():
    """ess from the FFT autocovariance (arviz's route) and from the kernel's fixed-order sums differ by rounding only.
    Measured on these cases (raw and rank-normalised split chains, seed 0): at most 3.6e-15 relative, at (2, 20001, 0.5);
    the tolerance is 16 x that, 5.8e-14."""
    rng = np.random.default_rng(0)
    for C, D, phi in ROUTE_CASES:
        x = ref.ar1(rng, C, D, phi)
        for A in (ref.split(x), ref.z_scipy(ref.split(x))):
            a, b = ref.ess(A, "fixed"), ref.ess(A, "fft")
            print(C, D, phi, a, b, abs(a - b) / abs(b))
            assert abs(a - b) <= ROUTE_TOL * abs(b), (C, D, phi, a, b)
        k = min(D // 2, 70)
        fixed, fft = ref.acov_fixed(ref.split(x), 0, k), ref.acov_fft(ref.split(x))[:, :k]
        assert np.abs(fixed - fft).max() <= 1e-13 * np.abs(fft[:, 0]).max()


def test_ranks_are_rankdata_and_z_is_norm_ppf():
    from scipy import stats
    rng = np.random.default_rng(1)
    for n in (1, 2, 5, 64, 1000):
        for a in (rng.standard_normal(n), np.round(rng.standard_normal(n), 1), np.full(n, 3.0),
                  np.where(rng.random(n) < 0.5, 0.0, -0.0)):
            r = stats.rankdata(a, "average")
            assert np.array_equal(ref.ranks(a), r)
            assert np.array_equal(ref.z_scipy(a.reshape(1, -1))[0], stats.norm.ppf((r - 0.375) / (n + 0.25)))


def test_hdi_scan_is_the_narrowest_interval():
    rng = np.random.default_rng(2)
    for n in (1, 2, 5, 50, 301):
        for x in (rng.standard_normal(n), np.round(rng.gamma(2.0, 1.0, n), 1)):
            for p in (0.5, 0.94):
                s = np.sort(x)
                inc = min(int(np.floor(p * n)), n - 1)
                best = min(range(n - inc), key=lambda j: (s[j + inc] - s[j], j))       # brute force, first minimum
                assert ref.hdi(x, p) == (s[best], s[best + inc])


def test_quantiles_are_numpys():
    rng = np.random.default_rng(3)
    for n in (4, 5, 37, 1000, 1001):
        x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)
        got = marginals_ref.percentiles(np.sort(x)[None], [5.0, 50.0, 95.0])[0]
        assert np.array_equal(got, np.quantile(x, [0.05, 0.5, 0.95]))
        assert np.array_equal(got, np.percentile(x, [5, 50, 95]))


def test_rhat_is_the_textbook_form():
    rng = np.random.default_rng(4)
    for M, n in ((2, 2), (2, 18), (6, 64), (16, 65), (4, 1000)):
        A = rng.standard_normal((M, n)) + rng.normal(0.0, 0.3, (M, 1))
        a, b = ref.rhat(A), ref.rhat_textbook(A)
        assert abs(a - b) <= 64 * 2.0 ** -53 * b, (M, n, a, b)       # both sums of n terms: rounding only
    assert np.isnan(ref.rhat(np.full((4, 10), 1.5)))


def test_moments_order_is_a_sum():
    rng = np.random.default_rng(5)
    for n in (1, 255, 256, 257, 5000):
        Y = rng.standard_normal((3, n))
        mean, css, lo, hi = ref.moments(Y)
        np.testing.assert_allclose(mean, Y.mean(axis=1), rtol=0, atol=1e-15 * np.sqrt(n))
        np.testing.assert_allclose(css, ((Y - Y.mean(axis=1, keepdims=True)) ** 2).sum(axis=1), rtol=1e-13)
        assert np.array_equal(lo, Y.min(axis=1)) and np.array_equal(hi, Y.max(axis=1))


LAW_SEEDS = 40
LAW_SPREAD = {0.0: 0.044, 0.5: 0.023, 0.9: 0.0098}


def test_ar1_law_of_the_autocorrelation_time():
    """AR(1) chains have tau = (1 + phi) / (1 - phi), so ess_mean / S estimates (1 - phi) / (1 + phi).  Measured first, at
    4 x 1000 draws over the 40 seeds 1000 .. 1039 (FFT route): phi 0: mean 0.9781, standard deviation over the seeds 0.0436,
    range 0.838 .. 1.057 (law 1); phi 0.5: 0.33333, 0.0227, 0.272 .. 0.381 (law 0.33333); phi 0.9: 0.05358, 0.0098,
    0.018 .. 0.075 (law 0.05263).  The band: the seeds must bracket the law, and their mean must lie within ONE measured
    standard deviation of it (LAW_SPREAD; Geyer's truncation biases the estimate at phi = 0 by half of that)."""
    for phi, spread in LAW_SPREAD.items():
        law = (1.0 - phi) / (1.0 + phi)
        r = np.array([ref.ess(ref.split(ref.ar1(np.random.default_rng(1000 + seed), 4, 1000, phi)), "fft") / 4000.0
                      for seed in range(LAW_SEEDS)])
        print(phi, law, r.mean(), r.std(), r.min(), r.max())
        assert r.min() < law < r.max(), (phi, r.min(), r.max())
        assert abs(r.mean() - law) <= spread, (phi, r.mean(), law)


def test_gpu_fixtures_have_no_stopping_lag_on_an_edge():
    """for every input of the GPU tests the smallest |even + odd| over the pairs Geyer's scan evaluates is at least 1e-9: no
    rounding can move a stopping lag (measured: the smallest is printed)"""
    worst = np.inf
    inputs = [ref.grid_input(C, D, V) for C in ref.GRID_C for D in ref.GRID_D for V in ref.GRID_V]
    sp = ref.special_inputs()
    inputs += [sp["constant"], sp["nan"][:, :, :2], sp["ar99"]]
    for X in inputs:
        info = {}
        ref.summary(X, info=info)
        if "gap" in info:
            worst = min(worst, info["gap"])
            assert info["gap"] >= 1e-9, (X.shape, info)
    print("smallest |even + odd|:", worst)
    info = {}
    ref.summary(sp["ar99"], info=info)
    assert info["max_t"] > 128      # the on-demand rounds of this input run more than once, past 64 and past 128 lags


# ------------------------------------------------------------------------------------------------ host functions
def test_names_text_and_mcse():
    from beat_amd import diagnostics as d
    assert d.hdi_names(0.94) == ("hdi_3%", "hdi_97%") and d.hdi_names(0.5) == ("hdi_25%", "hdi_75%")
    assert d.row_names(["uparr", "time", "like"], [3, 1, 1]) == ["uparr[0]", "uparr[1]", "uparr[2]", "time", "like"]
    sd, em, es = np.array([1.5, 2.0]), np.array([400.0, 50.5]), np.array([333.0, 20.25])
    a, b = d.mcse_columns(sd, em, es)
    ra, rb = ref.mcse_columns(sd, em, es)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)
    keys = ("mean", "sd", "hdi_3%", "hdi_97%", "mcse_mean", "mcse_sd", "ess_bulk", "ess_tail", "r_hat", "ess_mean", "ess_sd")
    table = dict((k, np.array([1.234567, -20.5])) for k in keys)
    table.update(names=["uparr[0]", "time"], flags=np.zeros(2, np.int32), rounds=1)
    text = d.summary_to_string(table).splitlines()
    assert len(text) == 3 and text[0].split() == list(keys[:9])
    assert text[1].split() == ["uparr[0]"] + ["1.2346"] * 9 and text[2].split() == ["time"] + ["-20.5000"] * 9
    assert len(set(len(t) for t in text)) == 1


# ------------------------------------------------------------------------------------------------ ABI, argument rules
NEW_ENTRIES = {"beatamd_autocov_lags_batch": 7, "beatamd_rank_normalize": 5, "beatamd_convergence_summary": 14}


def test_convergence_entries_are_declared_and_bound():
    from beat_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "beat_amd.h")).read()
    lib = _lib.load()
    for name, arity in NEW_ENTRIES.items():
        m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr)
        assert m, "%s is not declared" % name
        assert len(m.group(1).split(",")) == arity == len(_lib._PROTOS[name]), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    doc = hdr[hdr.index("convergence summary of a trace"):]
    for name in ("autocov_lags_batch", "rank_normalize", "convergence_summary"):
        assert re.search(r"%s \(apps/beat.py:1338-1363, backend.py:1401-1415" % name, doc), name
    assert "restated from memory" in doc and "unverified against an installed arviz" in doc


def test_argument_rules_need_no_device():
    from beat_amd import diagnostics as d, diagnostics_binding as db
    with pytest.raises(ValueError):
        d.summary(np.zeros(5))                              # not (C, D, V) or (D, V)
    with pytest.raises(ValueError):
        d.summary(np.zeros((2, 0, 3)))
    with pytest.raises(ValueError):
        d.summary(np.zeros((2, 8, 3)), hdi_prob=1.0)
    with pytest.raises(ValueError):
        d.summary(np.zeros((2, 8, 3)), first_lags=1)
    with pytest.raises(ValueError):
        d.summary(np.zeros((2, 8, 3)), var_batch=-1)
    with pytest.raises(ValueError):
        d.ess(np.zeros((2, 8)), method="median")
    with pytest.raises(ValueError):
        d.mcse(np.zeros((2, 8)), method="bulk")
    with pytest.raises(ValueError):
        d.ess(np.zeros((2, 8, 3)))                          # one variable only
    with pytest.raises(ValueError):
        d.autocov(np.zeros((2, 8)), -1)
    with pytest.raises(ValueError):
        d.rank_normalize(np.zeros(0))
    with pytest.raises(IndexError):
        db.check_columns([3], 3)
    assert db.tau_floor(2, 3) == 0.0 and db.tau_floor(2, 37) == 1.0 / np.log10(np.float64(72))
    assert db.COLUMNS == ref.COLUMNS and db.NCOL == 11
    with pytest.raises(NotImplementedError):
        d.summarize_stage("nowhere", None, [], sampler="NUTS")


@pytest.mark.skipif(_gpu_present(), reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    from beat_amd import BeatAmdError, diagnostics as d
    rng = np.random.default_rng(7)
    X = rng.standard_normal((2, 50, 3))
    calls = [lambda: d.summary(X), lambda: d.summary(X[0]), lambda: d.ess(X[:, :, 0]), lambda: d.ess(X[0, :, 0], "tail"),
             lambda: d.rhat(X[:, :, 0]), lambda: d.mcse(X[:, :, 0], "sd"), lambda: d.hdi(X[:, :, 0]),
             lambda: d.autocov(X[:, :, 0], 5), lambda: d.rank_normalize(X[:, :, 0])]
    for call in calls:
        with pytest.raises(BeatAmdError):
            call()


KERNELS = ("k_conv_iota", "k_conv_moments", "k_conv_hdi", "k_conv_write_raw", "k_conv_write_derived", "k_conv_rank_z",
           "k_acov_lags", "k_acov_combine", "k_conv_lagmean", "k_conv_regroup", "k_conv_geyer", "k_conv_rhat", "k_conv_finish")


def test_convergence_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "beat_amd", "csrc", "convergence.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "convergence.o")],
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
    assert len(seen) == len(KERNELS) + 1, sorted(seen)      # every kernel of the file is listed above; k_acov_lags has two shapes
    for kern in KERNELS:
        hits = [v for k, v in seen.items() if kern in k]
        assert hits, "no resource report for %s:\n%s" % (kern, r.stdout[-2000:])
        assert hits == [0] * len(hits), "%s uses scratch: %s" % (kern, hits)
    # the tile and the chunk of the lag kernel are stated once; the binding and the restatement repeat them
    from beat_amd import diagnostics_binding as db
    hpp = open(os.path.join(ROOT, "beat_amd", "csrc", "kernels.hpp")).read()
    assert "CV_ACOV_TILE = 512" in hpp and "CV_ACOV_CHUNK = 4096" in hpp
    assert (db.ACOV_TILE, db.ACOV_CHUNK) == (512, 4096) == (ref.TILE, ref.CHUNK)
    mk = open(os.path.join(ROOT, "beat_amd", "csrc", "Makefile")).read()
    assert "convergence.hip" in mk and "-ffp-contract=off" in mk
    txt = open(src).read()
    assert "atomicAdd" not in txt
