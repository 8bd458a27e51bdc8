"""CPU tests of the hyper-parameter estimation: the numpy restatement (tests/hyper_ref.py) against numbers of the
reference's own hyper_normal / _eval_prior / thin_buffer (tests/golden/hypers.npz, tools/gen_golden_hypers.py), the
hyper table of a mixed problem, the thinning rule and bounds arithmetic, no CPU fallback, and the compiler's resource
report of the two kernels."""
import os
import re
import shutil
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hyper_ref as href  # noqa: E402


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.parametrize("tag", ["shared", "specific"])
def test_h1_terms_vs_reference_hyper_normal(golden, tag):
    g = golden("hypers")
    typs, names, H, hp_index = href.fixture_tables(g, tag)
    n = len(typs)
    got = href.terms(g["hn_samples"], g["hn_slog"], np.zeros(n, dtype=int), hp_index, H, g["hn_llks"])
    exp = g["hn_%s_logpts" % tag]
    dev = np.max(np.abs(got - exp) / np.abs(exp))
    print("hyper_normal (%s): largest relative deviation %.3g" % (tag, dev))
    np.testing.assert_allclose(got, exp, rtol=1e-14)


def test_h1_laplacian_term_vs_reference_eval_prior(golden):
    g = golden("hypers")
    n = g["lap_h"].size
    got = href.terms(g["lap_P"], g["lap_logdet"], np.ones(n, dtype=int), np.zeros(n, dtype=int), g["lap_h"][None, :].T,
                     np.broadcast_to(g["lap_exponent"], (n, n)))
    got = np.diagonal(got)
    dev = np.max(np.abs(got - g["lap_logpt"]) / np.abs(g["lap_logpt"]))
    print("_eval_prior: largest relative deviation %.3g" % dev)
    np.testing.assert_allclose(got, g["lap_logpt"], rtol=1e-14)


def test_h1_like_order_is_a_sum():
    """the device's fixed order is a reordering of the plain sum: equal to it within the rounding of nterm additions"""
    rng = np.random.default_rng(3)
    for nterm, ends in ((1, [1]), (5, [2, 5]), (64, [64]), (200, [130, 131, 200]), (1024, [1000, 1024])):
        T = rng.normal(0, 1e3, (7, nterm))
        got = href.like(T, ends)
        np.testing.assert_allclose(got, T.sum(1), rtol=0, atol=nterm * 2.0 ** -52 * np.abs(T).sum(1).max())
    assert np.isnan(href.like(np.array([[1.0, np.nan, 2.0]]), [1, 3]))[0]


class _DS(object):
    def __init__(self, typ):
        self.typ = typ


def _mixed_problem(g):
    """two wavemaps with hp_specific, two geodetic types, a Laplacian with two slip variables; host description only"""
    from beat_amd.models import FFIProblem, GeodeticData, ParameterLayout, SeismicWavemap, dataset_hypers
    typs = [str(t) for t in g["hn_typs"]]
    idx = {t: [k for k, x in enumerate(typs) if x == t] for t in set(typs)}
    P, N = 6, 16
    wms = []
    for name, typ in (("any_P_0", "any_P_0_Z"), ("any_S_1", "any_S_1_T")):
        ks = idx[typ]
        wms.append(SeismicWavemap({}, np.zeros((len(ks), N)), np.ones(len(ks)), g["hn_slog"][ks],
                                  dataset_hypers([_DS(typ)] * len(ks), hp_specific=True), name=name))
    gk = sorted(idx["SAR"] + idx["GNSS"])
    sizes = [int(g["hn_samples"][k]) for k in gk]
    geo = GeodeticData({}, np.zeros(sum(sizes)), np.ones(sum(sizes)), sizes, [1.0] * len(gk), g["hn_slog"][gk],
                       dataset_hypers([_DS(typs[k]) for k in gk], hp_specific=True))
    sz = OrderedDict([("uparr", P), ("uperp", P), ("h_any_P_0_Z", len(idx["any_P_0_Z"])), ("h_any_S_1_T", len(idx["any_S_1_T"])),
                      ("h_GNSS", len(idx["GNSS"])), ("h_SAR", len(idx["SAR"])), ("h_laplacian", 1)])
    lay = ParameterLayout(sz)
    lower = {k: -2.0 for k in sz}
    upper = {k: 3.0 for k in sz}
    prob = FFIProblem(lay, [2], [3], [1.0], ["uparr", "uperp"], wms, geo, (np.eye(P), 1.25), lower, upper)
    order = idx["any_P_0_Z"] + idx["any_S_1_T"] + gk
    return prob, order, typs


def test_h2_hyper_table_of_a_mixed_problem(golden):
    from beat_amd.models import HyperModel, dataset_hypers
    g = golden("hypers")
    typs = [str(t) for t in g["hn_typs"]]
    # the Counter order of the reference, on the fixture's mixed list
    assert [i for _, i in dataset_hypers([_DS(t) for t in typs], hp_specific=True)] == list(g["hn_specific_index"])
    assert [i for _, i in dataset_hypers([_DS(t) for t in typs], hp_specific=False)] == list(g["hn_shared_index"])
    assert [n for n, _ in dataset_hypers([_DS(t) for t in typs])] == ["h_" + t for t in typs]
    prob, order, typs = _mixed_problem(g)
    hm = HyperModel(prob)
    assert hm.names == ["h_any_P_0_Z", "h_any_S_1_T", "h_GNSS", "h_SAR", "h_laplacian"]
    assert hm.nh == hm.nparams == len(typs) + 1
    assert hm.nterm == len(typs) + 2 and hm.nllk == hm.nterm + 1
    nP, nS = typs.count("any_P_0_Z"), typs.count("any_S_1_T")
    assert list(hm.group_end) == [nP + nS, len(typs), len(typs) + 2]
    assert hm.out_names == (["seis_like_any_P_0_%d" % i for i in range(nP)] + ["seis_like_any_S_1_%d" % i for i in range(nS)]
                            + ["geo_like_%d" % i for i in range(len(typs) - nP - nS)]
                            + ["laplacian_like_uparr", "laplacian_like_uperp", "like"])
    # every dataset term reads the entry of its name that the reference read for that dataset
    for k, ds in enumerate(order):
        name = "h_" + typs[ds]
        assert hm.hp_index[k] == hm.layout.offset(name, int(g["hn_specific_index"][ds])), (k, ds)
        assert hm.kind[k] == 0
    assert list(hm.kind[-2:]) == [1, 1] and list(hm.hp_index[-2:]) == [hm.layout.offset("h_laplacian")] * 2
    assert list(hm.M[-2:]) == [6, 6] and list(hm.slog[-2:]) == [1.25, 1.25]
    assert list(hm.M[nP + nS:len(typs)]) == [int(g["hn_samples"][k]) for k in order[nP + nS:]]
    np.testing.assert_array_equal(hm.lower, -2.0 * np.ones(hm.nh))
    assert list(hm.full_index) == list(range(12, 12 + hm.nh))
    # the files of a hyper trace: the Laplacian's terms form one vector variable
    from beat_amd.backend import population_shapes
    shapes, _ = population_shapes(hm.layout, hm.out_names)
    assert shapes["laplacian_like"] == (2,) and shapes["like"] == () and shapes["seis_like"] == (nP + nS,)


def test_h3_thinning_rule_and_bounds(golden):
    from beat_amd.models.hypers import bounds_of_extrema, hyper_bounds, kept_draws, thinned_length
    g = golden("hypers")
    for n, t in g["thin_cases"]:
        exp = list(g["thin_%d_%d" % (n, t)])
        assert exp == href.recorded_steps(int(n), int(t))
        assert thinned_length(n, t) == len(exp) == -(-int(n) // int(t))
        # the kernel's rule: step s is kept iff (n - 1 - s) % t == 0, in row (s - (n - 1) % t) / t
        kept = [s for s in range(n) if (n - 1 - s) % t == 0]
        assert kept == exp and [(s - (n - 1) % t) // t for s in kept] == list(range(len(exp)))
    n_steps, bt = int(g["bounds_n_steps"]), int(g["bounds_buffer_thinning"])
    for i in range(int(g["bounds_n"])):
        draws = g["bounds_draws_%d" % i]
        assert draws.shape[0] == thinned_length(n_steps, bt)       # burn is taken on the thinned length
        got = hyper_bounds(draws, burn=float(g["bounds_burn"]), thin=int(g["bounds_thin"]))
        assert got == tuple(g["bounds_expected"][i])
        # the two pieces estimate_hypers runs, with the extrema of the kept draws taken chain block by chain block
        kept = kept_draws(draws, float(g["bounds_burn"]), int(g["bounds_thin"]))
        assert kept.shape[0] == len(range(int(draws.shape[0] * float(g["bounds_burn"])), draws.shape[0], int(g["bounds_thin"])))
        blocks = [kept[:, :2], kept[:, 2:]]
        assert bounds_of_extrema(min(b.min() for b in blocks), max(b.max() for b in blocks)) == got
        assert got[0] == int(got[0]) and got[1] == int(got[1]) and got[2] == (got[0] + got[1]) / 2


def test_h3_host_counters_advance_like_single_steps():
    """BatchedMetropolis._advance_counters == n times the bookkeeping of step()"""
    import torch

    from beat_amd.sampler.hosttarget import HostTarget
    from beat_amd.sampler.metropolis import BatchedMetropolis
    for tune in (True, False):
        for interval in (1, 7, 50):
            for sut0 in sorted({0, 1, interval // 2, interval}):
                for n in (0, 1, 6, 7, 8, 49, 50, 51, 257):
                    st = BatchedMetropolis(HostTarget(lambda Q: Q[:, :1], 1), [0.0], [1.0], 2, device=torch.device("cpu"),
                                           tune=tune, tune_interval=interval)
                    st.steps_until_tune, st.n_steps_total = sut0, 11
                    sut = sut0
                    for _ in range(n):
                        if tune and sut == 0:
                            sut = interval
                        sut -= 1
                    st._advance_counters(n)
                    assert (st.steps_until_tune, st.n_steps_total) == (sut, 11 + n), (tune, interval, sut0, n)


@pytest.mark.skipif(_gpu_present(), reason="GPU present")
def test_h4_no_cpu_fallback_without_gpu(golden):
    import beat_amd
    from beat_amd.models import HyperModel, estimate_hypers
    prob, _, _ = _mixed_problem(golden("hypers"))
    hm = HyperModel(prob)
    H, llks = np.zeros((2, hm.nh)), np.ones((2, hm.nterm))
    hm.set_llks(llks)
    with pytest.raises(beat_amd.BeatAmdError):
        hm.batch(H)
    with pytest.raises(beat_amd.BeatAmdError):
        hm.chain_batch(H, np.zeros((2, hm.nllk)), 3, np.ones(2), np.zeros(2, dtype=np.int32), hm.lower, hm.upper, 0,
                       np.ones(hm.nh), 1, 0, 0, 0, 0)
    with pytest.raises(beat_amd.BeatAmdError):
        hm.astep_batch(H, np.zeros((2, hm.nllk)), H, np.ones(2), hm.lower, hm.upper, np.zeros(2), 1.0)

    class _F(object):       # a compiled model cannot exist without a GPU: the entry fails before it is asked anything
        problem = prob
    with pytest.raises(beat_amd.BeatAmdError):
        estimate_hypers(_F(), n_chains=2, n_steps=3)
    with pytest.raises(beat_amd.BeatAmdError):
        prob.compile()


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_h5_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "beat_amd", "csrc", "hyper.hip")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "hyper.o")],
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
    for kern in ("k_hyper_logp", "k_hyper_chain"):
        hits = [v for k, v in seen.items() if kern in k]
        assert hits, "no resource report for %s:\n%s" % (kern, r.stdout[-2000:])
        assert hits == [0] * len(hits), "%s uses scratch: %s" % (kern, hits)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("nh", [1, 3, 70])
def test_h6_chain_case_visits_every_branch(kind, nh):
    """the inputs of the one-launch / step-by-step comparison (tests/test_gpu_hypers.py): in the numpy chain on the
    device's Philox streams at least 5 % of the proposals leave the box and at least 5 % are accepted"""
    model, llk, lower, upper = href.chain_case(nh)
    C = 65
    rng = np.random.default_rng(1)
    H = lower + (upper - lower) * rng.random((C, nh))
    out = href.chain(model, H, np.broadcast_to(llk, (C, nh)), lower, upper, kind, np.ones(nh), seed=12345, n_steps=257,
                     scaling=0.05, tune_interval=50, buffer_thinning=3)
    out_share, acc_share = 1.0 - out["inbox"].mean(), out["accepted"].mean()
    print("kind %d nh %d: %.1f %% out of the box, %.1f %% accepted" % (kind, nh, 100 * out_share, 100 * acc_share))
    assert out_share >= 0.05 and acc_share >= 0.05
    assert out["trace"].shape == (86, C, 2 * nh + 1)
    np.testing.assert_array_equal(out["trace"][-1], np.concatenate([out["H"], out["LL"]], axis=1))
