"""
Moment magnitudes and moment-rate functions, the host side (no GPU): the numpy restatement of the kernels
(tests/momentrate_ref.py) against the fixture written from the reference's own methods (tools/gen_golden_momentrate.py),
the argument checks that need no device, the exports, and the array logic of ``summary.moment_rate_ensemble``.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import momentrate_ref as mr

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = mr.load_cases(os.path.join(HERE, "golden", "moment_rate.npz"))
NAMES = sorted(CASES)


def test_fixture_has_the_cases_of_the_issue():
    assert NAMES == ["long", "single", "ties", "two", "wide"]
    assert CASES["long"]["patch_nt"].max() == 130               # crosses the 64-lane loop twice
    assert (CASES["ties"]["patch_nt"] == 1).any()               # duration < deltat / 2
    assert CASES["wide"]["k"].size == 70
    assert [str(c) for c in CASES["two"]["comps"]] == ["uparr", "uperp", "utens"]
    assert (CASES["two"]["M0"] == 0.0).sum() == 1 and (CASES["two"]["Mw"][CASES["two"]["M0"] == 0.0] == 0.0).all()
    assert CASES["two"]["time"].std(axis=1).min() > 0.0         # the subfaults' times differ


@pytest.mark.parametrize("name", NAMES)
def test_restatement_spans_and_supports_are_the_reference_s(name):
    case, a = CASES[name], mr.case_arrays(CASES[name])
    for c in range(a["Q"].shape[0]):
        sp = mr.spans(a["starts"][c], case["durations"][c], a["sub_off"], a["sub_n"], float(case["deltat"]))
        np.testing.assert_array_equal(sp, case["spans"][c])
        for p in range(a["P"]):
            k0, amp = mr.half_sinusoid(a["starts"][c, p], case["durations"][c, p], float(case["deltat"]))
            assert (k0, amp.size) == (case["patch_k0"][c, p], case["patch_nt"][c, p])
    assert int(case["kbase"]) == case["spans"][:, -1, 0].min()


def _rates(case, a, **kw):
    offs = [a["offs"][v] for v in ("uparr", "uperp")]
    NT = case["rates"].shape[2]
    return [mr.moment_rates(a["Q"][c], offs, case["k"], a["starts"][c], a["dur_off"], a["sub_off"], a["sub_n"],
                            float(case["deltat"]), int(case["kbase"]), NT, **kw) for c in range(a["Q"].shape[0])]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_rates_within_the_bound_of_the_reference(name):
    """the restatement differs from the reference by the normalisation order alone (fold64 vs numpy's pairwise sum)"""
    case, a = CASES[name], mr.case_arrays(CASES[name])
    worst = 0.0
    for c, (rates, cover, count) in enumerate(_rates(case, a)):
        bound = mr.rate_bound(case["rates"][c], cover, count)
        diff = np.abs(rates - case["rates"][c])
        assert (diff <= bound).all()
        assert ((rates != 0.0) <= (count > 0)).all()             # nothing outside the patches' supports
        worst = max(worst, mr.worst_ratio(diff, bound))
    print("%s: largest |diff| / bound = %.3f" % (name, worst))


def test_the_bound_catches_a_float32_cosine():
    """a float32 evaluation of the cosine misses the bound by orders of magnitude"""
    case, a = CASES["two"], mr.case_arrays(CASES["two"])
    cos32 = lambda x: np.cos(x.astype(np.float32)).astype(np.float64)   # noqa: E731
    worst = 0.0
    for c, (rates, cover, count) in enumerate(_rates(case, a, cos=cos32)):
        bound = mr.rate_bound(case["rates"][c], cover, count)
        worst = max(worst, mr.worst_ratio(rates - case["rates"][c], bound))
    assert worst > 1.0e5


@pytest.mark.parametrize("name", NAMES)
def test_restatement_magnitudes(name):
    case, a = CASES[name], mr.case_arrays(CASES[name])
    offs = [a["offs"][v] for v in a["comps"]]
    M0, Mw = mr.magnitudes(a["Q"], offs, case["k"])
    P = a["P"]
    assert (np.abs(M0 - case["M0"]) <= P * mr.EPS * np.abs(case["M0"])).all()
    assert (np.abs(Mw - case["Mw"]) <= 4 * mr.EPS * np.abs(case["Mw"])).all()
    assert ((M0 == 0.0) == (case["M0"] == 0.0)).all()


@pytest.mark.parametrize("name", NAMES)
def test_rates_sum_to_the_moment(name):
    case, a = CASES[name], mr.case_arrays(CASES[name])
    offs = [a["offs"][v] for v in ("uparr", "uperp")]
    for c, (rates, _, _) in enumerate(_rates(case, a)):
        m = mr.patch_moments(a["Q"][c], offs, case["k"]).sum()
        assert abs(rates[-1].sum() - m) <= (a["P"] + rates.shape[1]) * mr.EPS * m


def test_fold64_is_the_stated_order():
    rng = np.random.default_rng(3)
    a = rng.uniform(0, 1, 130)
    part = [0.0] * 64
    for i, v in enumerate(a):
        part[i % 64] = part[i % 64] + v
    n = 32
    while n:
        part = [part[l] + part[l + n] for l in range(n)]
        n //= 2
    assert mr.fold64(a) == part[0]


# ---- exports, argument checks that need no device
def test_exports_present():
    from beat_amd import _lib
    lib = _lib.load()
    for name in ("beatamd_ffi_magnitudes_batch", "beatamd_ffi_moment_rate_spans_batch", "beatamd_ffi_moment_rates_batch",
                 "beatamd_trace_density_update_ranges"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    header = open(os.path.join(HERE, "..", "include", "beat_amd.h")).read()
    for name in ("beatamd_ffi_magnitudes_batch", "beatamd_ffi_moment_rate_spans_batch", "beatamd_ffi_moment_rates_batch",
                 "beatamd_trace_density_update_ranges", "BEATAMD_STF_HALF_SINUSOID"):
        assert name in header
    assert header.count("UNVERIFIED") >= 2


def test_null_context_is_einval():
    from beat_amd import _lib
    lib = _lib.load()
    assert lib.beatamd_ffi_magnitudes_batch(None, 0, 0, None, None, None, 0, None, None) == _lib.EINVAL
    assert lib.beatamd_ffi_moment_rate_spans_batch(None, 0, 0, None, None, None, 0.5, None) == _lib.EINVAL
    assert lib.beatamd_ffi_moment_rates_batch(None, 0, 0, None, None, None, 0, None, None, 0.5, 0, 0, 1, None,
                                              None) == _lib.EINVAL
    assert lib.beatamd_trace_density_update_ranges(None, 0, 0, 2, None, None, 0.5, None, None, 4, 4, 1.0,
                                                   None) == _lib.EINVAL


class _Local(object):
    def __init__(self):
        self.calls = []

    def magnitudes(self, Q, k, components=None):
        self.calls.append(("magnitudes", Q, k, components))
        return "M"

    def moment_rates(self, Q, k, deltat, individual=False):
        self.calls.append(("moment_rates", Q, k, deltat, individual))
        return "R"


def test_sharded_model_delegates_to_the_local_model():
    from beat_amd.models.sharded import TargetShardedLogp
    f = TargetShardedLogp.__new__(TargetShardedLogp)
    f.local = _Local()
    assert f.magnitudes("Q", "k", ["uparr"]) == "M"
    assert f.moment_rates("Q", "k", 0.5, individual=True) == "R"
    assert f.local.calls == [("magnitudes", "Q", "k", ["uparr"]), ("moment_rates", "Q", "k", 0.5, True)]


def test_slip_component_names_are_checked():
    from beat_amd.models.problem import LogpForwFunc

    class _Lay(object):
        def offset(self, name, i):
            return {"uparr": 0, "uperp": 6}[name] + i

    f = LogpForwFunc.__new__(LogpForwFunc)
    f.problem = type("P", (), dict(layout=_Lay(), slip_varnames=["uparr", "uperp"]))()
    assert f._slip_offsets(None, "x") == [0, 6]
    assert f._slip_offsets(["uperp"], "x") == [6]
    with pytest.raises(ValueError, match="utens"):
        f._slip_offsets(["utens"], "x")
    with pytest.raises(ValueError):
        f._slip_offsets([], "x")


# ---- the array logic of summary.moment_rate_ensemble
def test_ensemble_extent_and_truncation_on_arrays():
    from beat_amd import summary
    case = CASES["two"]
    nsub = 2
    idx = summary.ensemble_indices(case["rates"].shape[0], 7)
    assert idx.tolist() == np.floor(np.arange(0, 24, 24.0 / 7)).astype("int32").tolist()
    # the fixture's extent is the reference's over every draw's own stretch (draw 3 has no slip: zeros inside its span)
    ext = summary.moment_rate_extent(case["rates"][:, nsub], case["spans"][:, nsub], int(case["kbase"]),
                                     float(case["deltat"]))
    np.testing.assert_array_equal(np.array(ext), case["density_extent"])
    # zeros outside a span do not count: a curve lifted by 1 inside its span alone has min_rates 1
    rates = np.zeros((2, 10))
    spans = np.array([[2, 3], [4, 4]])
    rates[0, 2:5] = [1.0, 3.0, 2.0]
    rates[1, 4:8] = [1.5, 5.0, 4.0, 1.25]
    assert summary.moment_rate_extent(rates, spans, 0, 0.5) == (1.0, 3.5, 1.0, 5.0)
    assert summary.moment_rate_extent(rates[:, 1:], spans, 1, 0.5) == (1.0, 3.5, 1.0, 5.0)
    with pytest.raises(ValueError):
        summary.moment_rate_extent(rates, np.array([[0, 0], [0, 0]]), 0, 0.5)
    grid = case["density_raw"].copy()
    assert (grid > 12).any()
    np.testing.assert_array_equal(summary.truncate_density(grid, 24), case["density"])
    assert grid.max() == 12.0


# ---- resources: no kernel of the feature spills
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
@pytest.mark.parametrize("source,kernels", [
    ("momentrate.hip", ("k_moment_magnitude", "k_moment_rate_span", "13k_moment_rateE", "k_moment_rate_total")),
    ("summary.hip", ("k_trace_density_check_ranged", "k_trace_density_ranged"))])
def test_kernels_use_no_scratch(tmp_path, source, kernels):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(HERE, "..", "beat_amd", "csrc", source)
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "out.o")],
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
    for kern in kernels:
        hits = [v for k, v in seen.items() if kern in k]
        assert hits, "no resource report for %s:\n%s" % (kern, r.stdout[-2000:])
        assert hits == [0] * len(hits), "%s uses scratch: %s" % (kern, hits)
