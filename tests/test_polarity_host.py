"""The polarity composite, host side: the numpy restatement of the kernel (tests/polarity_ref.py) and the host adaptors
(beat_amd.sources, beat_amd.heart, models.distributions.polarity_llk, models.polarity, pytensorf.PolaritySynthesizer)
against the reference's own numbers and 50-digit mpmath values (tests/golden/polarity.npz, written by
tools/gen_golden_polarity.py); the C ABI table, the argument rules and the refusals; no CPU fallback.

Bounds: polarity_ref.K_M6 / E_LLK (derived there).  Observed here (numpy, printed by the tests): the restatement's m6 lies
<= 6 units of 2^-53 from the mpmath values for every source kind (the reference's own: 6.0 mtqt, 4.0 mt, 8.75 dc)."""
import re
from collections import OrderedDict

import numpy as np
import pytest

import polarity_ref as pref
from conftest import ROOT, load_golden

KINDS = ("mtqt", "mt", "dc")
WAVES = ("any_P", "any_SV", "any_SH")


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _rw(g):
    return np.concatenate([g["rw_" + w] for w in WAVES], axis=1)


def test_fixture_shape():
    g = load_golden("polarity")
    c38 = 3.0 * np.pi / 8.0
    P = g["P_mtqt"]
    assert P.shape[1] == 5 and P.shape[0] - int(g["n_edge_mtqt"]) == 200
    for k in ("mt", "dc"):
        assert g["P_" + k].shape[0] - int(g["n_edge_" + k]) == 200
    assert np.all(np.abs(P[:, 0]) <= c38) and np.all(np.abs(P[:, 1]) <= 1.0 / 3.0) and np.all((P[:, 4] >= 0) & (P[:, 4] <= 1))
    for col, vals in ((4, (0.0, 1.0)), (2, (0.0, 2.0 * np.pi)), (3, (np.pi / 2, -np.pi / 2)), (1, (1.0 / 3.0, -1.0 / 3.0)),
                      (0, (c38, -c38, np.nextafter(c38, 0.0), np.nextafter(-c38, 0.0)))):
        for v in vals:
            assert (P[:, col] == v).any(), (col, v)
    # exact table nodes among the w values
    u = c38 - P[:, 0]
    assert np.isin(u, g["u_mapping"][1:-1]).sum() >= 3
    assert np.all(np.diff(g["u_mapping"]) > 0) and g["u_mapping"].size == 1000
    t, a = g["takeoff"], g["azimuth"]
    assert t.min() == 0.0 and t.max() == np.pi and (t > np.pi / 2).any() and a.min() == 0.0 and a.max() < 2 * np.pi
    assert set(np.unique(g["obs"])) == {-1, 0, 1} and float(g["gamma"]) == 0.2 and list(g["sigmas"]) == [0.05, 0.3, 2.0]


def test_tables_and_interp_restatement():
    """the tables the package builds are the reference's bit for bit; the step-by-step interpolation is numpy.interp"""
    from beat_amd import sources
    g = load_golden("polarity")
    assert np.array_equal(sources.U_MAPPING, g["u_mapping"]) and np.array_equal(sources.BETA_MAPPING, g["beta_mapping"])
    assert np.array_equal(pref.U_TABLE, g["u_mapping"]) and np.array_equal(pref.BETA_TABLE, g["beta_mapping"])
    w = g["w_to_beta_w"]
    assert np.array_equal(pref.w_to_beta(w), g["w_to_beta"])
    assert np.array_equal(sources.w_to_beta(w, u_mapping=sources.U_MAPPING, beta_mapping=sources.BETA_MAPPING), g["w_to_beta"])
    assert np.array_equal(sources.w_to_beta(w), g["w_to_beta"])
    assert np.array_equal(sources.v_to_gamma(g["P_mtqt"][:, 1]), g["v_to_gamma"])
    assert np.array_equal(sources.w_to_delta(w), np.pi / 2.0 - g["w_to_beta"])
    x = np.concatenate([g["u_mapping"][[0, 1, 500, 998, 999]], [-1.0, 3.0, np.nan], np.linspace(0, 2.4, 777)])
    got, want = pref.interp_numpy_steps(x, g["u_mapping"], g["beta_mapping"]), np.interp(x, g["u_mapping"], g["beta_mapping"])
    assert np.array_equal(got, want, equal_nan=True)


def test_mtqt_source_properties_vs_reference():
    from beat_amd.sources import MTQTSource
    g = load_golden("polarity")
    worst = 0.0
    for i, p in enumerate(g["P_mtqt"]):
        s = MTQTSource(w=p[0], v=p[1], kappa=p[2], sigma=p[3], h=p[4])
        assert s.rho == 1.0
        for name in ("beta", "gamma", "theta"):
            assert getattr(s, name) == g["mtqt_" + name][i], name
        for name in ("rot_U", "lune_lambda", "m9_nwu", "m9"):
            err = np.max(np.abs(getattr(s, name) - g["mtqt_" + name][i]))
            worst = max(worst, err)
            assert err <= 16 * pref.U2, (name, i, err)
        assert np.array_equal(s.m6, [s.m9[0, 0], s.m9[1, 1], s.m9[2, 2], s.m9[0, 1], s.m9[0, 2], s.m9[1, 2]])
    print("MTQTSource vs reference: <= %.2f units of 2^-53" % (worst / pref.U2))


def test_reference_test_table_values():
    """Tape & Tape (2015) Appendix A, the three-decimal values of the reference's test (test/test_sources.py:21-58)"""
    from beat_amd.sources import MTQTSource
    pi = np.pi
    u, v, kappa, sigma, h = 3.0 / 8.0 * pi, -1.0 / 9.0, 4.0 / 5.0 * pi, -pi / 2.0, 3.0 / 4.0
    mt = MTQTSource(w=3.0 / 8.0 * pi - u, v=v, kappa=kappa, sigma=sigma, h=h)
    np.testing.assert_allclose(mt.rho, 1.0)
    np.testing.assert_allclose([mt.beta, mt.gamma], [1.571, -0.113], atol=1e-3, rtol=0.0)
    np.testing.assert_allclose(mt.theta, [0.723], atol=1e-3, rtol=0.0)
    np.testing.assert_allclose(mt.rot_U, [[-0.587, -0.809, 0.037], [0.807, -0.588, -0.051], [0.063, 0.0, 0.998]], atol=1e-3, rtol=0.0)
    np.testing.assert_allclose(mt.lune_lambda, [0.749, -0.092, -0.656], atol=1e-3, rtol=0.0)
    nwu = [[0.196, -0.397, -0.052], [-0.397, 0.455, 0.071], [-0.052, 0.071, -0.651]]
    ned = [[0.196, 0.397, 0.052], [0.397, 0.455, 0.071], [0.052, 0.071, -0.651]]
    np.testing.assert_allclose(mt.m9_nwu, nwu, atol=1e-3, rtol=0.0)
    np.testing.assert_allclose(mt.m9, ned, atol=1e-3, rtol=0.0)
    # the restatement at the same point, scaled back from sqrt(sum m9^2) = sqrt 2 to rho = 1
    m = pref.m6("mtqt", [[0.0, v, kappa, sigma, h]])[0] / np.sqrt(2.0)
    np.testing.assert_allclose(m, [0.196, 0.455, -0.651, 0.397, 0.052, 0.071], atol=1e-3, rtol=0.0)


def test_radiation_weights_vs_reference_and_matmul():
    from beat_amd import heart
    from beat_amd.sources import symmat6
    g = load_golden("polarity")
    t, a = g["takeoff"], g["azimuth"]
    fun = {"any_P": heart.radiation_weights_p, "any_SV": heart.radiation_weights_sv, "any_SH": heart.radiation_weights_sh}
    for w in WAVES:
        assert np.array_equal(fun[w](t, a), g["rw_" + w])
        assert np.array_equal(heart.calculate_radiation_weights(t, a, w), g["rw_" + w])
    assert heart.radiation_gamma(t, a).shape == heart.radiation_theta(t, a).shape == heart.radiation_phi(a).shape == (3, t.size)
    # weights == matmul: the six-vector order is the tree's own
    for row, i in zip(g["matmul"], g["matmul_cases"]):
        m9 = g["mtqt_m9"][i]
        got = np.concatenate([heart.radiation_matmul(m9, t, a, w) for w in WAVES])
        assert np.max(np.abs(got - row)) <= 8 * pref.U2
        m6 = np.array([m9[0, 0], m9[1, 1], m9[2, 2], m9[0, 1], m9[0, 2], m9[1, 2]])
        assert np.max(np.abs(_rw(g).T.dot(m6) - got)) <= 8 * pref.U2
        assert np.array_equal(symmat6(*m6), m9) or np.max(np.abs(symmat6(*m6) - m9)) <= 2 * pref.U2   # (m9 symmetric to rounding)
    assert heart.radiation_matmul(np.eye(3), t, a, "any_X") is None


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_m6_vs_mpmath_and_reference(kind):
    g = load_golden("polarity")
    m = pref.m6(kind, g["P_" + kind])
    err = np.abs(m - g["mp_m6_" + kind])
    print("%s: restatement m6 %.2f units of 2^-53 from mpmath (reference %.2f), bound %g"
          % (kind, err.max() / pref.U2, float(g["ref_m6_units_" + kind]), pref.K_M6))
    assert np.all(err <= pref.bound_m6())
    assert np.all(np.abs(m - g["ref_m6_" + kind]) <= 2 * pref.bound_m6())
    assert np.max(np.abs(g["ref_m6_" + kind] - g["mp_m6_" + kind])) <= pref.bound_m6()
    ssq = (m[:, :3] ** 2).sum(1) + 2 * (m[:, 3:] ** 2).sum(1)
    assert np.all(np.abs(ssq - 2.0) <= 16 * pref.U2)


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_amplitudes_and_llk(kind):
    g = load_golden("polarity")
    rw, obs, gamma = _rw(g), g["obs"].astype(np.float64), float(g["gamma"])
    n_amp, n_llk = g["mp_amp_" + kind].shape[0], g["mp_llk_" + kind].shape[1]
    m = pref.m6(kind, g["P_" + kind][:n_amp])
    amp = pref.amplitudes(rw, m)
    bd = pref.bound_amplitudes(rw)[None]
    assert np.all(np.abs(amp - g["mp_amp_" + kind]) <= bd) and np.all(np.abs(amp - g["ref_amp_" + kind]) <= 2 * bd)
    worst = 0.0
    for k, sg in enumerate(g["sigmas"]):
        ll = pref.llk(obs, amp[:n_llk], gamma, sg)
        want = g["mp_llk_" + kind][k]
        bl = pref.bound_llk(rw, g["mp_amp_" + kind][:n_llk], want, gamma, sg)
        assert np.all(np.abs(ll - want) <= bl) and np.all(np.abs(ll - g["ref_llk_" + kind][k]) <= 2 * bl)
        worst = max(worst, float(np.max(np.abs(ll - want) / bl)))
    print("%s: llk at most %.3f of its bound from mpmath" % (kind, worst))


def test_host_adaptors_pol_synthetics_and_llk():
    """heart.pol_synthetics and distributions.polarity_llk with the reference's signatures, one source at a time"""
    from beat_amd import heart
    from beat_amd.models.distributions import polarity_llk
    from beat_amd.sources import DCSource, MTQTSource, MTSource
    g = load_golden("polarity")
    rw, obs, gamma = _rw(g), g["obs"], float(g["gamma"])
    bd = pref.bound_amplitudes(rw)
    cls = {"mtqt": lambda p: MTQTSource(w=p[0], v=p[1], kappa=p[2], sigma=p[3], h=p[4]), "mt": lambda p: MTSource(*p),
           "dc": lambda p: DCSource(*p)}
    for kind in KINDS:
        for i in list(range(int(g["n_edge_" + kind]))) + [int(g["n_edge_" + kind]) + 3]:
            amp = heart.pol_synthetics(cls[kind](g["P_" + kind][i]), radiation_weights=rw)
            assert np.all(np.abs(amp - g["ref_amp_" + kind][i]) <= 2 * bd), (kind, i)
            for k, sg in enumerate(g["sigmas"]):
                ll = polarity_llk(obs, g["ref_amp_" + kind][i], gamma, sg)
                assert np.array_equal(ll, g["ref_llk_" + kind][k, i])
    n = g["takeoff"].size
    a = heart.pol_synthetics(cls["dc"]((30.0, 60.0, 20.0)), g["takeoff"], g["azimuth"], wavename="any_SH")
    assert np.array_equal(a, heart.pol_synthetics(cls["dc"]((30.0, 60.0, 20.0)), radiation_weights=g["rw_any_SH"])) and a.shape == (n,)
    with pytest.raises(ValueError, match="radiation weights"):
        heart.pol_synthetics(cls["dc"]((30.0, 60.0, 20.0)))


def test_dc_equals_mtqt_at_w_v_zero():
    """(strike, dip, rake) == MTQT(w = v = 0, kappa = strike, sigma = rake, h = cos dip) after the normalisation.  h = cos(dip)
    carries half an ulp of 1, which acos amplifies by 1 / sin(dip): the tolerance is that term plus the two chains' own"""
    rng = np.random.RandomState(5)
    n = 300
    P = np.stack([rng.uniform(0, 360, n), rng.uniform(5, 90, n), rng.uniform(-90, 90, n)], axis=1)
    d2r = np.pi / 180.0
    Q = np.stack([np.zeros(n), np.zeros(n), P[:, 0] * d2r, P[:, 2] * d2r, np.cos(P[:, 1] * d2r)], axis=1)
    a, b = pref.m6("dc", P), pref.m6("mtqt", Q)
    tol = (2 * pref.K_M6 + 8.0 / np.sin(P[:, 1] * d2r)) * pref.U2
    err = np.abs(a - b).max(axis=1)
    print("dc vs mtqt: %.2f units of 2^-53 at most" % (err.max() / pref.U2))
    assert np.all(err <= tol) and err.max() < 64 * pref.U2
    from beat_amd.sources import dc_m6
    got = np.array([dc_m6(*p) for p in P])
    ssq = (got[:, :3] ** 2).sum(1) + 2 * (got[:, 3:] ** 2).sum(1)
    assert np.all(np.abs(ssq - 2.0) <= 16 * pref.U2)          # the Aki & Richards tensor has the unit scale already
    assert np.all(np.abs(got - a) <= 16 * pref.U2)


def _problem(kind="mtqt", sampled_location=False, geodetic=None, **kw):
    from beat_amd.models import ParameterLayout, PolarityMap, PolarityProblem
    g = load_golden("polarity")
    names = {"mtqt": ["kappa", "sigma", "h"], "mt": ["mnn", "mee", "mdd", "mne", "mnd", "med"], "dc": ["strike", "dip", "rake"]}.get(kind, ["kappa"])
    sizes = OrderedDict((n, 1) for n in names)
    sizes["h_any_SH_pol_1"] = 1
    if sampled_location:
        sizes["depth"] = 1
    layout = ParameterLayout(sizes)
    n = g["takeoff"].size
    maps = [PolarityMap("any_P", g["takeoff"], g["azimuth"], g["obs"][:n]),
            PolarityMap("any_SH", g["takeoff"], g["azimuth"], g["obs"][2 * n:])]
    fixed = {"w": 0.0, "v": 0.0, "h_any_P_pol_0": 0.05, "north_shift": 0.0, "east_shift": 0.0}
    return PolarityProblem(layout, kind, maps, fixed=fixed, **kw), g


def test_problem_tables_names_and_rules():
    from beat_amd.models import PolarityMap, polarity_hyper_name
    prob, g = _problem()
    assert prob.hyper_names == ["h_any_P_pol_0", "h_any_SH_pol_1"] and polarity_hyper_name("any_P", 0) == "h_any_P_pol_0"
    assert prob.out_names == ["polarity_like", "like"] and prob.n_t == 2 * g["takeoff"].size and prob.gamma == 0.2
    off, fix = prob.source_tables()
    assert off.tolist() == [-1, -1, 0, 1, 2, -1] and fix.tolist() == [0.0] * 6
    hoff, hfix = prob.hyper_tables()
    assert hoff.tolist() == [-1, 3] and hfix.tolist() == [0.05, 0.0]
    rw = prob.radiation_weights()
    assert np.array_equal(rw, np.concatenate([g["rw_any_P"], g["rw_any_SH"]], axis=1)) and rw.flags.c_contiguous
    assert prob.observations().dtype == np.float64 and prob.maps[0].dataset.dtype == np.int16
    src = prob.source({"kappa": 1.0, "sigma": 0.3, "h": 0.5})
    assert (src.w, src.v, src.kappa, src.sigma, src.h) == (0.0, 0.0, 1.0, 0.3, 0.5)
    with pytest.raises(NotImplementedError, match="source location"):
        _problem(sampled_location=True)
    with pytest.raises(ValueError, match="unknown polarity source kind"):
        _problem(kind="rectangular")
    with pytest.raises(ValueError, match="wave type"):
        PolarityMap("any_Q", [0.1], [0.2], [1])
    with pytest.raises(ValueError, match=r"\+1, -1 or 0"):
        PolarityMap("any_P", [0.1], [0.2], [2])
    with pytest.raises(ValueError, match="takeoff angles"):
        PolarityMap("any_P", [0.1, 0.2], [0.2], [1])
    with pytest.raises(ValueError, match="hyper-parameter names"):
        _problem(hypers=["h_any_P_pol_0"])
    bad, _ = _problem(hypers=["h_any_P_pol_0", "h_missing"])
    with pytest.raises(KeyError, match="neither sampled nor fixed"):
        bad.hyper_tables()


def test_argument_rules_of_the_binding():
    from beat_amd.polarity_binding import check_polarity_source as chk
    k, off, fix, ntab, u, b = chk("mtqt", [-1, -1, 0, 1, 2, -1], np.zeros(6), nparams=4)
    assert (k, ntab) == (0, 1000) and off.dtype == np.int64 and u.size == b.size == 1000
    assert chk("mt", -np.ones(6), np.zeros(6))[0] == 1 and chk("dc", -np.ones(6), np.zeros(6))[3:] == (0, None, None)
    with pytest.raises(ValueError, match="unknown polarity source kind"):
        chk("okada", -np.ones(6), np.zeros(6))
    with pytest.raises(ValueError, match="six slots"):
        chk("mt", -np.ones(5), np.zeros(6))
    with pytest.raises(ValueError, match="outside q"):
        chk("mt", [0, 1, 2, 3, 4, 5], np.zeros(6), nparams=5)
    with pytest.raises(ValueError, match="outside q"):
        chk("mt", [-2, 1, 2, 3, 4, 5], np.zeros(6))
    with pytest.raises(ValueError, match="strictly increasing"):
        chk("mtqt", -np.ones(6), np.zeros(6), tables=(np.array([0.0, 1.0, 1.0]), np.zeros(3)))
    with pytest.raises(ValueError, match="one length"):
        chk("mtqt", -np.ones(6), np.zeros(6), tables=(np.array([0.0, 1.0]), np.zeros(3)))


def test_refusals_name_the_composite():
    from beat_amd.models import HyperModel, estimate_hypers
    from beat_amd.models.sharded import TargetShardedLogp
    from beat_amd.models.lsq import lsq_start_population
    from beat_amd.models.problem import LogpForwFunc, refuse_polarity
    from beat_amd.pytensorf import PolaritySynthesizer
    prob, _ = _problem()
    refuse_polarity(object(), "anything")            # a problem without the composite passes
    f = LogpForwFunc.__new__(LogpForwFunc)           # (no device: the refusals come before any device call)
    f.problem, f.model_id, f._dirty, f.nparams = prob, 0, None, prob.layout.size
    Q = np.zeros((2, prob.layout.size))
    for call in (lambda: f.update_llks(Q), lambda: f.variance_reductions(Q), lambda: f.obs_quads(),
                 lambda: f.standardized_residuals(Q, []), lambda: f.lsq_solution(Q), lambda: f.lsq_normal_equations(Q),
                 lambda: lsq_start_population(f, 4, 1), lambda: HyperModel(f), lambda: estimate_hypers(f),
                 lambda: TargetShardedLogp(prob)):
        with pytest.raises(NotImplementedError, match="polarity composite"):
            call()
    with pytest.raises(NotImplementedError, match="free source location"):
        PolaritySynthesizer(None, None, prob.maps[0], False, False)


def test_polarity_synthesizer_protocol():
    from beat_amd import heart
    from beat_amd.pytensorf import PolaritySynthesizer
    from beat_amd.sources import MTQTSource
    prob, g = _problem()
    op = PolaritySynthesizer(None, MTQTSource(), prob.maps[1], True, False)
    assert op.__props__ == ("engine", "source", "pmap", "is_location_fixed", "always_raytrace")
    assert op.infer_shape() == [(prob.maps[1].n_t,)]
    point = OrderedDict([("kappa", np.array([1.1])), ("sigma", np.array([-0.4])), ("h", np.array([0.3])), ("w", 0.1), ("v", -0.2),
                         ("depth", 5.0), ("h_any_SH_pol_1", 0.3)])
    got = op(point)
    want = heart.pol_synthetics(MTQTSource(w=0.1, v=-0.2, kappa=1.1, sigma=-0.4, h=0.3), radiation_weights=g["rw_any_SH"])
    assert np.array_equal(got, want) and op.varnames == list(point)
    out = [[None]]
    op.perform(None, list(point.values()), out)
    assert np.array_equal(out[0][0], want)


def test_symbols_declared_exported_and_bound():
    from beat_amd import _lib
    hdr = open(ROOT + "/include/beat_amd.h").read()
    for name, nargs in (("beatamd_ffi_model_add_polarity", 15), ("beatamd_mt6_batch", 11),
                        ("beatamd_polarity_amplitudes_batch", 13), ("beatamd_w_to_beta_batch", 7)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
        assert name in _lib.EXPORTS and len(_lib._PROTOS[name]) == nargs
        assert hasattr(_lib.load(), name)
    for k, v in (("BEATAMD_POL_MTQT", 0), ("BEATAMD_POL_MT", 1), ("BEATAMD_POL_DC", 2)):
        assert re.search(r"#define %s %d\b" % (k, v), hdr)
    assert (_lib.POL_MTQT, _lib.POL_MT, _lib.POL_DC) == (0, 1, 2)
    assert _lib.ABI_VERSION == 120 and "BEATAMD_VERSION 120" in re.sub(r"\s+", " ", hdr)
    src = open(ROOT + "/beat_amd/csrc/polarity.hip").read()
    for ref in ("sources.py:454-536", "heart.py:4086-4087", "distributions.py:143-173", "polarity.py:104-134"):
        assert ref in src
    for ref in ("sources.py:379-392", "heart.py:4053-4088", "polarity.py:104-134", "distributions.py:143-173"):
        assert ref in hdr


@pytest.mark.skipif(_gpu_present(), reason="GPU present")
def test_no_cpu_fallback_without_gpu():
    import beat_amd
    prob, g = _problem()
    with pytest.raises(beat_amd.BeatAmdError):
        prob.compile()
    with pytest.raises(beat_amd.BeatAmdError):
        from beat_amd.polarity_binding import w_to_beta_batch
        w_to_beta_batch(beat_amd.get_context(), g["w_to_beta_w"])
