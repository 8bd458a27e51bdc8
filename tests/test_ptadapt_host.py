"""CPU tests of the PT proposal adaptation: the numpy restatement of the streaming weighted moments (tests/ptadapt_ref.py)
against the reference's calc_sample_covariance (tests/golden/pt_proposal.npz, tools/gen_golden_ptcov.py), its HostOps
twin, the window bookkeeping of pt_sample against a plain restatement of beat/sampler/base.py:356-393, and the C ABI table."""
import os
import re

import numpy as np
import pytest

import ptadapt_ref as ref
from conftest import ROOT, load_golden

CASES = ("n1", "n5", "n7", "n17", "n33")


@pytest.fixture(scope="module")
def fix():
    return load_golden("pt_proposal")


def _case(fix, name):
    steps, R = (int(v) for v in fix[name + "_shape"])
    return fix[name + "_X"], fix[name + "_like"], steps, R


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_covariance(fix, name):
    """|cov - fixture|_ij <= 3 (N_s + 8) 2^-53 a_i a_j (ptadapt_ref.cov_bound).  The fixture of every case is the
    reference's calc_sample_covariance, except n1: the reference raises for one parameter (numpy.cov's 0-d result), the
    fixture holds the numpy.cov call it makes (tools/gen_golden_ptcov.py)."""
    X, like, steps, R = _case(fix, name)
    st, r0 = ref.window_state(X, like, steps, R)
    cov, flags = ref.finish(st, X.shape[1])
    assert flags[0] == 0 and st[0, 3] == steps * R and st[0, 4] == 0
    bound = ref.cov_bound(X, like, r0[0])
    frac = np.abs(cov[0] - fix[name + "_cov"]) / bound
    print("%s: largest |dcov| / bound = %.3g" % (name, frac.max()))
    assert (frac <= 1.0).all(), frac.max()
    F = np.zeros((1, X.shape[1], X.shape[1]))
    _, flags = ref.factor(st, X.shape[1], F)
    assert flags[0] == 0
    np.testing.assert_allclose(F[0].T @ F[0], cov[0], rtol=0, atol=1e-12 * np.abs(cov[0]).max())


@pytest.mark.parametrize("name", ("spike", "single"))
def test_degenerate_windows_are_flagged(fix, name):
    """the reference returns None for both (the generator asserts it): flag 1, the previous factor stays"""
    X, like, steps, R = _case(fix, name)
    st, _ = ref.window_state(X, like, steps, R)
    F = np.full((1, 5, 5), 7.0)
    _, flags = ref.factor(st, 5, F)
    assert flags[0] == 1 and (F == 7.0).all()


def _host_ops():
    from beat_amd.sampler.ops import HostOps
    return HostOps()


def test_hostops_twin_matches_restatement(fix):
    import torch
    ops = _host_ops()
    rng = np.random.default_rng(3)
    G, R, n, steps = 3, 5, 7, 9
    Q = 10.0 + rng.standard_normal((steps, G * R, n))
    like = -5.0 * rng.uniform(size=(steps, G * R))
    like[4, 5:10] += 8.0                     # a rescale on the way (group 1)
    Q[6, 2, 3] = np.nan                      # skipped rows, counted
    like[2, 11] = np.inf
    st_t = ops.group_moments_alloc(G, n)
    ref_t = torch.zeros((G, n), dtype=torch.float64)
    ops.group_moments_reset(st_t, n, torch.from_numpy(Q[0]), ref_t)
    st = ref.new_state(G, n)
    r0 = ref.group_ref(Q[0], G)
    assert np.array_equal(ref_t.numpy(), r0)
    for t in range(steps):
        L = torch.from_numpy(np.stack([np.zeros(G * R), like[t]], axis=1))   # like: the strided last column
        ops.group_moments_update(st_t, torch.from_numpy(Q[t]), L[:, -1], ref_t)
        ref.update(st, Q[t], like[t], r0)
    assert np.array_equal(st_t.numpy()[:, 3:5], st[:, 3:5]) and st[0, 4] == 1 and st[2, 4] == 1 and st[1, 4] == 0
    np.testing.assert_allclose(st_t.numpy(), st, rtol=1e-12, atol=1e-13)
    F = torch.full((G, n, n), 7.0, dtype=torch.float64)
    _, cov, flags = ops.group_moments_factor(st_t, n, F, want_cov=True)
    F_r = np.full((G, n, n), 7.0)
    cov_r, flags_r = ref.factor(st, n, F_r)
    assert flags.numpy().tolist() == flags_r.tolist() == [1, 0, 1]
    np.testing.assert_allclose(cov.numpy()[1], cov_r[1], rtol=1e-10, atol=0)
    np.testing.assert_allclose(F.numpy()[1], F_r[1], rtol=1e-9, atol=1e-12)
    assert (F.numpy()[[0, 2]] == 7.0).all()
    # the reset empties the state
    ops.group_moments_reset(st_t, n)
    assert np.array_equal(st_t.numpy(), ref.new_state(G, n))
    # fixture window through the twin
    X, lk, steps, R = _case(fix, "n17")
    st1 = ops.group_moments_alloc(1, 17)
    r1 = torch.zeros((1, 17), dtype=torch.float64)
    X3, l2 = X.reshape(steps, R, 17), lk.reshape(steps, R)
    ops.group_moments_reset(st1, 17, torch.from_numpy(X3[0]), r1)
    for t in range(steps):
        ops.group_moments_update(st1, torch.from_numpy(X3[t]), torch.from_numpy(l2[t]), r1)
    _, cov, flags = ops.group_moments_factor(st1, 17, torch.zeros((1, 17, 17), dtype=torch.float64), want_cov=True)
    assert int(flags[0]) == 0
    assert (np.abs(cov.numpy()[0] - fix["n17_cov"]) <= ref.cov_bound(X, lk, r1.numpy()[0])).all()


def test_hostops_grouped_draw():
    import torch
    ops = _host_ops()
    rng = np.random.default_rng(1)
    F = torch.from_numpy(np.triu(rng.standard_normal((3, 4, 4))))
    d, lu = ops.draw(F, 6, 5, 11, first_chain=2, groups=3)
    for g in range(3):
        d1, lu1 = ops.draw(F[g], 6, 5, 11, first_chain=2)
        np.testing.assert_allclose(d.numpy()[2 * g:2 * g + 2], d1.numpy()[2 * g:2 * g + 2], rtol=1e-14, atol=1e-15)
        assert np.array_equal(lu.numpy(), lu1.numpy())
    with pytest.raises(ValueError):
        ops.draw(F, 7, 5, 11, groups=3)


class CountingTarget(object):
    """a Gaussian whose evaluations are counted (HostTarget interface)"""

    def __init__(self, n):
        from beat_amd.sampler.hosttarget import HostTarget
        self.calls = 0
        self._t = HostTarget(self._like, n)
        self.nparams, self.nllk = n, 1

    def _like(self, q):
        self.calls += 1
        return -0.5 * ((q / 0.3) ** 2).sum(1)

    def batch(self, Q, out=None):
        return self._t.batch(Q, out)

    def astep_batch(self, *a, **k):
        return self._t.astep_batch(*a, **k)


def _run_counting(monkeypatch, **kw):
    from beat_amd.sampler import pt as ptmod
    intervals = []
    orig = ptmod.TemperingManager.draw_swap_interval

    def recording(self):
        intervals.append(orig(self))
        return intervals[-1]
    monkeypatch.setattr(ptmod.TemperingManager, "draw_swap_interval", recording)
    t = CountingTarget(3)
    out = ptmod.pt_sample(t, -2 * np.ones(3), 2 * np.ones(3), n_chains_posterior=1, n_chains_tempered=2, n_replicas=4,
                          n_samples=80, swap_interval=(3, 6), proposal_cov=kw.pop("proposal_cov", np.eye(3) * 0.05),
                          random_seed=9, **kw)
    return out, intervals, t


def test_window_bookkeeping_follows_the_reference(monkeypatch):
    (s, ls, man), intervals, t = _run_counting(monkeypatch, update_proposal=True, buffer_size=7, burnin=10)
    assert set(intervals) <= {3, 4, 5} and len(set(intervals)) > 1
    assert t.calls == 1 + sum(intervals) == 1 + man.loop_steps
    closed, updated = ref.window_closings(intervals, 7, 10)
    # keep_last: the first window closes after 7 steps, the later ones after 6 new samples each
    assert closed[:3] == [7, 13, 19] and man.windows_closed == closed
    # the burn-in decision belongs to the round: step 13 lies beyond burnin = 10, but counts only if its round began there
    assert [u[0] for u in man.proposal_updates] == updated and 0 < len(updated) < len(closed)
    assert updated[0] > 10 and all(isinstance(u[1], np.ndarray) and u[1].shape == (3,) for u in man.proposal_updates)
    assert man.proposal_factors is not None and tuple(man.proposal_factors.shape) == (3, 3, 3)


@pytest.mark.parametrize("family", ("Normal", "Laplace"))
def test_per_parameter_families_never_update(monkeypatch, family):
    (s, ls, man), intervals, t = _run_counting(monkeypatch, update_proposal=True, buffer_size=7, burnin=10,
                                               proposal_name=family, proposal_cov=0.2 * np.ones(3))
    assert man.proposal_updates == [] and man.windows_closed == [] and man.proposal_factors is None


def _toy(**kw):
    from beat_amd.sampler import pt_sample
    from beat_amd.sampler.hosttarget import HostTarget
    from test_samplers_cpu import _two_gaussians   # the toy of test_pt_manager_and_toy_sampling
    f, n = _two_gaussians()
    return pt_sample(HostTarget(f, n), -2 * np.ones(n), 2 * np.ones(n), n_chains_posterior=2, n_chains_tempered=6,
                     n_replicas=8, swap_interval=(20, 40), beta_tune_interval=5, proposal_cov=np.eye(n) * 0.02,
                     random_seed=5, **kw)


def test_default_run_is_unchanged():
    s0, l0, man0 = _toy(n_samples=300)
    s1, l1, man1 = _toy(n_samples=300, update_proposal=False)
    assert np.array_equal(s0, s1) and np.array_equal(l0, l1) and man0.history == man1.history
    # adaptation switched on, but burn-in beyond the run: windows close, nothing is ever updated
    s2, l2, man2 = _toy(n_samples=300, update_proposal=True, buffer_size=50, burnin=10 ** 6)
    assert np.array_equal(s0, s2) and np.array_equal(l0, l2) and man0.history == man2.history
    assert man2.proposal_updates == [] and len(man2.windows_closed) > 0 and man2.proposal_factors is None


def test_adapting_run_still_finds_both_modes():
    s, ls, man = _toy(n_samples=1500, update_proposal=True, buffer_size=50, burnin=100)
    assert s.shape == (1500, 4)
    np.testing.assert_allclose(np.abs(s[300:]).mean(axis=0), 0.5, rtol=0, atol=0.06)
    assert len(man.proposal_updates) > 0
    assert all((fl == 0).all() for _, fl in man.proposal_updates)
    F = man.proposal_factors.numpy()
    assert F.shape == (8, 4, 4) and not np.array_equal(F[0], F[7])


def test_temperatures_must_not_straddle_ranks(monkeypatch):
    from beat_amd import parallel
    from beat_amd.sampler import pt_sample
    t = CountingTarget(3)
    kw = dict(n_chains_posterior=1, n_chains_tempered=2, n_samples=20, swap_interval=(3, 6), random_seed=9)
    monkeypatch.setattr(parallel, "ensure_group", lambda: (1, 2, 0))     # 3 temperatures x 4 replicas on 2 ranks: 6 | 6
    with pytest.raises(ValueError, match="cut a temperature"):
        pt_sample(t, -2 * np.ones(3), 2 * np.ones(3), n_replicas=4, update_proposal=True, buffer_size=7, burnin=3, **kw)
    assert t.calls == 0                                                  # before any sampling
    # (a per-parameter family never adapts: nothing to check, and the straddling split samples as before)
    monkeypatch.setattr(parallel, "ensure_group", lambda: (0, 1, 0))
    pt_sample(t, -2 * np.ones(3), 2 * np.ones(3), n_replicas=4, update_proposal=True, buffer_size=7, burnin=3, **kw)
    assert t.calls > 0


def test_abi_table_has_the_new_entries():
    from beat_amd import _lib
    from beat_amd.engine import Context
    hdr = open(os.path.join(ROOT, "include", "beat_amd.h")).read()
    for name, nargs in (("beatamd_group_moments_reset", 7), ("beatamd_group_moments_update", 9),
                        ("beatamd_group_moments_factor", 7), ("beatamd_proposal_draw_grouped", 12),
                        ("beatamd_ffi_mstep_batch_grouped", 20)):
        assert name in _lib._PROTOS and name in _lib.EXPORTS, name
        assert len(_lib._PROTOS[name]) == nargs, (name, nargs, len(_lib._PROTOS[name]))
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert decl.count(",") + 1 == nargs, name
    for cite in ("beat/sampler/pt.py:758-761", "beat/sampler/base.py:363-393", "beat/backend.py:249-268",
                 "beat/covariance.py:865-909"):
        assert cite in hdr, cite
    assert _lib.ABI_VERSION == 120
    for m in ("group_moments_reset", "group_moments_update", "group_moments_factor", "proposal_draw_grouped",
              "ffi_mstep_batch_grouped"):
        assert callable(getattr(Context, m))
    assert Context.group_moments_stride(5) == ref.stride(5) == 38
