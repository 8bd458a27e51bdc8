"""
Parallel tempering -- counterpart of beat/sampler/pt.py.

The reference runs one MPI rank per tempered chain in a master/worker star: workers
sample a random number of Metropolis steps, send their last point to the master, which
pairs the first two arrivals and applies ``propose_chain_swap`` (:429-457).  Here all
replicas of a rank advance in ONE batched device call per step (per-replica beta), and the
exchange is a synchronous round: an all-gather of one likelihood per replica (RCCL), the same
even/odd adjacent-temperature swap sweep on every rank with a shared RandomState, and the swapped
states moved where they live (device gather; point to point only across rank boundaries).  The
swap rule, the beta ladder (``update_betas`` :179-221), the beta tuning (``tune_betas``
:331-354, ``tune`` :37-73) and the swap interval draw are the reference's; the pairing
order differs (asynchronous first-arrivals are not reproducible) -- statistical, not bit,
parity.

Proposal adaptation (``update_proposal``): every reference worker re-learns its multivariate proposal from its own trace
each time its buffer of ``buffer_size`` samples fills (``sample_pt_chain`` :758-761, ``_iter_sample`` base.py:363-393,
``calc_sample_covariance`` covariance.py:865-909).  Here a temperature is a group of ``n_replicas`` chains; the window's
likelihood-weighted moments are accumulated on the device after every step (``ProposalWindows``, csrc/ptadapt.hip) and
each temperature steps with its own factor (``BatchedMetropolis.set_group_proposals``).
"""
import numpy as np

from .. import parallel
from .._marshal import upload
from ..utility import ensure_cov_psd
from .base import univariate_proposals
from .metropolis import BatchedMetropolis


def tune(scale, acc_rate):
    """pt.py:37-73"""
    if acc_rate < 0.001:
        scale *= 0.85
    elif acc_rate < 0.05:
        scale *= 0.9
    elif acc_rate < 0.2:
        scale *= 0.95
    elif acc_rate > 0.95:
        scale *= 1.15
    elif acc_rate > 0.75:
        scale *= 1.10
    elif acc_rate > 0.5:
        scale *= 1.05
    return scale


def propose_chain_swap(beta1, beta2, llk1, llk2, log_u):
    """pt.py:429-457: alpha = (beta2 - beta1) * (llk1 - llk2); accept iff log(u) < alpha"""
    return log_u < (beta2 - beta1) * (llk1 - llk2)


class TemperingManager(object):
    """Ladder and swap bookkeeping (pt.py:101-470) for ``n_ladders`` temperatures x
    ``n_replicas`` independent replicas per temperature (BASELINE config 5: 32 x 256).
    Replica r of temperature k is global chain k * n_replicas + r."""

    def __init__(self, n_workers_posterior, n_workers_tempered, n_replicas=1,
                 swap_interval=(100, 300), beta_tune_interval=1000, random_seed=17):
        self.n_workers_posterior = int(n_workers_posterior)
        self.n_workers_tempered = int(n_workers_tempered)
        self.n_workers = self.n_workers_posterior + self.n_workers_tempered
        self.n_replicas = int(n_replicas)
        self.swap_interval = swap_interval
        self.beta_tune_interval = beta_tune_interval
        self._t_scale_min, self._t_scale_max = 1.01, 2.0
        self.current_scale = 1.2
        self.rng = np.random.RandomState(random_seed)  # shared by all ranks
        self.acceptance_matrix = np.zeros((self.n_workers, self.n_workers), dtype="int64")
        self.sample_count = np.zeros_like(self.acceptance_matrix)
        self.history = []
        self.update_betas()
        self._round = 0

    def update_betas(self, t_scale=None):
        """pt.py:179-221: betas = [1]*n_posterior + t_scale**-k, k = 1..n_tempered"""
        if t_scale is None:
            t_scale = self.current_scale
        self.current_scale = t_scale
        temperature = np.power(t_scale, np.arange(1, self.n_workers_tempered + 1))
        self.betas = np.array([1.0] * self.n_workers_posterior + (1.0 / temperature).tolist())
        return self.betas

    @property
    def chain_betas(self):
        return np.repeat(self.betas, self.n_replicas)

    def draw_swap_interval(self):
        """DiscreteBoundedUniform(lower, upper) (pt.py:149-152, config.py:1728-1738)"""
        lo, up = self.swap_interval
        return int(self.rng.randint(low=up - lo) + lo) if up > lo else int(lo)

    def swap_round(self, like):
        """One synchronous exchange sweep.  like (n_workers*n_replicas,) -> permutation p with
        new_state[i] = old_state[p[i]].  Even rounds pair ladders (0,1),(2,3).., odd rounds
        (1,2),(3,4)..; every replica column is an independent ladder."""
        K, R = self.n_workers, self.n_replicas
        perm = np.arange(K * R)
        like = np.asarray(like).reshape(K, R)
        start = self._round % 2
        logu = np.log(self.rng.uniform(size=(K, R)))
        for k in range(start, K - 1, 2):
            acc = propose_chain_swap(self.betas[k], self.betas[k + 1], like[k], like[k + 1], logu[k])
            self.sample_count[k, k + 1] += R
            self.sample_count[k + 1, k] += R
            n = int(acc.sum())
            self.acceptance_matrix[k, k + 1] += n
            self.acceptance_matrix[k + 1, k] += n
            a = k * R + np.nonzero(acc)[0]
            b = a + R
            perm[a], perm[b] = b, a
        self._round += 1
        return perm

    def get_acceptance_swap(self, k):
        c = self.sample_count[k, k + 1]
        return self.acceptance_matrix[k, k + 1] / float(c) if c else 0.0

    def tune_betas(self):
        """pt.py:331-354: acceptance between the posterior level and the first tempered
        level drives the temperature scale (inverse behaviour of step scaling)."""
        k = max(self.n_workers_posterior - 1, 0)
        acceptance = self.get_acceptance_swap(k)
        t_scale = min(max(tune(self.current_scale, acceptance), self._t_scale_min), self._t_scale_max)
        self.history.append((self.current_scale, acceptance))
        self.acceptance_matrix[:] = 0
        self.sample_count[:] = 0
        return self.update_betas(t_scale)


class ProposalWindows(object):
    """The trace buffers of the temperatures of one rank, as far as the proposal update reads them (backend.py:235-268,
    base.py:363-393): a window per temperature slot collects the states of its ``n_replicas`` chains after every step as
    streaming weighted moments; when it holds ``buffer_size`` samples it is closed -- the proposals are re-learned from it
    iff the round it closes in began after burn-in (``begin_round``) --, emptied, and the last sample put back as the first
    of the next window (keep_last).  Windows stay with the slot through swaps, as a worker's trace stays with the worker.

    A group whose covariance does not factor (flag 2) is repaired on the host alone: ``utility.ensure_cov_psd`` and a numpy
    Cholesky; a group with degenerate or non-finite moments (flag 1), or one whose repair fails, keeps its proposal (the
    reference's cov = None).  Unlike the reference, which passes EVERY matrix through ensure_cov_psd, the factorisation
    decides which matrices are repaired."""

    def __init__(self, stepper, n_groups, nparams, buffer_size, burnin, updates, closed):
        if int(buffer_size) < 2:
            raise ValueError("update_proposal: buffer_size must be at least 2")
        self.stepper, self.ops, self.torch = stepper, stepper.ops, stepper.torch
        self.G, self.n = int(n_groups), int(nparams)
        self.buffer_size, self.burnin = int(buffer_size), int(burnin)
        self.updates, self.closed = updates, closed
        self.count, self.update = 0, False
        self.state = self.ops.group_moments_alloc(self.G, self.n) if self.G else None
        self.ref = self.torch.zeros((self.G, self.n), dtype=self.torch.float64, device=stepper.device)
        # every temperature starts from the proposal of set_proposal; the stepper takes the grouped path from the first update
        self.factors = stepper.factor.unsqueeze(0).repeat(self.G, 1, 1).contiguous()

    def begin_round(self, steps_taken):
        """sample_pt_chain (pt.py:758-761): decided once per inter-swap run"""
        self.update = steps_taken > self.burnin

    def _add(self, Q, L):
        if self.count == 0:
            self.ops.group_moments_reset(self.state, self.n, Q, self.ref)
        self.ops.group_moments_update(self.state, Q, L[:, -1], self.ref)
        self.count += 1

    def after_step(self, Q, L, step):
        """the states after step number `step` (1-based count of the steps taken) enter the windows"""
        if self.G == 0:
            return
        self._add(Q, L)
        if self.count < self.buffer_size:
            return
        self.closed.append(step)
        if self.update:
            self.updates.append((step, self._relearn()))
        self.count = 0
        self._add(Q, L)   # keep_last

    def _relearn(self):
        _, cov, flags = self.ops.group_moments_factor(self.state, self.n, self.factors, want_cov=True)
        flags = flags.cpu().numpy().copy()
        for g in np.nonzero(flags == 2)[0]:
            try:
                F = np.linalg.cholesky(ensure_cov_psd(cov[g].cpu().numpy())).T
            except np.linalg.LinAlgError:
                continue
            if np.isfinite(F).all():
                self.factors[g].copy_(self.torch.from_numpy(np.ascontiguousarray(F)))
        if self.stepper.group_factors is None:
            self.stepper.set_group_proposals(self.factors)
            self.factors = self.stepper.group_factors
        return flags


def pt_sample(target, lower, upper, n_chains_posterior=1, n_chains_tempered=7, n_replicas=1,
              n_samples=1000, swap_interval=(100, 300), beta_tune_interval=10, proposal_cov=None,
              device=None, random_seed=17, tune_interval=100, record_every=1, update_proposal=False,
              buffer_size=5000, burnin=None, proposal_name="MultivariateNormal", start=None):
    """pt.py:793-906 driver.  Returns (posterior samples (n, nparams), their likelihood
    vectors, manager).  Samples of the beta == 1 replicas are recorded after every round.

    update_proposal: every temperature re-learns its multivariate proposal from its own window of ``buffer_size`` samples
    once ``burnin`` steps (None: int(n_samples * 0.1), pt.py:518) are over (``ProposalWindows``); the per-parameter
    families never update (base.py:368).  ``man.proposal_updates`` lists (step, flags of this rank's temperatures) per
    update, ``man.windows_closed`` the steps at which windows closed, ``man.proposal_factors`` the factors in use at the
    end (None before the first update).  proposal_name: the family of ``BatchedMetropolis.set_proposal`` (for a per-parameter
    family ``proposal_cov`` is the vector of scales, None: ones).  With several ranks every temperature's replicas must lie on one rank.

    start: (n_workers * n_replicas, nparams) start points of the replicas instead of the prior draws (a wrong length is the
    reference's TypeError, sampler/smc.py:429-436); the draws are still taken from the manager's stream.

    Exchange round: all-gather of ONE likelihood per replica, the swap sweep decided
    identically on every rank (shared RandomState), then the permutation is applied where the
    states live: local rows by a device gather, rows that change rank point to point
    (``parallel.exchange_rows``).  The replica states themselves are never gathered."""
    import torch
    start_points = start      # (`start` names this rank's first chain below)
    rank, world, _ = parallel.ensure_group()
    man = TemperingManager(n_chains_posterior, n_chains_tempered, n_replicas, swap_interval,
                           beta_tune_interval, random_seed)
    n_total = man.n_workers * n_replicas
    start, stop = parallel.chain_block(n_total, rank, world)
    adapt = bool(update_proposal) and proposal_name not in univariate_proposals
    if adapt and world > 1:
        # a temperature's window is accumulated where its replicas live, without a collective: every rank checks every
        # rank's block, so all of them raise together
        for r in range(world):
            if any(b % n_replicas for b in parallel.chain_block(n_total, r, world)):
                raise ValueError("update_proposal: the chains of rank %d, %s, cut a temperature of %d replicas in two; "
                                 "choose a rank count whose blocks end at temperature boundaries"
                                 % (r, parallel.chain_block(n_total, r, world), n_replicas))
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    stepper = BatchedMetropolis(target, lower, upper, stop - start, device=device,
                                tune_interval=tune_interval, seed=random_seed, first_chain=start)
    dev = stepper.device
    ops = stepper.ops
    if proposal_cov is None and proposal_name not in univariate_proposals:
        proposal_cov = np.diag(((upper - lower) * 0.05) ** 2)
    stepper.set_proposal(proposal_cov, proposal_name)
    Qall = lower + (upper - lower) * man.rng.random_sample((n_total, lower.size))
    if start_points is not None:
        from .smc import check_start
        Qall = check_start(start_points, n_total, lower.size)
    Q = upload(Qall[start:stop], dev)
    L = stepper.evaluate(Q).to(dev)
    npar = Q.shape[1]
    # posterior replicas (beta == 1) are the first n_posterior * n_replicas global chains
    n_post = man.n_workers_posterior * n_replicas
    p0, p1 = min(start, n_post), min(stop, n_post)
    samples, lsamples = [], []
    rounds = 0
    man.proposal_updates, man.windows_closed, man.proposal_factors = [], [], None
    windows = None
    if adapt:
        burnin = int(n_samples * 0.1) if burnin is None else int(burnin)
        windows = ProposalWindows(stepper, (stop - start) // n_replicas, npar, buffer_size, burnin, man.proposal_updates,
                                  man.windows_closed)
    # wall time and step count of the rounds alone (bench.py's pt_leg): man.loop_seconds / man.loop_steps
    if Q.is_cuda:
        torch.cuda.synchronize(dev)
    import time
    t_loop, man.loop_steps = time.perf_counter(), 0
    while sum(len(s) for s in samples) < n_samples:
        betas = torch.from_numpy(man.chain_betas[start:stop].copy()).to(dev)
        if windows is not None:
            windows.begin_round(man.loop_steps)
        for _ in range(man.draw_swap_interval()):
            stepper.step(Q, L, betas)
            man.loop_steps += 1
            if windows is not None:
                windows.after_step(Q, L, man.loop_steps)
        ops.check()
        QL = torch.cat([Q, L], 1)
        if rounds % record_every == 0:
            post = parallel.allgather_rows(QL[p0 - start:p1 - start]).cpu().numpy()
            samples.append(post[:, :npar].copy())
            lsamples.append(post[:, npar:].copy())
        like = parallel.allgather_rows(L[:, -1:].contiguous(), n_total)[:, 0].cpu().numpy()
        perm = man.swap_round(like)
        QL = parallel.exchange_rows(QL, perm, n_total, gather=ops.gather)
        Q, L = QL[:, :npar].contiguous(), QL[:, npar:].contiguous()
        rounds += 1
        if rounds % beta_tune_interval == 0 and man.n_workers_tempered > 0:
            man.tune_betas()
    if Q.is_cuda:
        torch.cuda.synchronize(dev)
    man.loop_seconds = time.perf_counter() - t_loop
    man.proposal_factors = stepper.group_factors
    return np.concatenate(samples)[:n_samples], np.concatenate(lsamples)[:n_samples], man
