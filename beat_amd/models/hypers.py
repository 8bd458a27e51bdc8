"""
Sampling the hyper-parameters alone -- the counterpart of ``beat sample --hypers``:

  beat/models/problems.py:261-297     Problem.built_hyper_model (like = sum of the composites' hyper formulas)
  beat/sampler/base.py:398-418        init_chain_hypers: a random source point per chain, update_llks
  beat/models/distributions.py:176-222  hyper_normal (through Composite.get_hyper_formula, models/base.py:110-123)
  beat/models/laplacian.py:88-96, 156-170  _eval_prior / get_hyper_formula (one term per slip variable)
  beat/models/base.py:304-379         estimate_hypers: the run and the new bounds

The source is fixed at one point per chain, every dataset's whitened misfit |W r|^2 is cached once
(``LogpForwFunc.update_llks``), Metropolis then runs on the noise scalings ``h_*`` alone and
``floor(min) - 2 ... ceil(max) + 2`` of the draws become the bounds of the main sampler.

``HyperModel`` is a *target* in the samplers' sense (``nparams``, ``nllk``, ``out_names``, ``batch``,
``astep_batch``, ``mstep_batch``) whose evaluation is one small kernel (``k_hyper_logp``); since nothing but a few hundred flops is
left of a step, ``chain_batch`` runs a whole chain of steps in ONE launch (``k_hyper_chain``) -- bit for bit the
step-by-step path.  There is no CPU fallback.
"""
import os
from collections import OrderedDict

import numpy as np

from .. import parallel
from .._marshal import upload
from .distributions import _Counter, get_hyper_name
from .problem import ParameterLayout, hyper_name_laplacian

KIND_DATASET, KIND_LAPLACIAN = 0, 1
CHAIN_MAX = 1024      # hyper-parameters / terms a chain of beatamd_hyper_chain_batch holds, each


def dataset_hypers(datasets, hp_specific=False):
    """(hyper-parameter name, index) per dataset as ``hyper_normal`` / ``multivariate_normal_chol`` read them
    (distributions.py:24-25, 117-126, 195-210): "h_" + dataset.typ, and with ``hp_specific`` the running count of
    that name (beat.utility.Counter), else 0"""
    count = _Counter()
    out = []
    for d in datasets:
        name = get_hyper_name(d)
        out.append((name, count(name) if hp_specific else 0))
    return out


def thinned_length(n_steps, buffer_thinning):
    """len(thin_buffer(list(range(n_steps)), buffer_thinning, ensure_last=True)) (beat/backend.py:100-118)"""
    return len(range(int(n_steps) - 1, -1, -max(1, int(buffer_thinning))))


def kept_draws(draws, burn=0.5, thin=2):
    """what ``mtrace.get_values(v, burn=int(thinned_chain_length * burn), thin=thin)`` keeps of every chain
    (models/base.py:352-363): draws (ndraws, chains, ...) along the first axis, numpy array or tensor; ``burn`` is a
    fraction of the THINNED chain length (the number of recorded draws)"""
    return draws[int(draws.shape[0] * burn)::int(thin)]


def bounds_of_extrema(dmin, dmax):
    """models/base.py:365-373: lower = floor(d.min()) - 2, upper = ceil(d.max()) + 2, testvalue their midpoint"""
    lower = np.floor(float(dmin)) - 2.0
    upper = np.ceil(float(dmax)) + 2.0
    return float(lower), float(upper), float((upper + lower) / 2.0)


def hyper_bounds(draws, burn=0.5, thin=2):
    """models/base.py:352-373 for one hyper-parameter name: draws (ndraws, chains, size) -> (lower, upper, testvalue);
    burn and thin are taken per chain and the chains combined.  ``estimate_hypers`` runs these two functions (the
    extrema of the kept draws all-gathered over the ranks in between)"""
    d = kept_draws(np.asarray(draws), burn, thin)
    return bounds_of_extrema(d.min(), d.max())


class HyperModel(object):
    """The hyper model of a compiled problem ``f`` (``FFIProblem.compile`` / ``GeodeticGeometryProblem.compile``), or of
    the problem description alone (tables only; the device side needs ``f`` or ``ctx``).

    Terms, in ``update_llks`` column order: every seismic dataset (wavemap by wavemap), every geodetic dataset, one
    term per slip variable of the Laplacian on ``h_laplacian``.  The hyper-parameter vector is the ``h_*`` slice of
    the problem's layout, in layout order.

    ``slog_pdet`` of every dataset is read from the problem description WHEN THE MODEL IS BUILT.
    ``LogpForwFunc.update_weights`` keeps the wavemaps' description in step with the device, so build the hyper model
    after the last weight update (a geodetic weight set changed behind the description is not seen).  A stale
    ``slog`` shifts a dataset's term by a constant: the draws and the bounds do not move, the recorded ``*_like``
    columns do."""

    def __init__(self, f, ctx=None):
        prob = getattr(f, "problem", f)
        from .problem import refuse_polarity
        refuse_polarity(prob, "estimate_hypers / HyperModel")
        self.f = f if prob is not f else None
        self.problem = prob
        self.ctx = ctx if ctx is not None else getattr(f, "ctx", None)
        full = prob.layout
        self.layout = ParameterLayout(OrderedDict((k, n) for k, n in full.varsizes.items() if k.startswith("h_")))
        if self.layout.size == 0:
            raise ValueError("the problem has no hyper-parameters (h_*) in its parameter vector")
        self.names = list(self.layout.varsizes)
        self.nparams = self.nh = self.layout.size
        # position of every hyper-parameter inside the problem's parameter vector
        self.full_index = np.concatenate([full.offsets[k] + np.arange(n) for k, n in self.layout.varsizes.items()])
        M, slog, kind, hp, names, ends = [], [], [], [], [], []
        for wm in prob.wavemaps:
            for t, (name, i) in enumerate(wm.hypers):
                M.append(getattr(wm, "nsamples", wm.data.shape[1])); slog.append(float(wm.slog_pdet[t])); kind.append(KIND_DATASET)
                hp.append(self.layout.offset(name, i))
                names.append("seis_like_%s_%d" % (wm.name, t))
        if prob.wavemaps:
            ends.append(len(M))
        g = prob.geodetic
        if g is not None:
            for d, (name, i) in enumerate(g.hypers):
                M.append(g.sizes[d]); slog.append(float(g.slog_pdets[d])); kind.append(KIND_DATASET)
                hp.append(self.layout.offset(name, i))
                names.append("geo_like_%d" % d)
            ends.append(len(M))
        if prob.laplacian is not None:
            L, logdet = prob.laplacian
            for v in prob.slip_varnames:
                M.append(np.shape(L)[0]); slog.append(float(logdet)); kind.append(KIND_LAPLACIAN)
                hp.append(self.layout.offset(hyper_name_laplacian, 0))
                names.append("laplacian_like_%s" % v)
            ends.append(len(M))
        self.M = np.asarray(M, dtype=np.int64)
        self.slog = np.asarray(slog, dtype=np.float64)
        self.kind = np.asarray(kind, dtype=np.int32)
        self.hp_index = np.asarray(hp, dtype=np.int32)
        self.group_end = np.asarray(ends, dtype=np.int32)
        self.nterm = int(self.M.size)
        self.nllk = self.nterm + 1
        self.out_names = names + ["like"]
        lo, up = full.bounds(prob.lower, prob.upper) if prob.lower is not None else (None, None)
        self.full_lower, self.full_upper = lo, up
        self.lower = None if lo is None else lo[self.full_index]
        self.upper = None if up is None else up[self.full_index]
        self._id = None
        self.llks = None

    @classmethod
    def from_tables(cls, nh, M, slog, kind, hp_index, group_end, lower=None, upper=None, ctx=None, out_names=None):
        """a hyper model from its term tables alone (term k: formula kind[k] on hyper-parameter hp_index[k] with M[k],
        slog[k]; group_end: exclusive ends of the composites); the hyper-parameters are one variable "h" of size nh"""
        self = cls.__new__(cls)
        self.f, self.problem, self.ctx = None, None, ctx
        self.layout = ParameterLayout(OrderedDict([("h", int(nh))]))
        self.names = ["h"]
        self.nparams = self.nh = int(nh)
        self.full_index = np.arange(self.nh)
        self.M = np.asarray(M, dtype=np.int64)
        self.slog = np.asarray(slog, dtype=np.float64)
        self.kind = np.asarray(kind, dtype=np.int32)
        self.hp_index = np.asarray(hp_index, dtype=np.int32)
        self.group_end = np.asarray(group_end, dtype=np.int32)
        self.nterm = int(self.M.size)
        self.nllk = self.nterm + 1
        self.out_names = list(out_names) if out_names is not None else ["geo_like_%d" % k for k in range(self.nterm)] + ["like"]
        self.lower = None if lower is None else np.asarray(lower, dtype=np.float64)
        self.upper = None if upper is None else np.asarray(upper, dtype=np.float64)
        self.full_lower, self.full_upper = self.lower, self.upper
        self._id, self.llks = None, None
        return self

    # -- device side
    def _device_id(self):
        if self._id is None:
            if self.ctx is None:
                from ..engine import get_context
                self.ctx = get_context()       # raises without the library or a GPU: there is no CPU fallback
            self._id = self.ctx.hyper_model_create(self.nh, self.M, self.slog, self.kind, self.hp_index, self.group_end)
        return self._id

    def release(self):
        if self._id is not None:
            self.ctx.hyper_model_destroy(self._id)
            self._id = None

    def set_llks(self, llks):
        """the cached misfits (C, nterm) the following evaluations condition on (``update_llks`` of the compiled model)"""
        if llks.shape[-1] != self.nterm:
            raise ValueError("expected %d misfit columns, got %d" % (self.nterm, llks.shape[-1]))
        self.llks = llks

    def _llks_for(self, H):
        if self.llks is None:
            raise RuntimeError("no cached misfits: call set_llks(f.update_llks(Q)) first")
        if self.llks.shape[0] != H.shape[0]:
            raise ValueError("%d chains, cached misfits of %d" % (H.shape[0], self.llks.shape[0]))
        return self.llks

    def batch(self, H, out=None):
        """H (C, nh) -> LL (C, nterm + 1): the terms, then like.  numpy or torch-cuda, like the cached misfits"""
        return self.ctx_or_raise().hyper_logp_batch(self._device_id(), H, self._llks_for(H), out)

    def ctx_or_raise(self):
        self._device_id()
        return self.ctx

    def astep_batch(self, Q0, L0, delta, scaling, lower, upper, log_u, beta, accepted=None):
        """metropolis.py:313-385 for all chains, in place on Q0 / L0 (device tensors), out of entries that exist with
        k_hyper_logp in the middle: propose (out-of-box rows parked), evaluate, accept (reads like from the last column)"""
        import torch
        ctx = self.ctx_or_raise()
        C = Q0.shape[0]
        if getattr(self, "_qprop", None) is None or self._qprop.shape != Q0.shape or self._qprop.device != Q0.device:
            self._qprop = torch.empty_like(Q0)
            self._inb = torch.empty(C, dtype=torch.int32, device=Q0.device)
            self._lprop = torch.empty((C, self.nllk), dtype=torch.float64, device=Q0.device)
        if accepted is None:
            accepted = torch.zeros(C, dtype=torch.int32, device=Q0.device)
        ctx.metropolis_propose(Q0, delta, scaling, lower, upper, self._qprop, self._inb)
        ctx.hyper_logp_batch(self._device_id(), self._qprop, self._llks_for(Q0), self._lprop)
        ctx.metropolis_accept(Q0, L0, self._qprop, self._lprop, self._inb, log_u, beta, accepted)
        return accepted

    def mstep_batch(self, Q0, L0, factor, kind, df, seed, step, first_chain, scaling, lower, upper, beta, accepted,
                    accepted_sum=None, n_accepted=None):
        """one Metropolis step with the proposal drawn on the device (the call signature of ``LogpForwFunc.mstep_batch``):
        ``beatamd_proposal_draw[_univariate]`` then ``astep_batch``; the counters follow on the device"""
        ctx = self.ctx_or_raise()
        C = Q0.shape[0]
        if kind is None:
            delta, log_u = ctx.proposal_draw(factor, C, seed, step, first_chain=first_chain, df=df)
        else:
            delta, log_u = ctx.proposal_draw_univariate(kind, factor, C, seed, step, first_chain=first_chain)
        self.astep_batch(Q0, L0, delta, scaling, lower, upper, log_u, beta, accepted)
        if accepted_sum is not None:
            accepted_sum += accepted
        if n_accepted is not None:
            n_accepted += accepted.sum()
        return accepted

    def chain_applicable(self):
        """what a chain's wavefront of k_hyper_chain holds; beyond it the step-by-step path is taken"""
        return self.nh <= CHAIN_MAX and self.nterm <= CHAIN_MAX

    def chain_batch(self, H, LL, n_steps, scaling, accepted_since_tune, lower, upper, kind, scales, seed, step0,
                    first_chain, tune_interval, steps_until_tune, buffer_thinning=1, trace=None, n_accepted=None):
        """``n_steps`` Metropolis steps (beta = 1) of every chain in one launch, in place on H, LL, scaling,
        accepted_since_tune (device tensors); trace (ndraws, C, nh + nterm + 1) or None.  The kernel gets raw
        pointers: shapes and types are checked here"""
        import torch
        ctx = self.ctx_or_raise()
        C, n_steps, bt = int(H.shape[0]), int(n_steps), int(buffer_thinning)
        if n_steps < 0 or bt < 1:
            raise ValueError("chain_batch: n_steps >= 0 and buffer_thinning >= 1")

        def need(what, t, shape, dtype):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError("chain_batch: %s must be a contiguous %s device tensor of shape %s, got %s"
                                 % (what, str(dtype).replace("torch.", ""), shape,
                                    (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t)))
        need("H", H, (C, self.nh), torch.float64)
        need("LL", LL, (C, self.nllk), torch.float64)
        need("scaling", scaling, (C,), torch.float64)
        need("accepted_since_tune", accepted_since_tune, (C,), torch.int32)
        for what, t in (("lower", lower), ("upper", upper), ("scales", scales)):
            need(what, t, (self.nh,), torch.float64)
        need("the cached misfits", self._llks_for(H), (C, self.nterm), torch.float64)
        if trace is not None:
            need("trace", trace, (thinned_length(n_steps, bt), C, self.nh + self.nllk), torch.float64)
        if n_accepted is not None:
            need("n_accepted", n_accepted, (), torch.int64)
        ctx.hyper_chain_batch(self._device_id(), n_steps, H, LL, scaling, accepted_since_tune, self._llks_for(H), lower,
                              upper, kind, scales, seed, step0, first_chain, tune_interval, steps_until_tune, bt, trace,
                              n_accepted)


def estimate_hypers(f, hyper_model=None, n_chains=20, n_steps=25000, tune_interval=50, burn=0.5, thin=2,
                    buffer_thinning=1, proposal_name="Normal", random_seed=20, homepath=None, backend="bin",
                    use_chain_batch=True):
    """models/base.py:304-379 on the device (defaults: config.py:1698-1712, 1771-1791 -- Metropolis, ``Normal``
    proposal with unit scales, 20 chains x 25 000 steps, tune_interval 50, burn 0.5, thin 2).

    f: compiled model (``update_llks``).  ``n_chains`` source points are drawn uniformly in the problem's box and the
    start points of ``h`` in theirs, from ``RandomState(random_seed)`` (identical on every rank; chain 0 starts at the
    test point, the middle of the box, metropolis.py:152); the misfits are cached once; the chains of this rank
    (``parallel.chain_block``) run in one launch, every ``buffer_thinning``-th draw recorded by the reference's rule.
    -> ({name: (lower, upper, testvalue)}, trace (ndraws, local chains, nh + nterm + 1) device tensor).
    With ``homepath`` the draws are written to ``homepath/hypers/stage_1`` in the reference's chain-file format.
    ``use_chain_batch=False`` takes the step-by-step path (same numbers).  ``update_covariances`` inside
    init_chain_hypers and writing a config file are not part of this."""
    import torch

    from ..backend import write_population
    from ..sampler.metropolis import BatchedMetropolis
    from ..sampler.ops import collective_check
    hm = hyper_model if hyper_model is not None else HyperModel(f)
    ctx = hm.ctx_or_raise()
    dev = torch.device("cuda", ctx.device)
    if hm.lower is None:
        raise ValueError("the problem carries no bounds (lower / upper)")
    rank, world, _ = parallel.ensure_group()
    rs = np.random.RandomState(random_seed)
    lo, up = hm.full_lower, hm.full_upper
    Q = lo + (up - lo) * rs.random_sample((int(n_chains), lo.size))
    H = hm.lower + (hm.upper - hm.lower) * rs.random_sample((int(n_chains), hm.nh))
    H[0] = (hm.upper + hm.lower) / 2.0
    a, b = parallel.chain_block(n_chains, rank, world)
    Qd = upload(Q[a:b], dev)
    Hd = upload(H[a:b], dev)
    llks = f.update_llks(Qd)
    # a source point outside the library grid raises here, like the reference's IndexError -- on EVERY rank, whichever
    # owns the chain (a rank raising alone would leave the others waiting in the next collective)
    collective_check(ctx, world)
    bad = torch.tensor([[0.0 if bool(torch.isfinite(llks).all()) else 1.0]], dtype=torch.float64, device=dev)
    if float(parallel.allgather_rows(bad).sum()) > 0.0:
        raise ValueError("Got NaN in the cached misfits! Source point outside the library grid?")
    hm.set_llks(llks)
    step = BatchedMetropolis(hm, hm.lower, hm.upper, b - a, device=dev, tune=tune_interval > 0,
                             tune_interval=max(1, int(tune_interval)), scale=1.0, seed=random_seed, first_chain=a)
    step.set_proposal(None, proposal_name)
    L = step.evaluate(Hd)
    ndraws = thinned_length(n_steps, buffer_thinning)
    trace = torch.empty((ndraws, b - a, hm.nh + hm.nllk), dtype=torch.float64, device=dev)
    n_acc = torch.zeros((), dtype=torch.int64, device=dev)
    step.use_chain_batch = bool(use_chain_batch)
    step.run(Hd, L, 1.0, n_steps, n_acc, trace=trace, buffer_thinning=buffer_thinning)
    ctx.synchronize()
    kept = kept_draws(trace[:, :, :hm.nh], burn, thin)
    # per NAME over all entries of the variable, all chains of all ranks: the extrema travel, not the draws
    ext = torch.empty((1, 2 * len(hm.names)), dtype=torch.float64, device=dev)
    for i, name in enumerate(hm.names):
        o, n = hm.layout.offsets[name], hm.layout.varsizes[name]
        ext[0, 2 * i] = kept[:, :, o:o + n].min()
        ext[0, 2 * i + 1] = kept[:, :, o:o + n].max()
    ext = parallel.allgather_rows(ext).cpu().numpy()
    bounds = OrderedDict((name, bounds_of_extrema(ext[:, 2 * i].min(), ext[:, 2 * i + 1].max()))
                         for i, name in enumerate(hm.names))
    if homepath is not None:
        tr = trace.cpu().numpy()
        write_population(os.path.join(homepath, "hypers"), 1, hm.layout, hm.out_names, tr[:, :, :hm.nh], tr[:, :, hm.nh:], backend, first_chain=a)
    return bounds, trace
