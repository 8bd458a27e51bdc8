"""
The convergence summary of a trace, computed on the device: what ``beat summarize`` writes to ``summary.txt`` --

  beat/apps/beat.py:1169-1334      the result trace: the kept draws of every chain, chain after chain, as ONE chain
  beat/backend.py:1401-1415        ``multitrace_to_inference_data``: one (chain, draw[, element]) array per variable
  beat/apps/beat.py:1338-1363      ``arviz.summary(idata, round_to=4, skipna=True)`` -> ``df.to_string``

with the columns ``mean sd hdi_3% hdi_97% mcse_mean mcse_sd ess_bulk ess_tail r_hat``, one row per scalar of every variable.
arviz is not a dependency: the statistics are RESTATED FROM MEMORY of arviz's ``stats/diagnostics.py`` and of Vehtari,
Gelman, Simpson, Carpenter & Buerkner (2021), unverified against an installed arviz (DESIGN.md 3.12b states them in full;
tests/convergence_ref.py is the numpy restatement the kernels are pinned to).

``X`` is a trace (C, D, V) -- C chains, D draws, V scalar variables --, or (D, V) for one chain; the single-variable
functions take (C, D) or (D,).  A numpy array gives numpy results; a torch-cuda tensor gives tensors on its device and the
trace never visits the host.  There is no CPU fallback: without a GPU the calls raise ``BeatAmdError``.

Formed on the host with numpy's expressions (from the small table, as the densities in ``beat_amd.marginals``):
``floor(hdi_prob S)`` (in the library, the same IEEE product and floor), ``mcse_mean = sd / sqrt(ess_mean)`` and
``mcse_sd = sd sqrt(e (1 - 1 / ess_sd)^(ess_sd - 1) - 1)``.

Deviations from arviz, all stated where they apply:
  * fewer than 4 draws give NaN diagnostics; ``mean``, ``sd`` and the interval are still filled;
  * a column holding a non-finite sample is flagged and all its entries are NaN (``skipna=True`` would skip the sample in
    ``mean``, ``sd`` and ``hdi``);
  * ``split`` takes the first and the last ``D // 2`` draws of every chain, first halves first (the statistics do not
    depend on the order of the rows).
"""
import os

import numpy as np

from . import diagnostics_binding as db
from ._marshal import is_dev, upload
from .engine import get_context

ESS_METHODS = ("bulk", "tail", "mean", "sd")


def hdi_names(hdi_prob=0.94):
    """arviz's names of the interval columns: ("hdi_3%", "hdi_97%") for 0.94"""
    lo = 100.0 * (1.0 - hdi_prob) / 2.0
    return "hdi_%g%%" % lo, "hdi_%g%%" % (100.0 - lo)


def mcse_columns(sd, ess_mean, ess_sd):
    """(mcse_mean, mcse_sd) from host columns, numpy's expressions"""
    sd, ess_mean, ess_sd = (np.asarray(a, dtype=np.float64) for a in (sd, ess_mean, ess_sd))
    with np.errstate(all="ignore"):
        fac = np.sqrt(np.exp(1) * (1 - 1 / ess_sd) ** (ess_sd - 1) - 1)
        return sd / np.sqrt(ess_mean), sd * fac


def _trace(X, single=False):
    """-> (ctx, device tensor (C, D, V), host?) of a trace given as (C, D, V) / (D, V) or, ``single``, (C, D) / (D,)"""
    shape = tuple(X.shape) if is_dev(X) else np.shape(X)
    want = (1, 2) if single else (2, 3)
    if len(shape) not in want or min(shape, default=0) < 1:
        raise ValueError("the trace must be %s with at least one entry a dimension, got %s"
                         % ("(chains, draws) or (draws,)" if single else "(chains, draws, variables) or (draws, variables)",
                            shape))
    if single:
        shape = shape + (1,)
    if len(shape) == 2:
        shape = (1,) + shape
    if is_dev(X):
        return get_context(X.device.index), X.contiguous().reshape(shape), False
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(shape)
    db.check_trace(X)
    ctx = get_context()      # (raises without the library or a GPU)
    return ctx, upload(X, "cuda:%d" % ctx.device), True


def _table(X, cols, hdi_prob, single=False, var_batch=None, first_lags=64):
    db.check_hdi_prob(hdi_prob), db.check_schedule(var_batch, first_lags)
    ctx, Xd, host = _trace(X, single)
    out, flags, rounds = db.convergence_summary(ctx, Xd, cols, hdi_prob, var_batch, first_lags)
    t = out.cpu().numpy()
    t[:, 4], t[:, 5] = mcse_columns(t[:, 1], t[:, 9], t[:, 10])
    return t, flags.cpu().numpy(), rounds, (None if host else Xd.device)


def _result(a, device):
    return a if device is None else upload(a, device)


def summary(X, var_names=None, hdi_prob=0.94, cols=None, var_batch=None, first_lags=64):
    """the table of ``arviz.summary`` as a dict of (K,) arrays under ``mean, sd, hdi_3%, hdi_97%, mcse_mean, mcse_sd, ess_bulk,
    ess_tail, r_hat`` (the interval names follow ``hdi_prob``), plus ``ess_mean`` and ``ess_sd``, ``flags`` (int32: 1 for a
    column with a non-finite sample, whose entries are all NaN) and ``names`` (``var_names`` or ``x0, x1, ...`` of the
    selected columns).  ``X``: (C, D, V), or (D, V) for one chain; ``cols``: the columns to summarise (None: all).

    ``var_batch`` (the variables of a pass over the workspace; None: sized to a budget) and ``first_lags`` (the lags of
    the first round of the on-demand autocovariance; the next rounds take four times as many for the scans that have not
    stopped) are the schedule: no bit of the table depends on them.  ``rounds`` in the result counts the rounds taken."""
    t, flags, rounds, device = _table(X, cols, hdi_prob, var_batch=var_batch, first_lags=first_lags)
    V = int((tuple(X.shape) if is_dev(X) else np.shape(X))[-1])
    c = db.check_columns(cols, V)
    if var_names is None:
        var_names = ["x%d" % i for i in range(V)]
    if len(var_names) != V:
        raise ValueError("var_names names %d variables, the trace has %d" % (len(var_names), V))
    lo, hi = hdi_names(hdi_prob)
    keys = ("mean", "sd", lo, hi, "mcse_mean", "mcse_sd", "ess_bulk", "ess_tail", "r_hat", "ess_mean", "ess_sd")
    table = dict((k, _result(np.ascontiguousarray(t[:, i]), device)) for i, k in enumerate(keys))
    table["flags"] = _result(flags, device)
    table["names"] = [var_names[int(i)] for i in c]
    table["rounds"] = rounds
    return table


def _one(X, column, hdi_prob=0.94):
    t, _, _, device = _table(X, None, hdi_prob, single=True)
    return t[0, column] if device is None else upload(t[0, column:column + 1], device)[0]


def ess(X, method="bulk"):
    """the effective sample size of one variable X (C, D) or (D,): ``method`` = "bulk" (rank-normalised split chains),
    "tail" (the smaller of the 5 % and 95 % indicator ESS), "mean" or "sd" (of the squared deviations)"""
    if method not in ESS_METHODS:
        raise ValueError("ess: unknown method %r (one of %s)" % (method, ", ".join(ESS_METHODS)))
    return _one(X, {"bulk": 6, "tail": 7, "mean": 9, "sd": 10}[method])


def rhat(X):
    """the rank-normalised split R-hat of one variable X (C, D) or (D,): the larger of the bulk and the folded value"""
    return _one(X, 8)


def mcse(X, method="mean"):
    """the Monte-Carlo standard error of the mean or of the standard deviation of one variable"""
    if method not in ("mean", "sd"):
        raise ValueError("mcse: unknown method %r ('mean' or 'sd')" % (method,))
    return _one(X, 4 if method == "mean" else 5)


def hdi(X, hdi_prob=0.94):
    """(lo, hi): the narrowest interval holding ``floor(hdi_prob S)`` + 1 of the S samples of one variable"""
    t, _, _, device = _table(X, None, hdi_prob, single=True)
    return t[0, 2:4].copy() if device is None else upload(t[0, 2:4], device)


def autocov(Y, nlags, lag0=0):
    """(R, nlags) (or (nlags,) for one row): the biased autocovariance ``(1/n) sum_i (y_i - m)(y_{i+k} - m)`` of every row of Y
    (R, n) at the lags ``lag0 <= k < lag0 + nlags`` -- what arviz's FFT route returns, summed here lag by lag in a fixed
    order; a lag >= n gives 0.  The value of a lag depends on no other argument."""
    one = len(tuple(Y.shape) if is_dev(Y) else np.shape(Y)) == 1
    db.check_lags(lag0, nlags)
    if is_dev(Y):
        ctx, Yd, host = get_context(Y.device.index), (Y.reshape(1, -1) if one else Y).contiguous(), False
        db.check_rows(Yd)
    else:
        Yh = db.check_rows(np.atleast_2d(np.asarray(Y, dtype=np.float64)))[0]
        ctx = get_context()
        Yd, host = upload(Yh, "cuda:%d" % ctx.device), True
    out = db.autocov_lags_batch(ctx, Yd, nlags, lag0)
    out = out[0] if one else out
    return out.cpu().numpy() if host else out


def rank_normalize(A, want_ranks=False):
    """z = Phi^-1((r - 3/8) / (A.size + 1/4)) with r = ``scipy.stats.rankdata(A.ravel(), "average")``, in A's shape (``-0.0``
    and ``0.0`` tie); ``want_ranks``: (z, r).  A non-finite value raises ``ValueError``."""
    if is_dev(A):
        ctx, Ad, host = get_context(A.device.index), A.contiguous(), False
    else:
        Ah = np.ascontiguousarray(A, dtype=np.float64)
        if Ah.size < 1:
            raise ValueError("rank_normalize: no values")
        ctx = get_context()
        Ad, host = upload(Ah, "cuda:%d" % ctx.device), True
    res = db.rank_normalize(ctx, Ad, want_ranks)
    if not host:
        return res
    return tuple(r.cpu().numpy() for r in res) if want_ranks else res.cpu().numpy()


# ------------------------------------------------------------------------------------------------ text
def row_names(var_names, sizes):
    """arviz's row names: ``var`` for a scalar variable, ``var[i]`` for the elements of a vector one"""
    return [n if s == 1 else "%s[%d]" % (n, i) for n, s in zip(var_names, sizes) for i in range(s)]


def summary_to_string(table, round_to=4):
    """the table as plain text, one row per name, the columns of ``arviz.summary`` right-aligned as ``DataFrame.to_string``
    lays them out; values rounded to ``round_to`` decimals (None: not rounded)"""
    keys = [k for k in table if k not in ("flags", "names", "rounds", "ess_mean", "ess_sd")]
    cols = [np.asarray(table[k].cpu().numpy() if is_dev(table[k]) else table[k], dtype=np.float64) for k in keys]
    if round_to is not None:
        cols = [np.round(c, round_to) for c in cols]
    cells = [[k] + ["%.*f" % (round_to, v) if round_to is not None else repr(float(v)) for v in c] for k, c in zip(keys, cols)]
    names = [""] + list(table["names"])
    widths = [max(len(s) for s in col) for col in cells]
    wn = max(len(s) for s in names)
    lines = []
    for r in range(len(names)):
        lines.append(names[r].ljust(wn) + "".join("  " + cells[c][r].rjust(widths[c]) for c in range(len(keys))))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ stages
def read_stage(stage_dir, layout, out_names, backend="bin"):
    """the chains of a stage directory -> (values (n_chains, n_draws, V), row names): the variables in file order (the free
    variables in layout order, then the likelihood block), flattened, every chain file ``chain-<k>`` with k >= 0"""
    from .backend import backend_catalog, population_shapes
    shapes, _ = population_shapes(layout, out_names)
    ext = {"bin": ".bin", "csv": ".csv"}[backend]
    ids = sorted(int(f[len("chain-"):-len(ext)]) for f in os.listdir(stage_dir)
                 if f.startswith("chain-") and f.endswith(ext) and f[len("chain-"):-len(ext)].lstrip("-").isdigit())
    ids = [i for i in ids if i >= 0]
    if not ids:
        raise ValueError("%s holds no chain files (chain-<k>%s)" % (stage_dir, ext))
    chains = []
    for i in ids:
        ch = backend_catalog[backend](stage_dir, shapes)
        ch.setup(0, i, overwrite=False)
        vals = [np.asarray(ch.get_values(v), dtype=np.float64) for v in shapes]
        chains.append(np.concatenate([v.reshape(v.shape[0], -1) for v in vals], axis=1))
    n = set(c.shape[0] for c in chains)
    if len(n) != 1:
        raise ValueError("%s: the chains hold different numbers of draws (%s)" % (stage_dir, sorted(n)))
    sizes = [int(np.prod(s, dtype=np.int64)) for s in shapes.values()]
    return np.stack(chains), row_names(list(shapes), sizes)


def summarize_stage(stage_dir, layout, out_names, sampler="SMC", final=True, burn=0.0, thin=1, per_chain=False, hdi_prob=0.94,
                    backend="bin", summary_file=None, round_to=4):
    """``summary.txt`` of a stage directory -> (table, text).  The draws are arranged as ``beat summarize`` collects its result
    trace (apps/beat.py:1169-1334): for "SMC" all kept draws of every chain (``final``) or the last one (an intermediate
    stage), for "Metropolis" the kept draws ``[int(floor(n burn))::thin]`` of every chain, for "PT" those of chain 0 -- chain
    after chain as ONE chain of n_chains x len(idxs) draws (backend.py:1401-1415).  ``per_chain=True`` keeps the chains
    apart instead, so that R-hat compares them.  The text goes to ``summary_file`` (default: ``summary.txt`` beside the
    stage directory; False: not written)."""
    if sampler not in ("SMC", "PT", "Metropolis"):
        raise NotImplementedError("Summarize function still needs to be implemented for %s sampler" % sampler)
    vals, names = read_stage(stage_dir, layout, out_names, backend)
    n = vals.shape[1]
    if sampler == "SMC":
        idxs = np.arange(n) if final else np.array([n - 1])
    else:
        idxs = np.arange(n)[int(np.floor(n * burn))::max(1, int(thin))]
    if sampler == "PT":
        vals = vals[:1]
    vals = vals[:, idxs]
    if not per_chain:
        vals = vals.reshape(1, -1, vals.shape[2])
    table = summary(vals, var_names=names, hdi_prob=hdi_prob)
    text = summary_to_string(table, round_to)
    if summary_file is None:
        summary_file = os.path.join(os.path.dirname(os.path.abspath(stage_dir)), "summary.txt")
    if summary_file:
        with open(summary_file, "w") as fh:
            fh.write(text)
    return table, text
