"""numpy restatement of the hyper model (csrc/hyper.hip): the terms of ``hyper_normal`` / the Laplacian's
``_eval_prior``, ``like`` in the device's fixed order, and a whole Metropolis chain on the Philox twin
(tests/philox_ref.py).  Test infrastructure: tests/test_hypers_host.py pins it to tests/golden/hypers.npz (numbers of
the reference's own functions), the GPU tests compare the kernels with it."""
import numpy as np

import philox_ref

LOG_2PI = np.log(2.0 * np.pi)


def terms(M, slog, kind, hp_index, H, llks):
    """H (C, nh), llks (C, nterm) -> (C, nterm); M, slog, kind, hp_index (nterm,)
    kind 0 (distributions.py:212-219)  -0.5 * (slog + (M * 2 * hp) + (1 / exp(hp * 2)) * llk)
    kind 1 (laplacian.py:92-96)        -0.5 * (-slog + (M * (LOG_2PI + 2 * hp)) + (1.0 / exp(hp * 2) * llk))"""
    M = np.asarray(M, dtype=np.int64)
    hp = np.asarray(H, dtype=np.float64)[:, np.asarray(hp_index)]
    llks = np.asarray(llks, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = (-0.5) * (slog + (M * 2 * hp) + (1 / np.exp(hp * 2)) * llks)
        lap = (-0.5) * (-slog + (M * (LOG_2PI + 2 * hp)) + (1.0 / np.exp(hp * 2) * llks))
    return np.where(np.asarray(kind) == 0, d, lap)


def like(T, group_end):
    """the device's order (hyper_like): per composite 64 strided partial sums (term k of the composite to partial
    k mod 64, ascending), a butterfly xor 32, 16, .. 1, then the composites added in order"""
    T = np.asarray(T, dtype=np.float64)
    total = np.zeros(T.shape[0])
    lanes = np.arange(64)
    k0 = 0
    with np.errstate(all="ignore"):
        for end in group_end:
            part = np.zeros((T.shape[0], 64))
            for k in range(k0, int(end)):
                part[:, (k - k0) % 64] += T[:, k]
            for off in (32, 16, 8, 4, 2, 1):
                part = part + part[:, lanes ^ off]
            total = total + part[:, 0]
            k0 = int(end)
    return total


def logp(M, slog, kind, hp_index, group_end, H, llks):
    """-> LL (C, nterm + 1): the terms, then like"""
    T = terms(M, slog, kind, hp_index, H, llks)
    return np.concatenate([T, like(T, group_end)[:, None]], axis=1)


def tune_factor(acc):
    """pymc's tune table as k_tune_scaling applies it (metropolis.py:294-306)"""
    f = np.ones_like(acc)
    for thr, fac in ((0.5, 1.1), (0.75, 2.0), (0.95, 10.0)):
        f = np.where(acc > thr, fac, f)
    for thr, fac in ((0.2, 0.9), (0.05, 0.5), (0.001, 0.1)):
        f = np.where(acc < thr, fac, f)
    return f


def recorded_steps(n_steps, buffer_thinning):
    """buffer[-1::-buffer_thinning] reversed, on the step numbers"""
    return list(range(n_steps))[-1::-buffer_thinning][::-1]


def chain(model, H, llks, lower, upper, kind, scales, seed, n_steps, scaling, step0=0, first_chain=0, tune_interval=0,
          steps_until_tune=None, accepted_since_tune=None, buffer_thinning=1):
    """metropolis.py:313-385 for C chains, n_steps steps, beta = 1, on the Philox streams of the device.
    model = (M, slog, kind, hp_index, group_end).  -> dict(H, LL, scaling, accepted_since_tune, n_accepted, trace
    (ndraws, C, nh + nterm + 1), inbox (n_steps, C), accepted (n_steps, C), steps_until_tune)"""
    H = np.array(H, dtype=np.float64)
    C, nh = H.shape
    LL = logp(*model, H, llks)
    scaling = np.array(np.broadcast_to(scaling, (C,)), dtype=np.float64)
    acc_since = np.zeros(C, dtype=np.int64) if accepted_since_tune is None else np.array(accepted_since_tune, dtype=np.int64)
    sut = tune_interval if steps_until_tune is None else int(steps_until_tune)
    rec = set(recorded_steps(n_steps, buffer_thinning))
    trace, inbox, accepted = [], np.zeros((n_steps, C), dtype=bool), np.zeros((n_steps, C), dtype=bool)
    for s in range(n_steps):
        if tune_interval > 0 and sut == 0:
            scaling = scaling * tune_factor(acc_since / float(tune_interval))
            acc_since[:] = 0
            sut = tune_interval
        step = (step0 + s) & 0xffffffff
        delta = philox_ref.univariate(C, nh, kind, scales, seed, step, first_chain)
        log_u = philox_ref.log_uniforms(C, seed, step, first_chain)
        Qp = H + (delta * scaling[:, None])
        inb = np.all((Qp >= lower) & (Qp <= upper), axis=1)
        Lp = logp(*model, np.where(inb[:, None], Qp, H), llks)
        with np.errstate(all="ignore"):
            mr = 1.0 * (Lp[:, -1] - LL[:, -1])
        acc = inb & np.isfinite(mr) & (log_u < mr)
        H[acc], LL[acc] = Qp[acc], Lp[acc]
        acc_since += acc
        inbox[s], accepted[s] = inb, acc
        sut -= 1
        if s in rec:
            trace.append(np.concatenate([H, LL], axis=1))
    return dict(H=H, LL=LL, scaling=scaling, accepted_since_tune=acc_since, n_accepted=int(accepted.sum()),
                trace=np.asarray(trace).reshape(len(trace), C, nh + LL.shape[1]), inbox=inbox, accepted=accepted,
                steps_until_tune=sut)


def chain_case(nh, seed=7):
    """inputs of the one-launch / step-by-step comparison: one term per hyper-parameter in two composites, M uniform in
    30..500, llk = M e^(2u) with u uniform in -1..3 (the mode of term k is h = u_k), box = mode +- 0.1
    -> (model, llk (nterm,), lower, upper)"""
    rng = np.random.default_rng(seed + nh)
    M = rng.integers(30, 501, nh)
    u = rng.uniform(-1.0, 3.0, nh)
    llk = M * np.exp(2.0 * u)
    mode = 0.5 * np.log(llk / M)
    slog = rng.uniform(-50.0, 50.0, nh)
    kind = (np.arange(nh) % 5 == 4).astype(np.int32)       # every fifth term takes the Laplacian's formula
    # (its mode is the same: d/dh [M 2h + e^(-2h) llk] = 0)
    group_end = [nh] if nh == 1 else [nh // 2, nh]
    return (M, slog, kind, np.arange(nh, dtype=np.int32), np.asarray(group_end, dtype=np.int32)), llk, mode - 0.1, mode + 0.1


def fixture_tables(g, tag):
    """tests/golden/hypers.npz, one of its two modes: (typs, names, H (sets, nh) with the named hyper-parameters side by side
    in name order, hp_index per dataset as the reference read it)"""
    typs = [str(t) for t in g["hn_typs"]]
    names = [str(n) for n in g["hn_names"]]
    sizes = [g["hn_%s_%s" % (tag, n)].shape[1] for n in names]
    off = dict(zip(names, np.concatenate([[0], np.cumsum(sizes)[:-1]])))
    H = np.concatenate([g["hn_%s_%s" % (tag, n)] for n in names], axis=1)
    hp_index = np.array([off["h_" + t] + i for t, i in zip(typs, g["hn_%s_index" % tag])])
    return typs, names, H, hp_index
