"""
TEST INFRASTRUCTURE ONLY: the numpy restatement of the PT proposal adaptation of csrc/ptadapt.hip, one operation per
line and one row at a time -- the streaming likelihood-weighted moments of a group of chains and their finish -- and of
the window bookkeeping of the reference (beat/sampler/base.py:356-393, beat/sampler/pt.py:758-761).

State of a group (include/beat_amd.h): m, S0, Sw2, count, nbad, 3 spare | S1 [n] | S2 [n, n] lower triangle.
"""
import numpy as np

HDR = 8


def stride(n):
    return HDR + n + n * n


def new_state(G, n):
    st = np.zeros((G, stride(n)))
    st[:, 0] = -np.inf
    return st


def group_ref(Q, G):
    """mean of the rows of every group, summed in replica order"""
    X = np.asarray(Q, dtype=np.float64).reshape(G, -1, Q.shape[1])
    acc = np.zeros((G, X.shape[2]))
    for r in range(X.shape[1]):
        acc = acc + X[:, r]
    return acc / float(X.shape[1])


def update(st, Q, like, ref):
    """one update of every group with its R rows, in place: Q (G * R, n), like (G * R,), ref (G, n)"""
    G, n = ref.shape
    X = np.asarray(Q, dtype=np.float64).reshape(G, -1, n)
    lk = np.asarray(like, dtype=np.float64).reshape(G, -1)
    for g in range(G):
        ok = [bool(np.isfinite(lk[g, r]) and np.isfinite(X[g, r]).all()) for r in range(X.shape[1])]
        st[g, 4] += ok.count(False)
        if not any(ok):
            continue
        m_new = max(st[g, 0], max(lk[g, r] for r in range(len(ok)) if ok[r]))
        s = np.exp(st[g, 0] - m_new)
        S1 = st[g, HDR:HDR + n]
        S2 = st[g, HDR + n:].reshape(n, n)
        st[g, 0] = m_new
        st[g, 1] *= s
        st[g, 2] *= s * s
        S1 *= s
        S2 *= s
        for r in range(len(ok)):
            if not ok[r]:
                continue
            w = np.exp(lk[g, r] - m_new)
            y = X[g, r] - ref[g]
            st[g, 1] += w
            st[g, 2] += w * w
            st[g, 3] += 1
            S1 += w * y
            S2 += np.tril(np.outer(w * y, y))
    return st


def finish(st, n):
    """-> (cov (G, n, n) symmetric, flags (G,) with 1 where the moments are degenerate or not finite)"""
    G = st.shape[0]
    cov = np.zeros((G, n, n))
    flags = np.zeros(G, dtype=np.int32)
    for g in range(G):
        S0, Sw2 = st[g, 1], st[g, 2]
        S1 = st[g, HDR:HDR + n]
        L = np.tril(st[g, HDR + n:].reshape(n, n))
        S2 = L + np.tril(L, -1).T
        with np.errstate(all="ignore"):
            fact = 1.0 - Sw2 / (S0 * S0)
            mu = S1 / S0
            cov[g] = (S2 / S0 - np.outer(mu, mu)) / fact
        if not (fact > 0.0) or st[g, 4] > 0 or not np.isfinite(cov[g]).all() or not np.isfinite(st[g, :2]).all():
            flags[g] = 1
    return cov, flags


def factor(st, n, F):
    """the finish and the upper factors F_g^T F_g = cov_g into F (flagged groups untouched) -> (cov, flags)"""
    cov, flags = finish(st, n)
    for g in range(st.shape[0]):
        if flags[g]:
            continue
        try:
            F[g] = np.linalg.cholesky(cov[g]).T
        except np.linalg.LinAlgError:
            flags[g] = 2
    return cov, flags


def window_state(X, like, steps, R):
    """the state of ONE group after a window of steps x R samples in step-major order, ref = mean of the first step's rows"""
    n = X.shape[1]
    X3, l2 = X.reshape(steps, R, n), like.reshape(steps, R)
    ref = group_ref(X3[0], 1)
    st = new_state(1, n)
    for t in range(steps):
        update(st, X3[t], l2[t], ref)
    return st, ref


def cov_bound(X, like, ref):
    """the bound of the issue on |cov_ij| differences between two evaluations of one window of N_s samples:
    3 (N_s + 8) 2^-53 a_i a_j with a_i = sqrt(sum_s w_s y_si^2 / fact), w normalised, y = x - ref -- three sequentially
    rounded sums of N_s terms (S2, and S1 twice in mu mu^T) plus the exp and the divisions"""
    ok = np.isfinite(like) & np.isfinite(X).all(1)
    w = np.exp(like[ok] - like[ok].max())
    w = w / w.sum()
    y = X[ok] - ref
    fact = 1.0 - (w * w).sum()
    a = np.sqrt((w[:, None] * y * y).sum(0) / fact)
    return 3.0 * (X.shape[0] + 8) * 2.0 ** -53 * np.outer(a, a)


def window_closings(n_steps_per_round, buffer_size, burnin):
    """Plain restatement of one reference worker (base.py:356-393 under sample_pt_chain, pt.py:758-761, with keep_last):
    -> (steps at which the buffer filled, steps at which the proposal was updated), steps counted from 1"""
    closed, updated = [], []
    count, taken = 0, 0
    for n_steps in n_steps_per_round:
        update_proposal = taken > burnin          # step.cumulative_samples > step.burnin, once per call
        for _ in range(n_steps):
            taken += 1
            count += 1                            # trace.buffer_write
            if count == buffer_size:              # BufferError
                closed.append(taken)
                if update_proposal:
                    updated.append(taken)
                count = 0                         # record_buffer
                count += 1                        # keep_last: the last sample is put back
    return closed, updated
