"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/hypers.npz by running the REFERENCE's own hyper-model arithmetic on seeded inputs.  Needs the
reference tree (oracle/ref_import.py finds it), so it runs where that tree is mounted; the fixture it writes is data
(inputs and expected outputs, none of the reference's text).

    python tools/gen_golden_hypers.py

Reference entry points exercised:
  beat/models/distributions.py:176-222   hyper_normal(datasets, hyperparams, llks, hp_specific)
  beat/models/laplacian.py:88-96         LaplacianDistributerComposite._eval_prior(hyperparam, exponent)
  beat/backend.py:100-118                thin_buffer(buffer, buffer_thinning, ensure_last=True)
  beat/models/base.py:352-373            the bounds arithmetic of estimate_hypers (floor(min) - 2, ceil(max) + 2, midpoint)

hyper_normal and _eval_prior are written against ``pytensor.tensor``; INSIDE THIS PROCESS ``distributions.tt`` /
``laplacian.tt`` are replaced by a small numpy namespace (``zeros``, ``exp``, ``set_subtensor`` writing through the
slice view), so the reference's own expressions produce the numbers as plain arrays.  estimate_hypers itself needs
a whole project; its three bound expressions are applied here to a seeded draw array that went through the
reference's ``get_values(burn, thin, combine)`` convention (burn and thin per chain, chains concatenated).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

ref_import.install()

from beat.models import distributions, laplacian  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _set_subtensor(view, value):
    view[...] = value
    return view.base if view.base is not None else view


NP_TT = SimpleNamespace(zeros=lambda n, dtype="float64": np.zeros(n, dtype=dtype), exp=np.exp,
                        set_subtensor=_set_subtensor)


def gen_hyper_normal(out, rng):
    typs = ["any_P_0_Z", "SAR", "any_P_0_Z", "GNSS", "SAR", "any_S_1_T", "any_P_0_Z", "SAR", "GNSS", "any_P_0_Z",
            "any_S_1_T", "SAR"]
    n = len(typs)
    samples = rng.integers(8, 5000, n)
    slog = rng.uniform(-4000.0, 4000.0, n)
    datasets = [SimpleNamespace(typ=t, samples=int(m), covariance=SimpleNamespace(slog_pdet=float(s)))
                for t, m, s in zip(typs, samples, slog)]
    names = sorted(set("h_" + t for t in typs))
    nsets = 12
    llks = 10.0 ** rng.uniform(-3.0, 7.0, (nsets, n))
    distributions.tt = NP_TT
    for tag, hp_specific in (("shared", False), ("specific", True)):
        sizes = {nm: (sum(1 for t in typs if "h_" + t == nm) if hp_specific else 1) for nm in names}
        H = {nm: rng.uniform(-20.0, 20.0, (nsets, sizes[nm])) for nm in names}
        exp = np.empty((nsets, n))
        for i in range(nsets):
            hyperparams = {nm: (H[nm][i] if hp_specific else H[nm][i, 0]) for nm in names}
            exp[i] = distributions.hyper_normal(datasets, hyperparams, llks[i], hp_specific=hp_specific)
        # which entry the reference read for dataset k: probe with one-hot sensitivity (the Counter order)
        index = np.empty(n, dtype=np.int64)
        for k in range(n):
            nm = "h_" + typs[k]
            base = {m_: np.zeros(sizes[m_]) if hp_specific else 0.0 for m_ in names}
            ref0 = distributions.hyper_normal(datasets, base, llks[0], hp_specific=hp_specific)[k]
            index[k] = 0
            if hp_specific:
                for j in range(sizes[nm]):
                    probe = {m_: np.zeros(sizes[m_]) for m_ in names}
                    probe[nm][j] = 1.0
                    if distributions.hyper_normal(datasets, probe, llks[0], hp_specific=True)[k] != ref0:
                        index[k] = j
        out["hn_%s_index" % tag] = index
        out["hn_%s_logpts" % tag] = exp
        for nm in names:
            out["hn_%s_%s" % (tag, nm)] = H[nm]
    out.update(hn_typs=np.array(typs), hn_names=np.array(names), hn_samples=samples.astype(np.int64), hn_slog=slog,
               hn_llks=llks)


def gen_laplacian(out, rng):
    laplacian.tt = NP_TT
    nsets = 12
    P = rng.integers(4, 3000, nsets)
    logdet = rng.uniform(-3000.0, 3000.0, nsets)
    h = rng.uniform(-20.0, 20.0, nsets)
    expo = 10.0 ** rng.uniform(-3.0, 7.0, nsets)
    val = np.empty(nsets)
    for i in range(nsets):
        fake = SimpleNamespace(sdet_shared_smoothing_op=float(logdet[i]), spatches=int(P[i]))
        val[i] = laplacian.LaplacianDistributerComposite._eval_prior(fake, float(h[i]), float(expo[i]))
    out.update(lap_P=P.astype(np.int64), lap_logdet=logdet, lap_h=h, lap_exponent=expo, lap_logpt=val)


def gen_thinning(out, rng):
    from beat.backend import thin_buffer
    cases = [(1, 1), (1, 3), (7, 1), (7, 2), (7, 3), (10, 5), (257, 3), (200, 7), (250, 2), (5, 9)]
    out["thin_cases"] = np.asarray(cases, dtype=np.int64)
    for n, t in cases:
        out["thin_%d_%d" % (n, t)] = np.asarray(thin_buffer(list(range(n)), t, ensure_last=True), dtype=np.int64)
    # the bounds of estimate_hypers on seeded draws: (ndraws, chains, size) per name
    n_steps, bt, burn, thin = 100, 3, 0.5, 2
    thinned_chain_length = len(thin_buffer(list(range(n_steps)), bt, ensure_last=True))
    res = []
    for i, size in enumerate((1, 4, 2)):
        draws = rng.normal(rng.uniform(-6, 6), rng.uniform(0.05, 1.5), (thinned_chain_length, 4, size))
        b = int(thinned_chain_length * burn)
        d = np.concatenate([draws[b::thin, c] for c in range(draws.shape[1])])      # get_values(combine=True)
        lower = np.floor(d.min()) - 2.0
        upper = np.ceil(d.max()) + 2.0
        res.append((lower, upper, (upper + lower) / 2.0))
        out["bounds_draws_%d" % i] = draws
    out.update(bounds_n_steps=np.array(n_steps), bounds_buffer_thinning=np.array(bt), bounds_burn=np.array(burn),
               bounds_thin=np.array(thin), bounds_expected=np.asarray(res), bounds_n=np.array(3))


def main():
    rng = np.random.default_rng(20261017)
    out = {"note": np.array(
        "hn_*: datasets of mixed typ (hn_typs, hn_samples, hn_slog), llks over ten decades, h in -20..20; hn_<tag>_logpts "
        "from the reference's hyper_normal with hp_specific off (shared) / on (specific), hn_<tag>_index the entry of the "
        "named hyper-parameter it read per dataset. lap_*: the reference's _eval_prior. thin_<n>_<t>: the reference's "
        "thin_buffer(list(range(n)), t). bounds_*: floor(min)-2 / ceil(max)+2 / midpoint of seeded draws after burn/thin.")}
    gen_hyper_normal(out, rng)
    gen_laplacian(out, rng)
    gen_thinning(out, rng)
    path = os.path.join(GOLDEN, "hypers.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f kB)" % (path, os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
