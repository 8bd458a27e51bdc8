"""
TEST INFRASTRUCTURE ONLY.

Writes tests/golden/pt_proposal.npz by running the REFERENCE's own calc_sample_covariance (beat/covariance.py:865-909: the
likelihood-weighted numpy.cov(..., aweights=, bias=False), then ensure_cov_psd) on seeded trace windows -- what a PT
worker learns its proposal from (beat/sampler/base.py:363-393, beat/backend.py:249-268).  Needs the reference tree
(oracle/ref_import.py finds it); the fixture is data (inputs and expected outputs, none of the reference's text).

    python tools/gen_golden_ptcov.py

calc_sample_covariance(buffer, lij, bij, beta) is called with two duck-typed arguments; it uses only lij.l2d,
lij.ordering["like"].list_ind and bij.map(point).data.

A window is `steps` x `replicas` samples in step-major order (sample s = step * replicas + replica): the order in which the
streaming update of csrc/ptadapt.hip sees them.  States: per replica a seeded random walk with steps of 0.1 from a start
within 0.1 of a mean of order 10.  Likes: -spread * u^4 for uniform u, i.e. spread over `spread` with about half of the
samples within 3 of the maximum (so that the weighted covariance keeps full rank).

  case   n   steps x replicas   spread
  n1      1   12 x 1             5
  n5      5   40 x 1             50
  n7      7   50 x 4             5
  n17    17   30 x 5             5
  n33    33    8 x 64            5
The generator asserts for each: a matrix comes back, ensure_cov_psd left it unchanged (it equals numpy.cov of the same
arguments), and lambda_min > 1e-8 lambda_max.

n1 is the exception: for one parameter numpy.cov returns a 0-d array, on which the reference's ensure_cov_psd raises
(numpy.linalg.cholesky and eigh refuse it), so calc_sample_covariance cannot be run.  Its expected value is the reference's
own numpy.cov call (covariance.py:889-898) restated here with the same arguments; the generator asserts that the
reference does raise, so the exception goes once the reference handles the case.

Degenerate windows, for which the reference returns None (stored as inputs only):
  spike   n 5, 20 x 2, one sample's like 800 above the rest
  single  n 5, one sample
"""
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import  # noqa: E402

ref_import.install()

from beat import covariance as rcov  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = (("n1", 1, 12, 1, 5.0), ("n5", 5, 40, 1, 50.0), ("n7", 7, 50, 4, 5.0), ("n17", 17, 30, 5, 5.0),
         ("n33", 33, 8, 64, 5.0))


class Lij(object):
    """list point = [x (n,), like (1,)]"""
    ordering = {"like": types.SimpleNamespace(list_ind=1)}

    def l2d(self, lpoint):
        return {"x": lpoint[0]}


class Bij(object):
    def map(self, point):
        return types.SimpleNamespace(data=point["x"])


def reference_cov(X, like):
    buffer = [([X[s], np.array([like[s]])], s) for s in range(X.shape[0])]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return rcov.calc_sample_covariance(buffer, Lij(), Bij(), beta=1.0)


def window(rng, n, steps, R, spread):
    mean = 10.0 + rng.standard_normal(n)
    x = mean + 0.1 * rng.standard_normal((R, n))
    X = np.empty((steps, R, n))
    for t in range(steps):
        x = x + 0.1 * rng.standard_normal((R, n))
        X[t] = x
    like = -spread * rng.uniform(size=steps * R) ** 4
    return X.reshape(steps * R, n), like


def main():
    rng = np.random.default_rng(20261019)
    out = {"note": np.array(
        "per case: X (steps * replicas, n) states in step-major order, like (steps * replicas,), shape = (steps, replicas), "
        "cov = beat.covariance.calc_sample_covariance(buffer, lij, bij, beta) of the window (n, n).  spike / single: "
        "windows for which the reference returns None (X, like, shape only)."),
        "cases": np.array([c[0] for c in CASES])}
    for name, n, steps, R, spread in CASES:
        X, like = window(rng, n, steps, R, spread)
        if n == 1:
            try:
                reference_cov(X, like)
            except np.linalg.LinAlgError:
                w = np.exp(like - like.max())
                cov = np.cov(X, aweights=w / np.sum(w), bias=False, rowvar=0)   # covariance.py:889-898
            else:
                raise AssertionError("the reference handles one parameter now: drop this branch")
        else:
            cov = reference_cov(X, like)
        assert cov is not None, name
        cov = np.atleast_2d(np.asarray(cov, dtype=np.float64))
        assert cov.shape == (n, n), (name, cov.shape)
        w = np.exp(like - like.max())
        plain = np.atleast_2d(np.cov(X, aweights=w / w.sum(), bias=False, rowvar=0))
        assert np.array_equal(cov, plain), name + ": ensure_cov_psd changed the matrix"
        lam = np.linalg.eigvalsh(cov)
        assert lam[0] > 1e-8 * lam[-1], (name, lam[0], lam[-1])
        out.update({name + "_X": X, name + "_like": like, name + "_shape": np.array([steps, R]), name + "_cov": cov})
        print("%-4s n = %2d  %3d x %2d samples  like range %.1f  lambda_min / lambda_max %.3g"
              % (name, n, steps, R, like.max() - like.min(), lam[0] / lam[-1]))
    X, like = window(rng, 5, 20, 2, 5.0)
    like[13] += 800.0
    assert reference_cov(X, like) is None
    out.update(spike_X=X, spike_like=like, spike_shape=np.array([20, 2]))
    X, like = window(rng, 5, 1, 1, 5.0)
    assert reference_cov(X, like) is None
    out.update(single_X=X, single_like=like, single_shape=np.array([1, 1]))
    print("spike, single: the reference returns None")
    path = os.path.join(GOLDEN, "pt_proposal.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f kB)" % (path, os.path.getsize(path) / 1e3))


if __name__ == "__main__":
    main()
