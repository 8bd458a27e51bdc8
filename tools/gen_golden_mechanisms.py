#!/usr/bin/env python
"""Writes tests/golden/mechanisms.npz: moment tensors at the edges of the per-draw arithmetic of csrc/mechanism.hpp and the
eigenvalues, standard decompositions and Hudson points of exactly those doubles, evaluated with mpmath at 50 digits from
the rules as the project states them (beat_amd/mechanisms.py) and rounded once to float64.  Data only.

    python tools/gen_golden_mechanisms.py
"""
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beat_amd.sources import dc_m6  # noqa: E402

mp.mp.dps = 50
IDX6 = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def mat(m6):
    a = mp.zeros(3, 3)
    for v, (i, j) in zip(m6, IDX6):
        a[i, j] = a[j, i] = mp.mpf(float(v))
    return a


def six(a):
    return [a[i, j] for i, j in IDX6]


def eig(a):
    """ascending eigenvalues and eigenvector columns; a diagonal matrix is its own answer"""
    if all(a[i, j] == 0 for i, j in ((0, 1), (0, 2), (1, 2))):
        order = sorted(range(3), key=lambda i: a[i, i])
        return [a[i, i] for i in order], [[mp.mpf(1 if r == i else 0) for r in range(3)] for i in order]
    E, Q = mp.eigsy(a)
    return [E[i] for i in range(3)], [[Q[r, i] for r in range(3)] for i in range(3)]


def decompose(m6):
    a = mat(m6)
    third = (a[0, 0] + a[1, 1] + a[2, 2]) / 3
    dev = a - third * mp.eye(3)
    e, v = eig(dev)
    order = sorted(range(3), key=lambda i: abs(e[i]))      # stable
    e, v = [e[i] for i in order], [v[i] for i in order]
    moment_iso, moment_dev = abs(third), abs(e[2])
    moment = moment_iso + moment_dev
    if moment_dev < mp.mpf(1e-6) * moment_iso:
        sdc = mp.mpf(0)
    else:
        sdc = e[2] * (1 + 2 * min(mp.mpf(0), e[0] / e[2]))
    dc = mp.zeros(3, 3)
    for i in range(3):
        for j in range(3):
            dc[i, j] = sdc * (v[2][i] * v[2][j] - v[1][i] * v[1][j])
    moments = [moment_iso, abs(sdc), moment_dev - abs(sdc), moment_dev, moment]
    ratios = [x / moment for x in moments[:4]] + [mp.mpf(1)]
    parts = [six(third * mp.eye(3)), six(dc), six(dev - dc), six(dev), six(a)]
    return moments, ratios, parts


def hudson(m6):
    e, _ = eig(mat(m6))
    m3, m2, m1 = e
    iso = (m1 + m2 + m3) / 3
    d1, d2, d3 = m1 - iso, m2 - iso, m3 - iso
    big = max(abs(d1), abs(d3))
    k = iso / (abs(iso) + big)
    t = 2 * d2 / big if big != 0 else mp.mpf(0)
    tau = t * (1 - abs(k))
    if tau * k <= 0:
        return e, (tau, k)
    if tau > 0:
        den = 1 - tau / 2 if tau < 4 * k else 1 - 2 * k
    else:
        den = 1 + tau / 2 if tau > 4 * k else 1 + 2 * k
    return e, (tau / den, k / den)


def rotated(diag, rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    a = q @ np.diag(diag) @ q.T
    a = 0.5 * (a + a.T)
    return [a[i, j] for i, j in IDX6]


def rows():
    rng = np.random.default_rng(20261020)
    out = []

    def add(label, m6):
        out.append((label, np.array(m6, dtype=np.float64)))

    for scale in (1e-20, 1.0, 1e20):
        for i in range(8):
            add("random scale %g" % scale, scale * rng.normal(size=6))
    for sdr in ((0.0, 90.0, 0.0), (30.0, 60.0, -90.0), (211.0, 17.0, 143.0), (95.0, 45.0, 90.0)):
        m = dc_m6(*sdr)
        add("dc exact %s" % (sdr,), m)
        add("dc perturbed 1e-9 %s" % (sdr,), m + 1e-9 * rng.normal(size=6))
    add("dc diagonal", [1.0, -1.0, 0.0, 0.0, 0.0, 0.0])
    add("dc off-diagonal", [0.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    for sign in (1.0, -1.0):
        add("clvd exact diagonal", sign * np.array([-1.0, -1.0, 2.0, 0.0, 0.0, 0.0]))
        r = np.array(rotated([-1.0, -1.0, 2.0], rng))
        add("clvd rotated", sign * r)
        add("clvd perturbed 1e-9", sign * (r + 1e-9 * rng.normal(size=6)))
    for iso in (1.0, -2.5):
        add("isotropic exact", [iso, iso, iso, 0.0, 0.0, 0.0])
        add("isotropic perturbed 1e-9", np.array([iso, iso, iso, 0.0, 0.0, 0.0]) + 1e-9 * rng.normal(size=6))
    add("two equal eigenvalues diagonal", [2.0, 5.0, 2.0, 0.0, 0.0, 0.0])
    add("two equal eigenvalues 1, 1, 3", [2.0, 2.0, 1.0, 1.0, 0.0, 0.0])
    add("two equal eigenvalues rotated", rotated([4.0, 4.0, -1.0], rng))
    for iso in (1.0, -1.0):
        for side in (-1.0, 1.0):
            a = 1e-6 * (1.0 + side * 1e-6)
            add("iso switch %+g side %+g diagonal" % (iso, side), [iso + a, iso, iso - a, 0.0, 0.0, 0.0])
            add("iso switch %+g side %+g off-diagonal" % (iso, side), [iso, iso, iso, a, 0.0, 0.0])
    add("diagonal", [3.0, -1.0, 0.5, 0.0, 0.0, 0.0])
    add("diagonal crack", [1.0, 1.0, 3.0, 0.0, 0.0, 0.0])
    add("diagonal lvd", [1.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    add("diagonal descending", [5.0, 1.0, -7.0, 0.0, 0.0, 0.0])
    return out


def main():
    data = rows()
    f = lambda seq: [float(x) for x in seq]      # noqa: E731  (one rounding to float64)
    m6, evals, moments, ratios, parts, uv = [], [], [], [], [], []
    for label, m in data:
        mo, ra, pa = decompose(m)
        e, (u, v) = hudson(m)
        m6.append(m)
        evals.append(f(e))
        moments.append(f(mo))
        ratios.append(f(ra))
        parts.append([f(p) for p in pa])
        uv.append([float(u), float(v)])
    path = os.path.join(ROOT, "tests", "golden", "mechanisms.npz")
    np.savez_compressed(path, labels=np.array([label for label, _ in data]), m6=np.array(m6), evals=np.array(evals),
                        moments=np.array(moments), ratios=np.array(ratios), parts=np.array(parts), uv=np.array(uv))
    print("%s: %d rows, %d bytes" % (path, len(data), os.path.getsize(path)))


if __name__ == "__main__":
    main()
