"""Validate the C restatement against the REFERENCE's own C extension: its outputs on 150 random grids are stored in
tests/golden/sweep_random.npz (oracle/gen_golden.py), and where the extension itself was compiled in place (oracle/_ref,
built by oracle/Makefile from the reference's beat/fast_sweeping/fast_sweep_ext.c) it is run on the same grids too."""
import glob
import importlib.util
import os

import numpy as np

from oracle import oracle as orc

_REF = os.path.join(os.path.dirname(os.path.abspath(orc.__file__)), "_ref")


def _load_ref():
    so = glob.glob(os.path.join(_REF, "fast_sweep_ext*.so"))
    if not so:
        return None
    spec = importlib.util.spec_from_file_location("fast_sweep_ext", so[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sweep_bit_exact_random_grids(golden):
    ref = _load_ref()
    g = golden("sweep_random")
    rng = np.random.default_rng(42)
    at = 0
    for psz, hd, hs, nd, ns in g["meta"]:
        hd, hs, nd, ns = int(hd), int(hs), int(nd), int(ns)
        # (the grids are the seeded draws the fixture was made from)
        assert (nd, ns) == (int(rng.integers(2, 21)), int(rng.integers(2, 21)))
        slow = 1.0 / rng.uniform(0.5, 6.0, nd * ns)
        assert psz == float(rng.uniform(0.5, 3.0))
        assert (hd, hs) == (int(rng.integers(0, nd)), int(rng.integers(0, ns)))
        assert np.array_equal(slow, g["slow"][at:at + nd * ns])
        a = g["times"][at:at + nd * ns]
        at += nd * ns
        b = orc.fast_sweep(slow, psz, hd, hs, nd, ns)
        assert np.array_equal(a, b)
        if ref is not None:
            assert np.array_equal(ref.fast_sweep(slow, psz, hd, hs, nd, ns), b)
    assert len(g["meta"]) == 150 and at == g["slow"].size == g["times"].size
