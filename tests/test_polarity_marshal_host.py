"""How the polarity entries marshal their array arguments (beat_amd/polarity_binding.py: functions of a ``Context``),
pinned on the host with the stub library and the case language of tests/test_marshal_host.py: float32, Fortran-ordered or
strided inputs and Python lists arrive as the C-contiguous arrays the library reads."""
import inspect
import re

import numpy as np
import pytest

from beat_amd import engine
from beat_amd import polarity_binding as pb
from beat_amd.sources import BETA_MAPPING, U_MAPPING
from test_marshal_host import A, F, H, O, SAME, _Stub, f8, i8, run


@pytest.fixture
def ctx(monkeypatch):
    monkeypatch.setattr(pb, "ptr", lambda a: a)
    c = engine.Context.__new__(engine.Context)
    c._lib, c._h, c.device = _Stub(), H, 0
    for name in ("ffi_model_add_polarity", "mt6_batch", "polarity_amplitudes_batch", "w_to_beta_batch"):
        # (the harness calls methods of its context: bind the module's functions to this one object)
        monkeypatch.setattr(c, name, getattr(pb, name).__get__(c), raising=False)
    return c


OFF = [-1, -1, 0, 1, 2, -1]
FIX = F(6)


def test_add_polarity(ctx):
    rw, obs = F(6, 5), np.array([1, -1, 0, 1, 1], dtype=np.int16)
    run(ctx, "ffi_model_add_polarity", (3, "mtqt", OFF, FIX, [2, 3], rw, obs, 0.2, [4, -1], F(2)), {},
        "beatamd_ffi_model_add_polarity",
        [H, 3, 0, A(OFF, i8), A(FIX), 2, A([2, 3], i8), A(rw), A(obs, f8), 0.2, A([4, -1], i8), A(F(2)), 1000, A(U_MAPPING),
         A(BETA_MAPPING)])
    # kinds without tables hand none over; the caller's tables are taken as they are given
    run(ctx, "ffi_model_add_polarity", (3, "dc", OFF, FIX, [5], rw, obs, 0.1, [4], [0.0]), {}, "beatamd_ffi_model_add_polarity",
        [H, 3, 2, A(OFF, i8), A(FIX), 1, A([5], i8), A(rw), A(obs, f8), 0.1, A([4], i8), A([0.0]), 0, None, None])
    u, b = np.array([0.0, 1.0, 3.0], dtype=np.float32), [0.0, 0.5, 1.0]
    run(ctx, "ffi_model_add_polarity", (3, "mtqt", OFF, FIX, [5], rw, obs, 0.1, [4], [0.0]), {"tables": (u, b)},
        "beatamd_ffi_model_add_polarity",
        [H, 3, 0, A(OFF, i8), A(FIX), 1, A([5], i8), A(rw), A(obs, f8), 0.1, A([4], i8), A([0.0]), 3, A(u), A(b)])
    with pytest.raises(ValueError, match="rw"):
        ctx.ffi_model_add_polarity(3, "dc", OFF, FIX, [4], rw, obs, 0.1, [4], [0.0])


def test_population_entries(ctx):
    Q, rw = F(3, 4), F(6, 5)
    run(ctx, "mt6_batch", (Q, "mt", OFF, FIX), {}, "beatamd_mt6_batch", [H, 1, 3, 4, A(Q), A(OFF, i8), A(FIX), 0, None, None, O((3, 6))], 10)
    o = np.empty((3, 6))
    run(ctx, "mt6_batch", (Q, "mtqt", OFF, FIX), {"out": o}, "beatamd_mt6_batch",
        [H, 0, 3, 4, A(Q), A(OFF, i8), A(FIX), 1000, A(U_MAPPING), A(BETA_MAPPING), SAME(o)], 10)
    run(ctx, "polarity_amplitudes_batch", (Q, "dc", OFF, FIX, rw), {}, "beatamd_polarity_amplitudes_batch",
        [H, 2, 3, 4, A(Q), A(OFF, i8), A(FIX), 0, None, None, 5, A(rw), O((3, 5))], 12)
    with pytest.raises(ValueError, match="outside q"):
        ctx.mt6_batch(Q, "mt", [0, 1, 2, 3, 4, 5], FIX)
    with pytest.raises(ValueError, match="n_stations"):
        ctx.polarity_amplitudes_batch(Q, "dc", OFF, FIX, F(5, 6))


def test_w_to_beta(ctx):
    w = F(7)
    run(ctx, "w_to_beta_batch", (w,), {}, "beatamd_w_to_beta_batch", [H, 7, A(w), 1000, A(U_MAPPING), A(BETA_MAPPING), O((7,))], 6)
    w2 = F(2, 3)
    run(ctx, "w_to_beta_batch", (w2,), {}, "beatamd_w_to_beta_batch", [H, 6, A(w2), 1000, A(U_MAPPING), A(BETA_MAPPING), O((2, 3))], 6)


def test_every_polarity_entry_is_covered():
    """every function of the binding module that hands an array over is exercised above; Context itself gained no method"""
    handing = {name for name, fn in inspect.getmembers(pb, inspect.isfunction)
               if fn.__module__ == pb.__name__ and re.search(r"\bptr\(", inspect.getsource(fn))}
    assert handing == {"ffi_model_add_polarity", "mt6_batch", "polarity_amplitudes_batch", "w_to_beta_batch"}
    assert not any(hasattr(engine.Context, name) for name in handing)
