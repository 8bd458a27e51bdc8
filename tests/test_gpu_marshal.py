"""
The device branches of ``beat_amd._marshal`` on (3, 4) tensors, and three calls with arguments on both sides against the
same calls made all-host, bit for bit (tests/test_marshal_host.py pins the host branches without a GPU).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_momentrate import CASES, _Model  # noqa: E402

from beat_amd import _marshal as m  # noqa: E402

pytestmark = pytest.mark.gpu

f8, i4, i8 = np.float64, np.int32, np.int64
HOST = (np.arange(12, dtype=f8) * 0.5 - 2).reshape(3, 4)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    import beat_amd
    return beat_amd.get_context(0)


@pytest.fixture(scope="module")
def dev(ctx):
    return "cuda:%d" % ctx.device


def test_upload_keeps_or_forces_the_dtype(torch, dev):
    for dt, tdt in ((f8, torch.float64), (np.float32, torch.float32), (i4, torch.int32), (i8, torch.int64)):
        src = np.asfortranarray(HOST.astype(dt))
        t = m.upload(src, dev)
        assert t.is_cuda and t.dtype == tdt and t.is_contiguous() and np.array_equal(t.cpu().numpy(), src)
        t = m.upload(src, dev, f8)
        assert t.is_cuda and t.dtype == torch.float64 and np.array_equal(t.cpu().numpy(), src.astype(f8))
    t = m.upload(HOST[:, ::2], torch.device(dev))                      # a strided view, a device object
    assert t.is_contiguous() and np.array_equal(t.cpu().numpy(), HOST[:, ::2])
    assert tuple(m.upload([[1, 2]], dev, i4).shape) == (1, 2)


def test_as_input_hands_device_tensors_on_or_refuses(torch, dev):
    t = m.upload(HOST, dev)
    assert m.is_dev(t) and not m.is_dev(t.cpu()) and not m.is_dev(HOST)
    assert m.as_input(t) is t and m.as_input(t.int(), i4) is not None and m.as_input(t.long(), i8).dtype == torch.int64
    for bad, dt in ((t.float(), f8), (t.t(), f8), (t[:, ::2], f8), (t, i4), (t.int(), i8), (t.int().t(), i4)):
        with pytest.raises(ValueError, match="device tensors must be contiguous %s" % np.dtype(dt).name):
            m.as_input(bad, dt)


def test_on_side_moves_either_way(torch, ctx, dev):
    t = m.upload(HOST, dev)
    up = m.on_side(np.asfortranarray(HOST.astype(np.float32)), t, f8, (3, 4), "a")           # host -> the side of a tensor
    assert up.is_cuda and up.device == t.device and up.dtype == torch.float64 and up.is_contiguous()
    assert np.array_equal(up.cpu().numpy(), HOST)
    up = m.on_side([0, 1, 0], (True, ctx.device), i4, (3,), "a")                             # host -> (device?, index)
    assert up.is_cuda and up.device.index == ctx.device and up.dtype == torch.int32 and up.tolist() == [0, 1, 0]
    assert m.on_side(t, t, f8, (3, 4), "a") is t and m.on_side(t, (True, ctx.device), f8, (3, 4), "a") is t
    for ref in (HOST, (False, ctx.device)):                                                  # device -> host
        down = m.on_side(t, ref, f8, (3, 4), "a")
        assert isinstance(down, np.ndarray) and down.dtype == f8 and down.flags.c_contiguous and np.array_equal(down, HOST)
    down = m.on_side(t.float().t(), HOST, f8, (4, 3), "a")
    assert isinstance(down, np.ndarray) and down.dtype == f8 and down.flags.c_contiguous and np.array_equal(down, HOST.T)
    b = m.on_side(0.5, t, f8, (3,), "a", broadcast=True)                                     # a host value, broadcast first
    assert b.is_cuda and b.dtype == torch.float64 and b.tolist() == [0.5] * 3
    b = m.on_side(np.float32([0, 1, 2, 3]), t, f8, (3, 4), "a", broadcast=True)
    assert b.is_cuda and b.is_contiguous() and np.array_equal(b.cpu().numpy(), np.tile([0.0, 1, 2, 3], (3, 1)))
    assert m.on_side(None, t, f8, (3,), "a") is None
    for bad in (t.float(), t.t().contiguous().t()):
        with pytest.raises(ValueError, match="device tensors must be contiguous float64"):
            m.on_side(bad, t, f8, (3, 4), "a")
    for arg in (t, HOST):
        with pytest.raises(ValueError, match=r"what must be \(4, 3\), got \(3, 4\)"):
            m.on_side(arg, t, f8, (4, 3), "what")
    with pytest.raises(ValueError, match=r"what must be \(4,\), got \(3, 4\)"):
        m.on_side(t, t, f8, (4,), "what", broadcast=True)                                    # a tensor is not broadcast


def test_new_honours_side_dtype_and_zeroing(torch, ctx, dev):
    t = m.upload(HOST, dev)
    for dt, tdt in ((f8, torch.float64), (i4, torch.int32), (i8, torch.int64)):
        for ref in (t, (True, ctx.device)):
            a = m.new(ref, (3, 4), dt)
            assert a.is_cuda and a.device.index == ctx.device and a.dtype == tdt and tuple(a.shape) == (3, 4) and a.is_contiguous()
            z = m.new(ref, (3, 4), dt, zero=True)
            assert z.is_cuda and z.dtype == tdt and not z.any().item()
    assert m.new(t, (0, 4)).numel() == 0
    assert isinstance(m.new((False, ctx.device), (3,), i4), np.ndarray)


def test_checked_validates_side_shape_dtype_layout(torch, dev):
    t = m.upload(HOST, dev)
    out = torch.empty((3, 4), dtype=torch.float64, device=dev)
    assert m.checked(out, t, (3, 4), f8, "out") is out and m.is_canonical(out, f8, (3, 4), t)
    spans = torch.empty((3, 4), dtype=torch.int64, device=dev)
    assert m.checked(spans, t, (3, 4), i8, "spans") is spans
    made = m.checked(None, t, (3, 4), i8, "spans", zero=True)
    assert made.is_cuda and made.dtype == torch.int64 and not made.any().item()
    # float64 is no int64 although both names end alike in their last two characters; int32 is no int64
    for bad, dt in ((out.float(), f8), (out.t(), f8), (out[:2], f8), (out.cpu().numpy(), f8), (out, i8), (spans.int(), i8)):
        assert not m.is_canonical(bad, dt, (3, 4), t)
        with pytest.raises(ValueError, match=r"out must be a contiguous %s \(3, 4\) array on X's side" % np.dtype(dt).name):
            m.checked(bad, t, (3, 4), dt, "out", of="X")
    with pytest.raises(ValueError, match="on Q's side"):
        m.checked(out, HOST, (3, 4), f8, "out")                                              # a device out for host input
    assert m.is_canonical(out) and not m.is_canonical(out.t())                               # no shape, no side asked


# ------------------------------------------------------------------------------------------ mixed sides, end to end
def test_chain_groups_upload_their_keys(ctx, dev):
    k0, k1 = np.float32([0.5, 3.0, 1.0, 2.5, 2.0]), [1, 0, 3, 2, 4]
    host = ctx.gf_chain_groups(k0, k1, 4)
    assert host.dtype == np.uint32 and host.shape == (2, 4)
    assert np.array_equal(ctx.gf_chain_groups(m.upload(k0, dev, f8), m.upload(k1, dev, f8), 4), host)
    assert np.array_equal(ctx.gf_chain_groups(k0, m.upload(k1, dev, f8), 4), host)


def test_magnitudes_with_device_points_and_host_moments(ctx, dev):
    name = min(CASES, key=lambda n: CASES[n]["k"].size * CASES[n]["M0"].size)
    model = _Model(ctx, CASES[name])
    try:
        a, k = model.a, CASES[name]["k"]
        M0, Mw = ctx.ffi_magnitudes_batch(model.mid, a["Q"], k, a["P"])
        D0, Dw = ctx.ffi_magnitudes_batch(model.mid, m.upload(a["Q"], dev), k, a["P"])
        assert isinstance(M0, np.ndarray) and D0.is_cuda and Dw.is_cuda
        assert np.array_equal(D0.cpu().numpy(), M0) and np.array_equal(Dw.cpu().numpy(), Mw) and (M0 > 0).any()
        H0, Hw = ctx.ffi_magnitudes_batch(model.mid, a["Q"], m.upload(k, dev), a["P"])       # and the other way round
        assert isinstance(H0, np.ndarray) and np.array_equal(H0, M0) and np.array_equal(Hw, Mw)
    finally:
        model.close()


def test_geodetic_library_on_the_device_from_host_inputs(ctx):
    params = np.array([[0.5, -0.3, 3.0, 30.0, 60.0, 90.0, 2.0, 1.5, 1.0, 0.0],
                       [1.0, 0.2, 5.0, 120.0, 45.0, 0.0, 3.0, 2.0, 1.0, 0.0]])
    east, north = np.float32([-4.0, 1.5, 6.0]), [2.0, -3.0, 0.5]
    los = np.asfortranarray(np.array([[0.6, -0.1, 0.79], [0.0, 0.0, 1.0], [-0.5, 0.3, 0.81]]))
    odw = np.array([1.0, 0.5, 2.0])
    host = ctx.geo_gf_library(params, east, north, los, odw)
    devG = ctx.geo_gf_library(params, east, north, los, odw, device=True)
    assert isinstance(host, np.ndarray) and host.shape == (2, 3) and np.isfinite(host).all() and host.any()
    assert devG.is_cuda and devG.device.index == ctx.device and tuple(devG.shape) == (2, 3)
    assert np.array_equal(devG.cpu().numpy(), host)


def test_density_with_device_traces_scalar_tmin_host_extent(ctx, dev):
    Y = np.array([[[0.1, 0.8, -0.4, 0.3]], [[-0.7, 0.2, 0.6, -0.1]]])                        # (2, 1, 4)
    extent = np.array([0.0, 2.0, -1.0, 1.0])
    host = ctx.trace_density_update(Y, 0.25, 0.5, extent, grid_size=(6, 5))
    got = ctx.trace_density_update(m.upload(Y, dev), 0.25, 0.5, extent, grid_size=(6, 5))
    assert isinstance(host, np.ndarray) and host.shape == (1, 6, 5) and host.any()
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), host)
    again = ctx.trace_density_update(m.upload(Y, dev), 0.25, 0.5, extent, grid_size=(6, 5), grid=got)
    assert again is got
    assert np.array_equal(got.cpu().numpy(), ctx.trace_density_update(Y, 0.25, 0.5, extent, grid_size=(6, 5), grid=host.copy()))
