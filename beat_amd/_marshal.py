"""
How an array crosses from Python into ``libbeat_amd.so``: each rule once.

An array lives on one of two sides: the host (numpy; results come back as numpy) or a GPU (a torch CUDA tensor; results
are tensors on the same device).  The library reads contiguous arrays of one of three dtypes.  torch is imported only
where a tensor is at hand or has to be made, so the package imports without it.
"""
import numpy as np

_TORCH_DTYPES = {}


def torch_dtype(dtype):
    """the torch dtype of a numpy one (the only table of the three dtypes the library reads)"""
    if not _TORCH_DTYPES:
        import torch
        _TORCH_DTYPES.update({np.float64: torch.float64, np.int32: torch.int32, np.int64: torch.int64})
    return _TORCH_DTYPES[dtype]


def is_dev(a):
    """a torch tensor on a GPU (host tensors and everything numpy takes are the host side)"""
    return hasattr(a, "data_ptr") and not isinstance(a, np.ndarray) and a.is_cuda


def _device(ref):
    """the torch device of a side -- given as an array of that side or as a (device?, index) pair --, None for the host"""
    if isinstance(ref, tuple):
        return "cuda:%d" % ref[1] if ref[0] else None
    return ref.device if is_dev(ref) else None


def as_input(a, dtype=np.float64):
    """``a`` as the library reads it: a C-contiguous ``dtype`` view or copy of anything numpy takes.  A torch tensor (on
    either side) is handed on as it is, so it must be contiguous and of ``dtype`` already; None stays None."""
    if a is None:
        return None
    if hasattr(a, "data_ptr") and not isinstance(a, np.ndarray):
        if a.dtype != torch_dtype(dtype) or not a.is_contiguous():
            raise ValueError("device tensors must be contiguous %s" % np.dtype(dtype).name)
        return a
    return np.ascontiguousarray(a, dtype=dtype)


def upload(a, device, dtype=None):
    """host array -> tensor on ``device``; dtype None keeps the array's own"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)


def on_side(a, ref, dtype, shape, what, broadcast=False):
    """``a`` as a contiguous ``dtype`` array of ``shape`` on the side of ``ref`` (see ``_device``), moved there from the other
    side if need be; ``broadcast``: a host value is first broadcast to ``shape``.  None stays None."""
    if a is None:
        return None
    device = _device(ref)
    if is_dev(a) and device is None:
        a = a.cpu().numpy()
    if not is_dev(a):
        if broadcast:
            a = np.broadcast_to(np.asarray(a, dtype=dtype), shape)
        a = np.ascontiguousarray(a, dtype=dtype)
        if device is not None:
            a = upload(a, device)
    else:
        a = as_input(a, dtype)
    if tuple(a.shape) != tuple(shape):
        raise ValueError("%s must be %s, got %s" % (what, tuple(shape), tuple(a.shape)))
    return a


def new(ref, shape, dtype=np.float64, zero=False):
    """an uninitialised (``zero``: zeroed) ``dtype`` array of ``shape`` on the side of ``ref`` (see ``_device``)"""
    device = _device(ref)
    if device is None:
        return (np.zeros if zero else np.empty)(shape, dtype=dtype)
    import torch
    return (torch.zeros if zero else torch.empty)(shape, dtype=torch_dtype(dtype), device=device)


def is_canonical(a, dtype=np.float64, shape=None, ref=None):
    """whether the library can write into ``a`` as it stands: a contiguous ``dtype`` array (tensor) and, where given, of
    ``shape`` and on the side of the array ``ref``"""
    if isinstance(a, np.ndarray):
        ok = a.flags.c_contiguous and a.dtype == dtype
    else:
        ok = hasattr(a, "data_ptr") and a.is_contiguous() and a.dtype == torch_dtype(dtype)
    return bool(ok and (shape is None or tuple(a.shape) == tuple(shape)) and (ref is None or is_dev(a) == is_dev(ref)))


def checked(a, ref, shape, dtype, what, of="Q", zero=False):
    """the caller's ``a`` if it is canonical, of ``shape`` and on the side of the array ``ref`` (ValueError if not, naming
    ``what`` and the argument ``of`` whose side it is); None: a new array there"""
    if a is None:
        return new(ref, shape, dtype, zero)
    if not is_canonical(a, dtype, shape, ref):
        raise ValueError("%s must be a contiguous %s %s array on %s's side" % (what, np.dtype(dtype).name, tuple(shape), of))
    return a
