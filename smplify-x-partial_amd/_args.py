"""Arguments on their way into libsfx.so: the one check of a torch tensor handed to the library, the output tensor a caller may
supply, the stream argument, pointer-or-NULL and the cfg's ign_part_pairs.  The library dereferences what it is given, so
whatever is refused is refused here, with a ValueError / TypeError, before any launch.  There is no CPU fallback."""
import ctypes as C

import numpy as np


def tensor(name, t, shape, device=None, dtype=None, optional=False, convert=False, make_contiguous=False,
           non_tensor=TypeError, holder="the handle"):
    """`t` as the library reads it: a detached, contiguous CUDA tensor of `dtype` (default float32) and `shape`.
    shape: a tuple; None is a wildcard (the batch dimension of a call that takes B from this tensor).
    device: the torch.device the tensor must be on, `holder` naming in the message what lives there; None = any GPU.
    optional: None passes through (a NULL pointer).  convert: another dtype is converted, not refused.  make_contiguous:
    strides are repaired by a copy, not refused.  non_tensor: the exception class of an argument that is no tensor.
    What the tensor is gets checked before where it is."""
    import torch
    if t is None and optional:
        return None
    if not torch.is_tensor(t):
        raise non_tensor("%s: a torch tensor is needed, got %s" % (name, type(t).__name__))
    dtype = dtype or torch.float32
    if t.dim() != len(shape) or any(n is not None and n != m for n, m in zip(shape, t.shape)):
        want = tuple(("B" if i == 0 else "n") if n is None else n for i, n in enumerate(shape))
        raise ValueError("%s: shape %s, expected %s" % (name, tuple(t.shape), want))
    if t.dtype != dtype and not convert:
        raise ValueError("%s: %s is needed, got %s" % (name, str(dtype).replace("torch.", ""), t.dtype))
    if not t.is_contiguous() and not make_contiguous:
        raise ValueError("%s: a contiguous tensor is needed (strides %s)" % (name, tuple(t.stride())))
    if t.device.type != "cuda":
        raise ValueError("%s: a CUDA tensor is needed (no CPU fallback), got device %s" % (name, t.device))
    if device is not None and t.device != device:
        raise ValueError("%s: on %s, %s on %s" % (name, t.device, holder, device))
    return t.detach().to(dtype).contiguous()


def out_tensor(name, out, shape, device):
    """An output the caller may supply: `out` as it is when it is a float32 contiguous tensor of `shape` on `device`, a new
    one when it is None."""
    import torch
    if out is None:
        return torch.empty(list(shape), dtype=torch.float32, device=device)
    if (not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous()
            or out.device != device):
        raise ValueError("%s: a contiguous float32 %s tensor on %s is needed" % (name, tuple(shape), device))
    return out


def stream(given, device=None):
    """The stream argument of a call: `given` (a raw stream) or the current stream of `device` (None = the current device)."""
    import torch
    return C.c_void_p(given if given is not None else torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    """Device pointer of a tensor; None = NULL."""
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ign_pairs(ign_part_pairs):
    """The cfg's ign_part_pairs (["9,16", ...] strings or (a, b) tuples; None = none) as an int32 [n][2] array."""
    pairs = []
    for p in ign_part_pairs or []:
        a, b = (int(x) for x in p.split(",")) if isinstance(p, str) else p
        pairs.append((a, b))
    return np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2), dtype=np.int32)
