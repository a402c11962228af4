"""The argument scaffold of the Python bindings, the torch-side counterpart of csrc/host_call.h: what every binding of an add-on
does to its tensors before the C-ABI call and to its outputs after it.  The C-ABI takes raw pointers and trusts the sizes, so every
tensor a kernel will read or write passes through _dev_f32 here.  Plain functions; a refusal is a FotgError, before any HIP call."""
import ctypes as C

import torch

from ._lib import FotgError


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(device=None):
    """the caller's current stream ON THE CONTEXT'S DEVICE (not on whatever device happens to be current)"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _dev_f32(t, name, device=None, shape=None, dtype=torch.float32):
    """The C-ABI takes raw pointers and trusts the sizes: everything a kernel will read or write is checked here --
    dtype, contiguity, device and, where the caller knows it, the exact shape."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise FotgError("%s must be a contiguous %s CUDA(HIP) tensor" % (name, str(dtype).replace("torch.", "")))
    if device is not None and t.device != device:
        raise FotgError("%s lives on %s, the context on %s" % (name, t.device, device))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise FotgError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t


def flow_form(flow, name="flow"):
    """a dense flow or a batch of them, by its dimensions alone"""
    if not isinstance(flow, torch.Tensor) or flow.dim() not in (3, 4) or flow.shape[-1] != 2:
        raise FotgError("%s must be a (n, h, w, 2) or (h, w, 2) tensor" % name)


def dense_flow(flow, name="flow", max_dim=None):
    """flow (n, h, w, 2) or (h, w, 2) checked: (the flow as (n, h, w, 2), whether it was single, n, h, w); max_dim: None or the
    most rows and columns the feature takes"""
    flow_form(flow, name)
    single = flow.dim() == 3
    f = flow.unsqueeze(0) if single else flow
    n, h, w = (int(v) for v in f.shape[:3])
    if max_dim is None and (n < 1 or h < 1 or w < 1):
        raise FotgError("flow has an empty dimension: %s" % (tuple(flow.shape),))
    if max_dim is not None and (n < 1 or h < 1 or w < 1 or h > max_dim or w > max_dim):
        raise FotgError("flow must have between 1 and %d rows and columns: %s" % (max_dim, tuple(flow.shape)))
    return _dev_f32(f, name), single, n, h, w


def two_channel(ofc, what):
    """what: the feature's phrase, "the warp needs a two-channel flow" """
    if ofc.nch != 2:
        raise FotgError("%s (this is a depth-mode context)" % what)


def coarse_flow(ofc, coarse, what, name="coarse", count="n"):
    """a batch of the context's coarse flows, by the context's mode and its batch: n.  Its shape is coarse_shape's to check."""
    n = coarse.shape[0] if isinstance(coarse, torch.Tensor) and coarse.dim() == 4 else 0
    two_channel(ofc, what)
    if n < 1 or n > ofc.max_batch:
        raise FotgError("%s must be (%s, h_l, w_l, 2) with 1 <= %s <= max_batch" % (name, count, count))
    return int(n)


def coarse_shape(ofc, coarse, name, n):
    wl, hl = ofc.out_size()
    return _dev_f32(coarse, name, ofc.device, (n, hl, wl, 2))


def batched(t, single):
    """the input of a single call with the batch dimension the C-ABI expects; what is no tensor is left for the check to refuse"""
    return t.unsqueeze(0) if single and isinstance(t, torch.Tensor) else t


def optional(t, name, device, shape, dtype=torch.float32, single=False):
    """None, or the checked tensor (batched when single)"""
    return None if t is None else _dev_f32(batched(t, single), name, device, shape, dtype)


def image_stack(t, name, n, h, w, device, dtypes, single=False):
    """an image stack (n, h, w) or (n, h, w, c), c in (1, 3), of one of dtypes, checked: (the stack, batched when single, channels).
    n = None: a stack of its own size (h and w are not looked at)."""
    t = batched(t, single)
    if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4) or t.dtype not in dtypes:
        raise FotgError("%s must be a (n, h, w) or (n, h, w, c) %s tensor" % (name, " or ".join(str(d).replace("torch.", "") for d in dtypes)))
    if n is None:
        n, h, w = (int(v) for v in t.shape[:3])
        if min(n, h, w) < 1:
            raise FotgError("%s has an empty dimension: %s" % (name, tuple(t.shape)))
    ch = 1 if t.dim() == 3 else int(t.shape[3])
    if ch not in (1, 3) or tuple(t.shape[:3]) != (n, h, w):
        raise FotgError("%s has shape %s, expected (%d, %d, %d) or (%d, %d, %d, 1 | 3)" % (name, tuple(t.shape), n, h, w, n, h, w))
    return _dev_f32(t, name, device, dtype=t.dtype), ch


def unbatch(outs, single, always_tuple=False):
    """the outputs that were asked for (the others are None), without the batch dimension when single; one output alone is
    returned as itself unless the caller always returns a tuple"""
    outs = tuple(o[0] if single else o for o in outs if o is not None)
    return outs[0] if len(outs) == 1 and not always_tuple else outs


def cat_chunks(parts):
    """the results of the chunks of a driver -- each a tensor, None, or a tuple of such, all of one structure -- joined along
    dimension 0; one chunk alone is returned as it is"""
    first = parts[0]
    if first is None or len(parts) == 1:
        return first
    if isinstance(first, tuple):
        return tuple(cat_chunks([p[j] for p in parts]) for j in range(len(first)))
    if first.dtype == torch.uint32:                # torch.cat has no uint32 kernel; the bits are those of int32
        return torch.cat([t.view(torch.int32) for t in parts]).view(torch.uint32)
    return torch.cat(parts)
