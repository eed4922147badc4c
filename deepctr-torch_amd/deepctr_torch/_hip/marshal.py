"""The one place tensors become C-ABI arguments (include/dctr.h): device pointers, int arrays, row layouts with their
leading dimensions, workspaces, checked calls.  Everything reaches the library through the module ``lib`` at call time."""
import ctypes

import torch

from . import lib as L


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def i32s(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def i64s(values):
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


def r4(n):
    return (int(n) + 3) // 4 * 4


def rows2(t, what):
    """``(t, ld)``: ``[B, W]`` float32 with unit stride inside a row and rows that do not overlap.  A tensor that already is
    -- contiguous, or a row-strided view such as a column slice of the gather's output -- comes back as the same object;
    anything else as a contiguous float32 copy.  ``ld``: the row stride, or W for a single row."""
    L.require_gpu(t, what)
    if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or \
            (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.float().contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def rows3(t, what):
    """``(t, ld)``: ``[B, R, D]`` float32 with contiguous (R, D) rows; the batch stride may be anything >= R*D (views of the
    gather's output and of a previous layer's feature maps pass through without a copy)."""
    L.require_gpu(t, what)
    if t.dtype != torch.float32:
        t = t.float()
    B, R, D = t.shape
    if (D > 1 and t.stride(2) != 1) or (R > 1 and t.stride(1) != D) or (B > 1 and t.stride(0) < R * D):
        t = t.contiguous()
    return t, (t.stride(0) if B > 1 else R * D)


def padded_rows(t, ld_min=0, vec=4):
    """``(t, ld)``: ``[B, W]`` float32 rows for ``vec``-wide loads -- unit inner stride, base pointer on ``4 * vec`` bytes
    (16 by default), row stride a multiple of ``vec`` and at least ``max(W, ld_min)``.  A tensor that already is (a
    slab-seated weight, an aligned view of the gather's output) passes through; anything else gets a copy with
    ``ld = r4(max(W, ld_min))`` whose columns behind W are zero."""
    W = t.shape[1] if t.dim() == 2 else -1
    if t.dtype != torch.float32 or W < 0 or (W > 1 and t.stride(1) != 1) or t.stride(0) % vec or \
            t.data_ptr() % (4 * vec) or t.stride(0) < max(W, ld_min):
        ld = r4(max(W, ld_min))
        buf = torch.zeros((t.shape[0], ld), dtype=torch.float32, device=t.device)
        buf[:, :W].copy_(t.detach())
        return buf, ld
    return t, t.stride(0)


def workspace(entry, *args, device):
    """float32 scratch of the size the library's ``entry`` (a ``*_workspace_floats`` function) reports, at least 1."""
    return torch.empty((max(1, getattr(L.lib(), entry)(*args)),), dtype=torch.float32, device=device)


def call(entry, *args):
    """Run the library's ``entry`` and raise, naming it, unless it returns DCTR_OK."""
    L.check(getattr(L.lib(), entry)(*args), entry)
