"""CCPM's convolution + k-max pooling stack (csrc/ccpm.hip)."""
import torch

from .. import lib as L
from ..marshal import call, i32s, ptr, rows2, rows3, workspace


class CCPMConvFunction(torch.autograd.Function):
    """ConvLayer of CCPM on ``E [B, F, D]`` (csrc/ccpm.hip): ``(E, params, widths, filters, ks, keep) -> [B, C_L * k_L * D]``.
    ``params`` is the packed vector the kernel reads (weight, bias of layer 1, then layer 2, ...).  With ``keep`` (a
    backward will follow) the forward also records the field every pooled element came from, one byte each, and the
    backward routes by it; without (``predict``) the kernel gets no selection buffer."""

    @staticmethod
    def forward(ctx, E, params, widths, filters, ks, keep):
        E, lde = rows3(E, "CCPM conv input")
        B, F, D = E.shape
        P = params.detach().float().contiguous()
        nl = len(filters)
        arrs = [i32s(a) for a in (widths, filters, ks)]
        n_out = int(filters[-1]) * int(ks[-1]) * D
        n_sel = sum(int(c) * int(k) for c, k in zip(filters, ks)) * D
        sel = torch.empty((B, n_sel), dtype=torch.uint8, device=E.device) if keep else None
        out = torch.empty((B, n_out), dtype=torch.float32, device=E.device)
        call("dctr_ccpm_fwd", ptr(E), lde, B, F, D, nl, *arrs, ptr(P), ptr(out), n_out,
             ptr(sel), L.stream_handle(E.device))
        if keep:
            ctx.save_for_backward(E, P, sel)
            ctx.spec = (tuple(widths), tuple(filters), tuple(ks))
        return out

    @staticmethod
    def backward(ctx, gout):
        E, P, sel = ctx.saved_tensors
        widths, filters, ks = ctx.spec
        E, lde = rows3(E, "CCPM conv input")
        B, F, D = E.shape
        dev = E.device
        nl = len(filters)
        arrs = [i32s(a) for a in (widths, filters, ks)]
        gout, ldg = rows2(gout, "CCPM conv gradient")
        gE = torch.empty((B, F, D), dtype=torch.float32, device=dev)
        gP = torch.empty_like(P)
        ws = workspace("dctr_ccpm_bwd_workspace_floats", B, P.numel(), device=dev)
        call("dctr_ccpm_bwd", ptr(E), lde, B, F, D, nl, *arrs, ptr(P), ptr(sel), ptr(gout),
             ldg, ptr(gE), F * D, ptr(gP), ptr(ws), L.stream_handle(dev))
        return gE, gP, None, None, None, None

