"""AFN's logarithmic transformation layer (csrc/log_transform.hip)."""
import torch

from .. import lib as L
from ..marshal import call, ptr, rows2, rows3, workspace


def _f32(t):
    return t.detach().float().contiguous()


class LogTransformFunction(torch.autograd.Function):
    """LogTransformLayer on ``X [B, F, E]`` (csrc/log_transform.hip):
    ``(X, W, bias, bn0_w, bn0_b, bn1_w, bn1_b, mean0, var0, mean1, var1, train, keep) -> (out [B, E*H], stats [4, E])``.

    ``train``: both norms use the batch's statistics, which come back in ``stats`` (mean0, var0, mean1, var1; the
    variances biased; float64, the precision the backward normalises in) for the caller's running-statistics update; the four statistics arguments are ignored.  Otherwise
    one launch on the statistics handed in, and ``stats`` is empty.  ``keep`` (a backward will follow; train mode only)
    saves the inputs and ``stats`` -- nothing of the output's size."""

    @staticmethod
    def forward(ctx, X, W, bias, bn0_w, bn0_b, bn1_w, bn1_b, mean0, var0, mean1, var1, train, keep):
        X, ldx = rows3(X, "log transform input")
        B, F, E = X.shape
        W, bias = _f32(W), _f32(bias).reshape(-1)
        H = W.shape[1]
        bn = [_f32(t) for t in (bn0_w, bn0_b, bn1_w, bn1_b)]
        dev = X.device
        out = torch.empty((B, E * H), dtype=torch.float32, device=dev)
        if train:
            stats = torch.empty((4, E), dtype=torch.float64, device=dev)
            ws = workspace("dctr_log_transform_workspace_floats", B, F, E, H, device=dev)
            call("dctr_log_transform_fwd_train", ptr(X), ldx, B, F, E, H, ptr(W), ptr(bias), *[ptr(t) for t in bn],
                 ptr(out), E * H, ptr(stats), ptr(ws), L.stream_handle(dev))
        else:
            if keep:
                raise RuntimeError("LogTransformFunction: the backward exists for batch statistics (train=True) only")
            stats = torch.empty((0, E), dtype=torch.float64, device=dev)
            run = [_f32(t) for t in (mean0, var0, mean1, var1)]
            call("dctr_log_transform_fwd_eval", ptr(X), ldx, B, F, E, H, ptr(W), ptr(bias), ptr(bn[0]), ptr(bn[1]),
                 ptr(run[0]), ptr(run[1]), ptr(bn[2]), ptr(bn[3]), ptr(run[2]), ptr(run[3]), ptr(out), E * H,
                 L.stream_handle(dev))
        if keep:
            ctx.save_for_backward(X, W, bias, bn[0], bn[1], bn[2], stats)
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, gout, _gstats):
        X, W, bias, bn0_w, bn0_b, bn1_w, stats = ctx.saved_tensors
        X, ldx = rows3(X, "log transform input")
        B, F, E = X.shape
        H = W.shape[1]
        dev = X.device
        gout, ldg = rows2(gout, "log transform gradient")
        gX = torch.empty((B, F, E), dtype=torch.float32, device=dev)
        gW = torch.empty((F, H), dtype=torch.float32, device=dev)
        gbias = torch.empty((1, 1, H), dtype=torch.float32, device=dev)
        gbn = torch.empty((4, E), dtype=torch.float32, device=dev)
        ws = workspace("dctr_log_transform_workspace_floats", B, F, E, H, device=dev)
        call("dctr_log_transform_bwd", ptr(X), ldx, B, F, E, H, ptr(W), ptr(bias), ptr(bn0_w), ptr(bn0_b), ptr(bn1_w),
             ptr(stats), ptr(gout), ldg, ptr(gX), F * E, ptr(gW), ptr(gbias), ptr(gbn[0]), ptr(gbn[1]), ptr(gbn[2]),
             ptr(gbn[3]), ptr(ws), L.stream_handle(dev))
        return gX, gW, gbias, gbn[0], gbn[1], gbn[2], gbn[3], None, None, None, None, None, None
