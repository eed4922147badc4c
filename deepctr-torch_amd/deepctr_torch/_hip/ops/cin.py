"""The Compressed Interaction Network of xDeepFM (interaction.py:207-248; csrc/cin.hip, head.hip)."""
import ctypes
import os

import torch

from .. import lib as L
from ..marshal import call, ptr, rows3, workspace


def cin_layer_forward(H, X0, W2d, bias, relu):
    """A = act(W . (H (x) X0) + bias): ``[B, h, D], [B, M, D] -> [B, O, D]`` (no autograd; see CINLayerFunction)."""
    H, ldh = rows3(H, "CIN hidden input")
    X0, ldx = rows3(X0, "CIN field input")
    B, h, D = H.shape
    M = X0.shape[1]
    O = W2d.shape[0]
    if M > 32:
        raise NotImplementedError("the gfx950 CIN kernels support at most 32 fields (got %d)" % M)
    W2d = W2d.contiguous()
    A = torch.empty((B, O, D), dtype=torch.float32, device=H.device)
    ws = workspace("dctr_cin_workspace_floats", h, M, O, device=H.device)
    call("dctr_cin_layer_fwd", ptr(H), ldh, ptr(X0), ldx, ptr(W2d), ptr(bias), B, h, M, D, O, int(bool(relu)),
         ptr(A), O * D, ptr(ws), L.stream_handle(H.device))
    return A


class CINLayerFunction(torch.autograd.Function):
    """One CIN layer with the activation (relu or none) fused: ``dctr_cin_layer_fwd`` / ``dctr_cin_layer_bwd``."""

    @staticmethod
    def forward(ctx, H, X0, W2d, bias, relu):
        A = cin_layer_forward(H, X0, W2d, bias, relu)
        ctx.relu = bool(relu)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(H, X0, W2d, A if relu else None)
        return A

    @staticmethod
    def backward(ctx, gA):
        H, X0, W2d, A = ctx.saved_tensors
        H, ldh = rows3(H, "CIN hidden input")
        X0, ldx = rows3(X0, "CIN field input")
        B, h, D = H.shape
        M, O = X0.shape[1], W2d.shape[0]
        gA = gA.contiguous().float()
        W2d = W2d.contiguous()
        dev = H.device
        gH = torch.empty((B, h, D), dtype=torch.float32, device=dev)
        gX0 = torch.empty((B, M, D), dtype=torch.float32, device=dev)
        gW = torch.empty((O, h * M), dtype=torch.float32, device=dev)
        gb = torch.empty((O,), dtype=torch.float32, device=dev) if ctx.has_bias else None
        ws = workspace("dctr_cin_bwd_workspace_floats", B, h, M, D, O, device=dev)
        call("dctr_cin_layer_bwd", ptr(gA), ptr(A), O * D, int(ctx.relu), ptr(H), ldh, ptr(X0), ldx, ptr(W2d), B,
             h, M, D, O, ptr(gH), h * D, ptr(gX0), M * D, 0, ptr(gW), ptr(gb), ptr(ws), L.stream_handle(dev))
        return gH, gX0, gW, gb, None


class CINStackFunction(torch.autograd.Function):
    """The whole CIN (interaction.py:207-248) as ONE autograd node, optionally with the bias-free 1-unit projection
    xDeepFM puts on its output (xdeepfm.py:72, :97):

        x        [B, F, D] field matrix, or the gather's [B, >= F*D] row matrix whose first F*D columns are the fields
                 (xDeepFM: the gradient comes back in that shape -- no view backward (fill + slice copy) behind the CIN)
        wb       W_1, b_1, W_2, b_2, ...: the conv1ds' ``[O, h*F, 1]`` weights and ``[O]`` biases (None = no bias)
        w_head   None -> returns the CIN output ``[B, featuremap_num]``; ``[1, featuremap_num]`` -> returns
                 ``[B, 1]`` = output @ w_head.T

    Every layer's pooling kernel writes its block of the ``[B, featuremap_num]`` output in place (no torch.cat) and the
    backward reads the blocks' gradients in place (no slice copies); the layers' field-matrix gradients accumulate in one
    buffer inside the kernels (no adds); with ``w_head`` the projection's backward towards the layers is folded into the
    gradient-assembly kernel (dctr_cin_pool_bwd) and its forward is one wave-per-row dot product (dctr_rows_dot).
    Per layer: dctr_cin_layer_fwd + dctr_cin_pool_fwd forward, dctr_cin_pool_bwd + dctr_cin_layer_bwd backward."""

    @staticmethod
    def forward(ctx, x, F, D, relu, split_half, w_head, *wb):
        if x.dim() == 2:
            if x.shape[1] < F * D or x.stride(1) != 1 or x.dtype != torch.float32:
                raise ValueError("CIN: the row matrix must hold F*D contiguous float32 columns")
            X0 = x[:, :F * D].unflatten(1, (F, D))
        else:
            X0 = x
        B = X0.shape[0]
        dev = x.device
        n = len(wb) // 2
        sizes = [wb[2 * i].shape[0] for i in range(n)]
        geo = []                          # per layer: (O, n_hidden, pool_from, offset of its block)
        off = 0
        for i, O in enumerate(sizes):
            last = i == n - 1
            nh = 0 if last else (O // 2 if split_half else O)
            pf = nh if split_half else 0
            geo.append((O, nh, pf, off))
            off += O - pf
        fm = off
        feat = torch.empty((B, fm), dtype=torch.float32, device=dev)
        As = []
        hidden = X0
        for i in range(n):
            O, nh, pf, o0 = geo[i]
            bias = wb[2 * i + 1]
            A = cin_layer_forward(hidden, X0, wb[2 * i].reshape(O, -1), bias, relu)
            if B > 0:
                call("dctr_cin_pool_fwd", ptr(A), B, O, D, pf, ctypes.c_void_p(feat.data_ptr() + 4 * o0), fm,
                     L.stream_handle(dev))
            As.append(A)
            hidden = A[:, :nh] if nh > 0 else None
        ctx.geo, ctx.relu, ctx.F, ctx.D, ctx.fm = geo, bool(relu), int(F), int(D), fm
        ctx.flat = x.dim() == 2
        ctx.x_cols = x.shape[1] if ctx.flat else 0
        ctx.has_head = w_head is not None
        ctx.has_bias = [wb[2 * i + 1] is not None for i in range(n)]
        ctx.w_shapes = [tuple(wb[2 * i].shape) for i in range(n)]
        ctx.save_for_backward(x, w_head, feat if ctx.has_head else None, *(list(wb[0::2]) + As))
        if not ctx.has_head:
            return feat
        if w_head.numel() != fm:
            raise ValueError("CIN head: %d weights for %d feature maps" % (w_head.numel(), fm))
        logit = torch.empty((B, 1), dtype=torch.float32, device=dev)
        wh = w_head.detach().contiguous()
        call("dctr_rows_dot", ptr(feat), fm, ptr(wh), B, fm, ptr(logit), L.stream_handle(dev))
        return logit

    @staticmethod
    def backward(ctx, g):
        sv = ctx.saved_tensors
        x, w_head, feat = sv[0], sv[1], sv[2]
        n = len(ctx.geo)
        Ws, As = sv[3:3 + n], sv[3 + n:3 + 2 * n]
        F, D, fm = ctx.F, ctx.D, ctx.fm
        dev = x.device
        B = x.shape[0]
        st = L.stream_handle(dev)
        g = g.contiguous().float()
        ctx_join = False
        if ctx.flat:
            X0 = x[:, :F * D].unflatten(1, (F, D))
            gx = torch.empty((B, ctx.x_cols), dtype=torch.float32, device=dev)
            # (the dense columns behind the fields are not the CIN's inputs: zeroed by the joining launch at the end, or here)
            ctx_join = B > 0 and (F * D) % 4 == 0 and ctx.x_cols % 4 == 0 and os.environ.get("DCTR_GLUE_KERNELS", "1") != "0"
            if ctx.x_cols > F * D and not ctx_join:
                gx[:, F * D:].zero_()
            ld_gx = ctx.x_cols
        else:
            X0 = x
            gx = torch.empty((B, F, D), dtype=torch.float32, device=dev)
            ld_gx = F * D
        X0r, ldx = rows3(X0, "CIN field input")
        g_wh = None
        if ctx.has_head:
            if B > 0 and os.environ.get("DCTR_GLUE_KERNELS", "1") != "0":
                # g_w = g^T feat as fixed-order column sums (csrc/head.hip k_colsum_part) instead of a [1, B] x [B, fm] GEMM
                g_wh = torch.empty((fm,), dtype=torch.float32, device=dev)
                ws = workspace("dctr_relu_bwd_bias_workspace_floats", B, fm, device=dev)
                call("dctr_rows_tdot", ptr(feat), feat.stride(0), ptr(g), B, fm, ptr(g_wh), ptr(ws), st)
                g_wh = g_wh.reshape(w_head.shape)
            else:
                g_wh = torch.mm(g.reshape(1, B), feat).reshape(w_head.shape)
            wh = w_head.detach().contiguous().reshape(-1)
        rets = [None] * (2 * n)
        g_hidden = None
        first_gh = None
        for i in range(n - 1, -1, -1):
            O, nh, pf, o0 = ctx.geo[i]
            A = As[i]
            H = X0 if i == 0 else As[i - 1][:, :ctx.geo[i - 1][1]]
            Hr, ldh = (X0r, ldx) if i == 0 else rows3(H, "CIN hidden input")
            h = Hr.shape[1]
            gA = torch.empty((B, O, D), dtype=torch.float32, device=dev)
            if ctx.has_head:
                gp, ld_gp, whp = ptr(g), 1, ctypes.c_void_p(wh.data_ptr() + 4 * o0)
            else:
                gp, ld_gp, whp = ctypes.c_void_p(g.data_ptr() + 4 * o0), fm, None
            if B > 0:
                # (the relu's backward is applied while gA is assembled: the layer kernels then need no mask loads)
                call("dctr_cin_pool_bwd", ptr(g_hidden) if nh > 0 else None, gp, ld_gp, whp,
                     ptr(A) if ctx.relu else None, B, O, D, nh, pf, ptr(gA), st)
            W2d = Ws[i].detach().reshape(O, -1)
            W2d = W2d if W2d.is_contiguous() else W2d.contiguous()
            # the hidden rows' gradient: the previous layer's g_hidden; layer 1's hidden state IS the field matrix -- its
            # two gradients meet in gx (the symmetric kernel writes them from different threads: a scratch + one add)
            gH = torch.empty((B, h, D), dtype=torch.float32, device=dev)
            gW = torch.empty((O, W2d.shape[1]), dtype=torch.float32, device=dev)
            gb = torch.empty((O,), dtype=torch.float32, device=dev) if ctx.has_bias[i] else None
            ws = workspace("dctr_cin_bwd_workspace_floats", B, h, F, D, O, device=dev)
            call("dctr_cin_layer_bwd", ptr(gA), ptr(A), O * D, 0, ptr(Hr), ldh, ptr(X0r), ldx, ptr(W2d), B, h, F,
                 D, O, ptr(gH), h * D, ptr(gx), ld_gx, int(i != n - 1), ptr(gW), ptr(gb), ptr(ws), st)
            rets[2 * i] = gW.reshape(ctx.w_shapes[i])
            rets[2 * i + 1] = gb
            if i == 0:
                first_gh = gH
            else:
                g_hidden = gH
        if B > 0:
            if ctx.flat and ctx_join:
                # gx[:, :F D] += first_gh and gx[:, F D:] = 0 in one launch (in place: every lane reads and writes its own words)
                fg = first_gh.reshape(B, F * D)
                call("dctr_rows_join", ptr(gx), ld_gx, ptr(fg), fg.stride(0), F * D, None, 0, 0, ptr(gx), ld_gx, B,
                     st)
            elif ctx.flat:
                gx[:, :F * D].add_(first_gh.reshape(B, F * D))
            else:
                gx.add_(first_gh)
        return (gx, None, None, None, None, g_wh) + tuple(rets)

