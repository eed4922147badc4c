"""CrossNet in its three parameterisations: vector, matrix, mixture of low-rank experts (csrc/cross.hip, cross_tower.hip)."""
import ctypes

import torch

from .. import lib as L
from .. import mlp as _mlp
from ..marshal import call, padded_rows, ptr, r4, rows2, workspace


class CrossNetVecFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, kernels, bias):
        X, ldx = rows2(X, "CrossNet input")
        B, W = X.shape
        Lyr = kernels.shape[0]
        if W > 2048:
            raise NotImplementedError("the gfx950 CrossNet kernel supports in_features <= 2048 (got %d)" % W)
        k2, b2 = kernels.reshape(Lyr, W).contiguous(), bias.reshape(Lyr, W).contiguous()
        Y = torch.empty((B, W), dtype=torch.float32, device=X.device)
        call("dctr_crossnet_vec_fwd", ptr(X), ldx, B, W, Lyr, ptr(k2), ptr(b2), ptr(Y), W,
             L.stream_handle(X.device))
        ctx.save_for_backward(X, k2, b2)
        ctx.kshape, ctx.bshape = kernels.shape, bias.shape
        return Y

    @staticmethod
    def backward(ctx, gY):
        X, k2, b2 = ctx.saved_tensors
        X, ldx = rows2(X, "CrossNet input")
        B, W = X.shape
        Lyr = k2.shape[0]
        gY, ldg = rows2(gY, "CrossNet output gradient")
        gX = torch.empty((B, W), dtype=torch.float32, device=X.device)
        gk, gb = torch.empty_like(k2), torch.empty_like(b2)
        ws = workspace("dctr_crossnet_vec_bwd_workspace_floats", B, W, Lyr, device=X.device)
        call("dctr_crossnet_vec_bwd", ptr(X), ldx, B, W, Lyr, ptr(k2), ptr(b2), ptr(gY), ldg, ptr(gX), W, ptr(gk), ptr(gb),
             ptr(ws), L.stream_handle(X.device))
        return gX, gk.reshape(ctx.kshape), gb.reshape(ctx.bshape)


class CrossNetMatFunction(torch.autograd.Function):
    """CrossNet, matrix parameterisation (reference interaction.py:448-451): ``x_{l+1} = x_0 * (x_l W_l^T + b_l) + x_l``
    for all layers in ONE forward launch (16 samples per workgroup, x_0 / x_l in LDS, fp32 MFMA) and, for the backward,
    one data launch + the tower's weight-gradient kernels (csrc/cross_tower.hip: dctr_crossnet_mat_fwd / _bwd)."""

    @staticmethod
    def _desc(Wpad, b2, hs, us, gW, gb, W):
        return _mlp.fill_desc([(Wpad[l], b2[l], hs[l], us[l], gW[l] if gW is not None else None,
                                gb[l] if gb is not None else None, W, W, Wpad.stride(1), hs[l].stride(0), 0)
                               for l in range(len(hs))])

    @staticmethod
    def forward(ctx, X, kernels, bias):
        L.require_gpu(X, "CrossNet input")
        B, W = X.shape
        Lyr = kernels.shape[0]
        ld = r4(W)
        X, _ = padded_rows(X)
        # weights with rows padded to a multiple of 4 floats (zeros), one [L, W, ld] block
        Wpad = torch.zeros((Lyr, W, ld), dtype=torch.float32, device=X.device)
        Wpad[:, :, :W].copy_(kernels.detach())
        b2 = bias.detach().reshape(Lyr, W).contiguous()
        hs = [torch.empty((B, ld), dtype=torch.float32, device=X.device) for _ in range(Lyr)]
        us = [torch.empty((B, ld), dtype=torch.float32, device=X.device) for _ in range(Lyr)]
        desc = CrossNetMatFunction._desc(Wpad, b2, hs, us, None, None, W)
        call("dctr_crossnet_mat_fwd", ctypes.byref(desc), ptr(X), X.stride(0), B, L.stream_handle(X.device))
        ctx.save_for_backward(X, Wpad, b2, *(hs + us))
        ctx.dims = (B, W, Lyr, ld)
        ctx.kshape, ctx.bshape = kernels.shape, bias.shape
        return hs[-1][:, :W]

    @staticmethod
    def backward(ctx, gY):
        B, W, Lyr, ld = ctx.dims
        saved = ctx.saved_tensors
        X, Wpad, b2 = saved[0], saved[1], saved[2]
        hs, us = list(saved[3:3 + Lyr]), list(saved[3 + Lyr:3 + 2 * Lyr])
        g = torch.zeros((B, ld), dtype=torch.float32, device=X.device)
        g[:, :W].copy_(gY)
        gW = torch.empty((Lyr, W, ld), dtype=torch.float32, device=X.device)
        gb = torch.empty((Lyr, W), dtype=torch.float32, device=X.device)
        gX = torch.empty((B, ld), dtype=torch.float32, device=X.device)
        desc = CrossNetMatFunction._desc(Wpad, b2, hs, us, gW, gb, W)
        ws = workspace("dctr_crossnet_mat_bwd_workspace_floats", ctypes.byref(desc), B, device=X.device)
        call("dctr_crossnet_mat_bwd", ctypes.byref(desc), ptr(X), X.stride(0), B, ptr(g), ld, ptr(gX), ld, ptr(ws),
             L.stream_handle(X.device))
        return gX[:, :W], gW[:, :, :W].reshape(ctx.kshape), gb.reshape(ctx.bshape)


class CrossNetMixFunction(torch.autograd.Function):
    """CrossNetMix of DCN-Mix (reference interaction.py:499-534): per cross layer a mixture of low-rank experts,
    ``x_{l+1} = x_0 * (sum_e softmax(x_l G^T)_e * tanh(tanh(x_l V_e) C_e^T) U_e^T + b) + x_l``.  All layers in ONE
    forward launch (csrc/cross_tower.hip ``dctr_crossnet_mix_fwd``: three dense fp32-MFMA layers per cross layer on a 16-sample
    tile kept in LDS) and one backward-data launch + the tower's weight-gradient kernels.  The weights travel packed:
    ``W1 = [V (E*R rows) | G (E rows)] x W``, ``W2 = blockdiag(C_e)``, ``W3[w, e*R + r] = U_e[w, r]``."""

    @staticmethod
    def _pack(U, V, C, G, bias):
        Lc, E, W, R = U.shape
        ER = E * R
        ldW, ldE = r4(W), r4(ER)
        dev = U.device
        W1 = torch.zeros((Lc, ER + E, ldW), dtype=torch.float32, device=dev)
        W1[:, :ER, :W] = V.permute(0, 1, 3, 2).reshape(Lc, ER, W)       # row e*R + r = V_e[:, r]
        W1[:, ER:, :W] = G.unsqueeze(0)
        W2 = torch.zeros((Lc, ER, ldE), dtype=torch.float32, device=dev)
        for e in range(E):
            W2[:, e * R:(e + 1) * R, e * R:(e + 1) * R] = C[:, e]         # v2[e, r] = sum_s C[e, r, s] v1[e, s]
        W3 = torch.zeros((Lc, W, ldE), dtype=torch.float32, device=dev)
        W3[:, :, :ER] = U.permute(0, 2, 1, 3).reshape(Lc, W, ER)        # W3[w, e*R + r] = U_e[w, r]
        return W1, W2, W3, bias.reshape(Lc, W).contiguous()

    @staticmethod
    def _desc(W1, W2, W3, b2, bufs, grads, dims):
        B, W, Lc, E, R = dims
        ER = E * R
        layers = []
        for lc in range(Lc):
            for k, (Wt, K, N) in enumerate(((W1[lc], W, ER + E), (W2[lc], ER, ER), (W3[lc], ER, W))):
                h, dh = bufs[3 * lc + k]
                gW, gb = grads[3 * lc + k] if grads is not None else (None, None)
                layers.append((Wt, b2[lc] if k == 2 else None, h, dh, gW, gb, K, N, Wt.stride(0), h.stride(0), 0))
        return _mlp.fill_desc(layers)

    @staticmethod
    def forward(ctx, X, U, V, C, G, bias):
        L.require_gpu(X, "CrossNetMix input")
        B, W = X.shape
        Lc, E, _, R = U.shape
        ER = E * R
        X, _ = padded_rows(X)
        W1, W2, W3, b2 = CrossNetMixFunction._pack(U.detach(), V.detach(), C.detach(), G.detach(), bias.detach())
        bufs = []
        for lc in range(Lc):
            for n in (ER + E, ER, W):
                bufs.append((torch.empty((B, r4(n)), dtype=torch.float32, device=X.device),
                             torch.empty((B, r4(n)), dtype=torch.float32, device=X.device)))
        dims = (B, W, Lc, E, R)
        desc = CrossNetMixFunction._desc(W1, W2, W3, b2, bufs, None, dims)
        call("dctr_crossnet_mix_fwd", ctypes.byref(desc), E, R, ptr(X), X.stride(0), B, L.stream_handle(X.device))
        ctx.save_for_backward(X, W1, W2, W3, b2, *[t for pair in bufs for t in pair])
        ctx.dims = dims
        ctx.shapes = (U.shape, V.shape, C.shape, G.shape, bias.shape)
        return bufs[-1][0][:, :W]

    @staticmethod
    def backward(ctx, gY):
        B, W, Lc, E, R = ctx.dims
        ER = E * R
        saved = ctx.saved_tensors
        X, W1, W2, W3, b2 = saved[:5]
        flat = saved[5:]
        bufs = [(flat[2 * i], flat[2 * i + 1]) for i in range(3 * Lc)]
        dev = X.device
        ld = r4(W)
        g = torch.zeros((B, ld), dtype=torch.float32, device=dev)
        g[:, :W].copy_(gY)
        gW1, gW2, gW3 = torch.empty_like(W1), torch.empty_like(W2), torch.empty_like(W3)
        gb = torch.empty((Lc, W), dtype=torch.float32, device=dev)
        grads = []
        for lc in range(Lc):
            grads += [(gW1[lc], None), (gW2[lc], None), (gW3[lc], gb[lc])]
        gX = torch.empty((B, ld), dtype=torch.float32, device=dev)
        desc = CrossNetMixFunction._desc(W1, W2, W3, b2, bufs, grads, ctx.dims)
        ws = workspace("dctr_crossnet_mix_bwd_workspace_floats", ctypes.byref(desc), B, device=dev)
        call("dctr_crossnet_mix_bwd", ctypes.byref(desc), E, R, ptr(X), X.stride(0), B, ptr(g), ld, ptr(gX), ld,
             ptr(ws), L.stream_handle(dev))
        # unpack: V / G from the rows of gW1, the diagonal blocks of gW2, U from gW3
        gV = gW1[:, :ER, :W].reshape(Lc, E, R, W).permute(0, 1, 3, 2)
        gG = gW1[:, ER:, :W].sum(0)
        gC = torch.stack([gW2[:, e * R:(e + 1) * R, e * R:(e + 1) * R] for e in range(E)], dim=1)
        gU = gW3[:, :, :ER].reshape(Lc, W, E, R).permute(0, 2, 1, 3)
        sU, sV, sC, sG, sb = ctx.shapes
        return gX[:, :W], gU.reshape(sU), gV.reshape(sV), gC.reshape(sC), gG.reshape(sG), gb.reshape(sb)

