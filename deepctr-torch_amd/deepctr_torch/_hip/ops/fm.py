"""FM-family pooling over field embeddings: FM, BiInteractionPooling, the input-aware FM of IFM / DIFM, AFM (csrc/fm.hip,
iafm.hip, afm.hip)."""
import torch

from .. import lib as L
from ..marshal import call, ptr, r4, rows2, rows3, workspace


# ---- FM on explicit tensors (interaction.py:26-34) --------------------------------------------------
class FMFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, E):
        L.require_gpu(E, "FM input")
        if E.dim() != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % E.dim())
        E, lde = rows3(E, "FM input")
        B, F, D = E.shape
        y = torch.empty((B,), dtype=torch.float32, device=E.device)
        call("dctr_fm_fwd", ptr(E), lde, B, F, D, ptr(y), L.stream_handle(E.device))
        ctx.save_for_backward(E)
        return y.unsqueeze(1)

    @staticmethod
    def backward(ctx, gy):
        E, lde = rows3(ctx.saved_tensors[0], "FM input")
        B, F, D = E.shape
        gy = gy.reshape(B).contiguous().float()
        gE = torch.empty((B, F, D), dtype=torch.float32, device=E.device)
        call("dctr_fm_bwd", ptr(E), lde, B, F, D, ptr(gy), ptr(gE), F * D, 0, L.stream_handle(E.device))
        return gE


class BiPoolFunction(torch.autograd.Function):
    """BiInteractionPooling on the gather's rows (csrc/fm.hip): ``G [B, ld]`` (fields first, dense block at
    ``dense_off``) -> ``[B, r4(D + n_dense)]`` = ``[bi | dense]``, the NFM tower's input; the backward hands back a
    gradient with G's layout."""

    @staticmethod
    def forward(ctx, G, F, D, dense_off, n_dense):
        G, _ = rows2(G, "BiInteractionPooling input")
        B = G.shape[0]
        ld_o = r4(D + n_dense)
        out = torch.zeros((B, ld_o), dtype=torch.float32, device=G.device) if ld_o != D + n_dense else \
            torch.empty((B, ld_o), dtype=torch.float32, device=G.device)
        call("dctr_bi_pooling_fwd", ptr(G), G.stride(0), B, F, D, dense_off, n_dense, ptr(out), ld_o,
             L.stream_handle(G.device))
        ctx.save_for_backward(G)
        ctx.dims = (F, D, dense_off, n_dense)
        return out

    @staticmethod
    def backward(ctx, gout):
        (G,) = ctx.saved_tensors
        F, D, dense_off, n_dense = ctx.dims
        B = G.shape[0]
        gout, _ = rows2(gout, "BiInteractionPooling gradient")
        gG = torch.zeros_like(G) if G.shape[1] != F * D + n_dense or (n_dense and dense_off != F * D) else \
            torch.empty_like(G)
        call("dctr_bi_pooling_bwd", ptr(G), G.stride(0), B, F, D, dense_off, n_dense, ptr(gout), gout.stride(0),
             ptr(gG), gG.stride(0), L.stream_handle(G.device))
        return gG, None, None, None, None


# ---- input-aware FM of IFM / DIFM (ifm.py:74-83, difm.py:96-102, basemodel.py:80-91; csrc/iafm.hip) -----------------
class IAFMFunction(torch.autograd.Function):
    """``(G, Wl | None, Z1, Z2 | None) -> (y_lin [B, 1], y_fm [B, 1])`` with ``m = F softmax(Z1)`` or ``Z1 + Z2``:
    the refined wide sum and FM on the refined embeddings, one launch per direction.  ``G [B, ld]`` is the gather's buffer
    (its first ``F * D`` columns are read in place; the gradient handed back has G's layout, zero outside the field block),
    ``Wl [B, n_wl + 1]`` the per-field wide buffer of a ``wide_per_field`` plan (its gradient is that plan's ``g_wide``)."""

    @staticmethod
    def forward(ctx, G, Wl, Z1, Z2, mode, F, D, n_wl):
        G, _ = rows2(G, "input-aware FM input")
        Z1, _ = rows2(Z1, "input-aware factor")
        Z2 = rows2(Z2, "input-aware factor")[0] if Z2 is not None else None
        Wl = rows2(Wl, "per-field wide weights")[0] if Wl is not None else None
        B = G.shape[0]
        dev = G.device
        m = torch.empty((B, F), dtype=torch.float32, device=dev)
        y_lin = torch.empty((B,), dtype=torch.float32, device=dev)
        y_fm = torch.empty((B,), dtype=torch.float32, device=dev)
        call("dctr_iafm_fwd", ptr(G), G.stride(0), ptr(Wl), Wl.stride(0) if Wl is not None else 0, n_wl, ptr(Z1),
             Z1.stride(0), ptr(Z2), Z2.stride(0) if Z2 is not None else 0, mode, B, F, D, ptr(m), F, ptr(y_lin),
             ptr(y_fm), L.stream_handle(dev))
        ctx.save_for_backward(G, Wl, m)
        ctx.cfg = (int(mode), int(F), int(D), int(n_wl), Z2 is not None)
        ctx.set_materialize_grads(False)
        return y_lin.unsqueeze(1), y_fm.unsqueeze(1)

    @staticmethod
    def backward(ctx, g_lin, g_fm):
        G, Wl, m = ctx.saved_tensors
        mode, F, D, n_wl, two = ctx.cfg
        if g_lin is None and g_fm is None:
            return None, None, None, None, None, None, None, None
        B = G.shape[0]
        dev = G.device
        g_lin = g_lin.reshape(B).contiguous().float() if g_lin is not None else None
        g_fm = g_fm.reshape(B).contiguous().float() if g_fm is not None else None
        gG = torch.empty_like(G)
        if G.shape[1] > F * D:
            gG[:, F * D:].zero_()      # (the kernel writes the field block only; autograd adds the tower's gradient to this)
        gWl = torch.empty_like(Wl) if Wl is not None else None
        gZ = torch.empty((B, F), dtype=torch.float32, device=dev)
        call("dctr_iafm_bwd", ptr(G), G.stride(0), ptr(Wl), Wl.stride(0) if Wl is not None else 0, n_wl, ptr(m), F,
             mode, B, F, D, ptr(g_lin), ptr(g_fm), ptr(gG), gG.stride(0), ptr(gWl),
             gWl.stride(0) if gWl is not None else 0, ptr(gZ), F, L.stream_handle(dev))
        return gG, gWl, gZ, (gZ if two else None), None, None, None, None


def iafm_supported(F, D):
    return bool(L.lib().dctr_iafm_supported(int(F), int(D)))


def iafm(G, Wl, Z1, Z2, softmax, F, D):
    """``(y_lin [B, 1], y_fm [B, 1])`` of the input-aware FM over the gather's buffer ``G`` (see IAFMFunction).  ``Wl`` is the
    per-field wide buffer ``[B, n + 1]`` (n = F, or 0 for a linear side of dense columns only) or None (no linear side).
    Shapes the kernel does not hold (``dctr_iafm_supported``) take the same formulas as torch ops."""
    n_wl = 0 if Wl is None else int(Wl.shape[1]) - 1
    if iafm_supported(F, D):
        return IAFMFunction.apply(G, Wl, Z1, Z2, L.IAFM_SOFTMAX if softmax else L.IAFM_SUM, int(F), int(D), n_wl)
    B = G.shape[0]
    m = float(F) * Z1.softmax(1) if softmax else Z1 + Z2
    y_lin = torch.zeros((B, 1), dtype=G.dtype, device=G.device)
    if Wl is not None:
        if n_wl:
            y_lin = y_lin + torch.sum(Wl[:, :n_wl] * m, dim=1, keepdim=True)
        y_lin = y_lin + Wl[:, n_wl:n_wl + 1]
    v = G[:, :F * D].reshape(B, F, D) * m.unsqueeze(-1)
    y_fm = 0.5 * torch.sum(torch.pow(torch.sum(v, dim=1), 2) - torch.sum(v * v, dim=1), dim=1, keepdim=True)
    return y_lin, y_fm


class AFMFunction(torch.autograd.Function):
    """AFMLayer on ``E [B, F, D]`` (csrc/afm.hip): ``(E, W [D, A], b [A], h [A, 1], p [D, 1]) -> [B, 1]``."""

    @staticmethod
    def forward(ctx, E, W, b, h, p):
        E, lde = rows3(E, "AFM input")
        B, F, D = E.shape
        A = W.shape[1]
        if D > 64 or A > 32 or F > 64 or F < 2:
            raise NotImplementedError("the gfx950 AFM kernel supports 2 <= fields <= 64, embedding_dim <= 64, "
                                      "attention_factor <= 32 (got F=%d, D=%d, A=%d)" % (F, D, A))
        Wc, bc, hc, pc = (t.detach().float().contiguous() for t in (W, b, h.reshape(-1), p.reshape(-1)))
        y = torch.empty((B,), dtype=torch.float32, device=E.device)
        call("dctr_afm_fwd", ptr(E), lde, B, F, D, A, ptr(Wc), ptr(bc), ptr(hc), ptr(pc), ptr(y),
             L.stream_handle(E.device))
        ctx.save_for_backward(E, Wc, bc, hc, pc)
        ctx.shapes = (tuple(h.shape), tuple(p.shape))
        return y.unsqueeze(1)

    @staticmethod
    def backward(ctx, gy):
        E, W, b, h, p = ctx.saved_tensors
        E, lde = rows3(E, "AFM input")
        B, F, D = E.shape
        A = W.shape[1]
        dev = E.device
        gy = gy.reshape(B).contiguous().float()
        gE = torch.empty((B, F, D), dtype=torch.float32, device=dev)
        gW, gb = torch.empty_like(W), torch.empty_like(b)
        gh, gp = torch.empty_like(h), torch.empty_like(p)
        ws = workspace("dctr_afm_bwd_workspace_floats", B, D, A, device=dev)
        call("dctr_afm_bwd", ptr(E), lde, B, F, D, A, ptr(W), ptr(b), ptr(h), ptr(p), ptr(gy), ptr(gE), F * D,
             ptr(gW), ptr(gb), ptr(gh), ptr(gp), ptr(ws), L.stream_handle(dev))
        return gE, gW, gb, gh.reshape(ctx.shapes[0]), gp.reshape(ctx.shapes[1])

