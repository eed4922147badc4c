"""Sequence and attention layers: InteractingLayer (AutoInt), DIN's attention pooling, DIEN's GRU family (csrc/interact.hip,
din.hip, gru_seq.hip)."""
import torch

from .. import lib as L
from ..marshal import call, i32s, i64s, ptr, rows2, rows3, workspace


class InteractFunction(torch.autograd.Function):
    """InteractingLayer on ``E [B, F, D]`` (csrc/interact.hip): ``(E, Wq, Wk, Wv, Wr | None) -> [B, F, D]``."""

    @staticmethod
    def forward(ctx, E, Wq, Wk, Wv, Wr, heads, scaling):
        E, lde = rows3(E, "InteractingLayer input")
        B, F, D = E.shape
        ws = [w.detach().float().contiguous() if w is not None else None for w in (Wq, Wk, Wv, Wr)]
        out = torch.empty((B, F, D), dtype=torch.float32, device=E.device)
        call("dctr_interacting_fwd", ptr(E), lde, B, F, D, int(heads), int(bool(scaling)), ptr(ws[0]), ptr(ws[1]),
             ptr(ws[2]), ptr(ws[3]), ptr(out), F * D, L.stream_handle(E.device))
        ctx.save_for_backward(E, *[w for w in ws if w is not None])
        ctx.cfg = (int(heads), bool(scaling), ws[3] is not None)
        return out

    @staticmethod
    def backward(ctx, gout):
        heads, scaling, has_res = ctx.cfg
        saved = ctx.saved_tensors
        E, Wq, Wk, Wv = saved[0], saved[1], saved[2], saved[3]
        Wr = saved[4] if has_res else None
        E, lde = rows3(E, "InteractingLayer input")
        B, F, D = E.shape
        dev = E.device
        gout, _ = rows2(gout.reshape(B, F * D), "InteractingLayer gradient")
        gE = torch.empty((B, F, D), dtype=torch.float32, device=dev)
        gWq, gWk, gWv = torch.empty_like(Wq), torch.empty_like(Wk), torch.empty_like(Wv)
        gWr = torch.empty_like(Wr) if has_res else None
        ws = workspace("dctr_interacting_bwd_workspace_floats", B, D, device=dev)
        call("dctr_interacting_bwd", ptr(E), lde, B, F, D, heads, int(scaling), ptr(Wq), ptr(Wk), ptr(Wv), ptr(Wr),
             ptr(gout), gout.stride(0), ptr(gE), F * D, ptr(gWq), ptr(gWk), ptr(gWv), ptr(gWr), ptr(ws),
             L.stream_handle(dev))
        return gE, gWq, gWk, gWv, gWr, None, None


def interacting_supported(F, D, H):
    return bool(L.lib().dctr_interacting_supported(int(F), int(D), int(H)))


DIN_ACT = {"linear": 0, "relu": 1, "sigmoid": 2, "prelu": 3, "dice": 4}     # include/dctr.h, dctr_din_attn_fwd


def din_attention_supported(T, dims, hidden, act):
    """True when csrc/din.hip runs this shape: E = sum(dims) <= 64, at most 4 segments, 1 <= T <= 128, 1 to 3 hidden
    layers of at most 128 units, ``act`` one of ``DIN_ACT``."""
    if act not in DIN_ACT or not dims or not hidden:
        return False
    return bool(L.lib().dctr_din_attn_supported(int(T), len(dims), i32s(dims), len(hidden), i32s(hidden), DIN_ACT[act]))



class DINAttentionFunction(torch.autograd.Function):
    """AttentionSequencePoolingLayer (csrc/din.hip): ``(Q [B, ld_q], K [B, ld_k] | None, params, segs, T, hidden, act,
    softmax, lengths [B] int32 | None, mask [B, T] uint8 | None, keep) -> [B, E]``.

    ``segs``: one ``(dim, q_off, k_off, k_step)`` per history feature: where its query and its first key start inside a
    row of Q / K and how far apart two positions lie.  ``K = None``: the keys lie in Q's rows (the model's gathered row) and
    ONE gradient row comes back.  ``params``: the packed vector the kernel reads (include/dctr.h).  ``keep``: a backward
    will follow, so the forward also writes the ``[B, T]`` weights; everything else is recomputed."""

    @staticmethod
    def forward(ctx, Q, K, params, segs, T, hidden, act, softmax, lengths, mask, keep):
        Q, ldq = rows2(Q, "DIN attention query")
        shared = K is None
        Kt, ldk = (Q, ldq) if shared else rows2(K, "DIN attention keys")
        B = Q.shape[0]
        P = params.detach().float().contiguous()
        dims, qo, ko, ks = zip(*segs)
        E = int(sum(dims))
        out = torch.empty((B, E), dtype=torch.float32, device=Q.device)
        wts = torch.empty((B, int(T)), dtype=torch.float32, device=Q.device) if keep else None
        cargs = (int(T), len(dims), i32s(dims), i64s(qo), i64s(ko), i64s(ks), ptr(lengths), ptr(mask), len(hidden),
                 i32s(hidden), DIN_ACT[act], int(bool(softmax)), ptr(P))
        call("dctr_din_attn_fwd", ptr(Q), ldq, ptr(Kt), ldk, B,
             *(cargs + (ptr(out), E, ptr(wts), L.stream_handle(Q.device))))
        if keep:
            ctx.save_for_backward(Q, Kt, P, wts, lengths, mask)
            ctx.cfg = (shared, tuple(segs), int(T), tuple(hidden), act, bool(softmax))
        return out

    @staticmethod
    def backward(ctx, gout):
        Q, Kt, P, wts, lengths, mask = ctx.saved_tensors
        shared, segs, T, hidden, act, softmax = ctx.cfg
        Q, ldq = rows2(Q, "DIN attention query")
        Kt, ldk = (Q, ldq) if shared else rows2(Kt, "DIN attention keys")
        B, dev = Q.shape[0], Q.device
        dims, qo, ko, ks = zip(*segs)
        gout, ldg = rows2(gout, "DIN attention gradient")
        # (zeros: the kernel writes the segments, whatever else the rows hold gets no gradient from here)
        gQ = torch.zeros(Q.shape, dtype=torch.float32, device=dev)
        gK = gQ if shared else torch.zeros(Kt.shape, dtype=torch.float32, device=dev)
        gP = torch.empty_like(P)
        ws = workspace("dctr_din_attn_bwd_workspace_floats", B, P.numel(), device=dev)
        call("dctr_din_attn_bwd", ptr(Q), ldq, ptr(Kt), ldk, B, T, len(dims), i32s(dims), i64s(qo), i64s(ko),
             i64s(ks), ptr(lengths), ptr(mask), len(hidden), i32s(hidden), DIN_ACT[act], int(softmax), ptr(P),
             ptr(wts), ptr(gout), ldg, ptr(gQ), gQ.shape[1], ptr(gK), gK.shape[1], ptr(gP), ptr(ws),
             L.stream_handle(dev))
        return gQ, (None if shared else gK), gP, None, None, None, None, None, None, None, None


GRU_MODE = {"GRU": 0, "AIGRU": 1, "AGRU": 2, "AUGRU": 3}                      # include/dctr.h, dctr_gru_seq_fwd


def gru_seq_supported(T, dims, mode="GRU"):
    """True when csrc/gru_seq.hip runs this shape: H = sum(dims) <= 64, at most 4 segments, 1 <= T <= 128."""
    if mode not in GRU_MODE or not dims:
        return False
    return bool(L.lib().dctr_gru_seq_supported(int(T), len(dims), i32s(dims), GRU_MODE[mode]))


class GRUSeqFunction(torch.autograd.Function):
    """The variable-length recurrences of DIEN (csrc/gru_seq.hip): ``(X [B, ld_x], att [B, T] | None, params, segs, T,
    mode, lengths [B] int32, want_states, want_last, keep) -> (states [B, T, H] | None, last [B, H] | None)``.

    ``segs``: one ``(dim, x_off, x_step)`` per segment of the input inside a row of X (the gathered row read in place, or
    ``[(H, 0, H)]`` for a contiguous ``[B, T*H]``).  ``params``: the packed ``W_ih | W_hh | b_ih | b_hh``.  ``keep``: a
    backward will follow, so the forward also writes the states (whether asked for or not) and the ``[B, T, 4, H]`` gates."""

    @staticmethod
    def forward(ctx, X, att, params, segs, T, mode, lengths, want_states, want_last, keep):
        X, ldx = rows2(X, "GRU input")
        B, dev = X.shape[0], X.device
        P = params.detach().float().contiguous()
        dims, xo, xs = zip(*segs)
        H, T = int(sum(dims)), int(T)
        A = att.detach().float().contiguous() if att is not None else None
        states = torch.empty((B, T, H), dtype=torch.float32, device=dev) if (want_states or keep) else None
        last = torch.empty((B, H), dtype=torch.float32, device=dev) if want_last else None
        gates = torch.empty((B, T, 4, H), dtype=torch.float32, device=dev) if keep else None
        call("dctr_gru_seq_fwd", ptr(X), ldx, B, T, len(dims), i32s(dims), i64s(xo), i64s(xs), ptr(lengths),
             ptr(A), GRU_MODE[mode], ptr(P), ptr(states), T * H, ptr(last), H, ptr(gates), L.stream_handle(dev))
        if keep:
            ctx.save_for_backward(X, A, P, lengths, states, gates)
            ctx.cfg = (tuple(segs), T, mode, bool(want_states), bool(want_last))
        return (states if want_states else None), last

    @staticmethod
    def backward(ctx, g_states, g_last):
        X, A, P, lengths, states, gates = ctx.saved_tensors
        segs, T, mode, want_states, want_last = ctx.cfg
        X, ldx = rows2(X, "GRU input")
        B, dev = X.shape[0], X.device
        dims, xo, xs = zip(*segs)
        H = int(sum(dims))
        gs = g_states.float().contiguous() if (want_states and g_states is not None) else None
        gl = g_last.float().contiguous() if (want_last and g_last is not None) else None
        if gs is None and gl is None:
            gl = torch.zeros((B, H), dtype=torch.float32, device=dev)
        # (zeros: the kernel writes the segments, whatever else the rows hold gets no gradient from here)
        gX = torch.zeros(X.shape, dtype=torch.float32, device=dev)
        gA = torch.empty((B, T), dtype=torch.float32, device=dev) if A is not None else None
        gP = torch.empty_like(P)
        ws = workspace("dctr_gru_seq_bwd_workspace_floats", B, H, device=dev)
        call("dctr_gru_seq_bwd", ptr(X), ldx, B, T, len(dims), i32s(dims), i64s(xo), i64s(xs), ptr(lengths),
             ptr(A), GRU_MODE[mode], ptr(P), ptr(states), T * H, ptr(gates), ptr(gs), T * H, ptr(gl), H, ptr(gX),
             gX.shape[1], ptr(gA), ptr(gP), ptr(ws), L.stream_handle(dev))
        return gX, gA, gP, None, None, None, None, None, None, None

