"""Gate mix of the multi-task models (models/multitask; csrc/gate_mix.hip)."""
import ctypes
import os

import torch

from .. import lib as L
from ..marshal import call, i32s, i64s, ptr, r4, rows2, workspace


class _MixMeta(object):
    """Static description of one gate-mix call (kept out of autograd's tensor arguments)."""

    def __init__(self, P, members, keep):
        self.P, self.members, self.keep = int(P), tuple(tuple(int(e) for e in m) for m in members), bool(keep)


def _mix_call(entry, xs, P, dim, B, gates, extra, dev):
    xp = (ctypes.c_void_p * P)(*[t.data_ptr() for t, _ in xs])
    call(entry, xp, i64s([ld for _, ld in xs]), P, dim, B, gates, len(gates), *extra, L.stream_handle(dev))


class GateMixFunction(torch.autograd.Function):
    """``(meta, x_0 .. x_{P-1}, h_0 .. h_{G-1}, W_0 .. W_{G-1}) -> (out_0 .. out_{G-1})``: every gate over one pool of
    expert outputs as one launch per direction (``dctr_gate_mix_fwd / _bwd``).  A gate whose output nothing used gets
    ``None`` for its input and weight gradients, as autograd leaves them in the reference."""

    @staticmethod
    def forward(ctx, meta, *tensors):
        P, G = meta.P, len(meta.members)
        xs = [rows2(t.detach(), "expert output") for t in tensors[:P]]
        hs = [rows2(t.detach(), "gate input") for t in tensors[P:P + G]]
        Ws = [rows2(t.detach(), "gate weight") for t in tensors[P + G:]]
        B, dim = xs[0][0].shape
        dev = xs[0][0].device
        ld_o = r4(dim)         # (a later tower reads the view in place: 16-byte rows)
        outs = [torch.empty((B, ld_o), dtype=torch.float32, device=dev) for _ in range(G)]
        ws = [torch.empty((B, len(m)), dtype=torch.float32, device=dev) if meta.keep else None for m in meta.members]
        gates = (L.Gate * G)()
        for g in range(G):
            (h, ldh), (W, ldw), q = hs[g], Ws[g], gates[g]
            q.h, q.ld_h, q.H = h.data_ptr(), ldh, h.shape[1]
            q.W, q.ld_w, q.n = W.data_ptr(), ldw, len(meta.members[g])
            q.out, q.ld_out = outs[g].data_ptr(), ld_o
            q.w = ws[g].data_ptr() if ws[g] is not None else None
            for j, e in enumerate(meta.members[g]):
                q.member[j] = e
        _mix_call("dctr_gate_mix_fwd", xs, P, dim, B, gates, (), dev)
        ctx.meta = meta
        if meta.keep:
            ctx.save_for_backward(*([t for t, _ in xs] + [t for t, _ in hs] + [t for t, _ in Ws] + ws))
        ctx.set_materialize_grads(False)
        return tuple(o[:, :dim] if ld_o != dim else o for o in outs)

    @staticmethod
    def backward(ctx, *gouts):
        meta = ctx.meta
        P, G = meta.P, len(meta.members)
        if all(g is None for g in gouts):
            return (None,) * (1 + P + 2 * G)
        saved = ctx.saved_tensors
        xs = [rows2(t, "expert output") for t in saved[:P]]
        hs = [rows2(t, "gate input") for t in saved[P:P + G]]
        Ws = [rows2(t, "gate weight") for t in saved[P + G:P + 2 * G]]
        ws = saved[P + 2 * G:]
        B, dim = xs[0][0].shape
        dev = xs[0][0].device
        gos = [None if g is None else rows2(g, "gate output gradient") for g in gouts]
        gxs = [torch.empty((B, dim), dtype=torch.float32, device=dev) for _ in range(P)]
        ghs = [torch.empty((B, h.shape[1]), dtype=torch.float32, device=dev) for h, _ in hs]
        gWs = [(torch.empty if B else torch.zeros)((W.shape[0], ldw), dtype=torch.float32, device=dev) for W, ldw in Ws]
        gates = (L.Gate * G)()
        for g in range(G):
            (h, ldh), (W, ldw), q = hs[g], Ws[g], gates[g]
            q.h, q.ld_h, q.H = h.data_ptr(), ldh, h.shape[1]
            q.W, q.ld_w, q.n = W.data_ptr(), ldw, len(meta.members[g])
            q.w = ws[g].data_ptr()
            if gos[g] is not None:
                q.g_out, q.ld_gout = gos[g][0].data_ptr(), gos[g][1]
            q.g_h, q.ld_gh, q.gW = ghs[g].data_ptr(), max(1, h.shape[1]), gWs[g].data_ptr()
            for j, e in enumerate(meta.members[g]):
                q.member[j] = e
        ns, lds = i32s([len(m) for m in meta.members]), i32s([ldw for _, ldw in Ws])
        work = workspace("dctr_gate_mix_bwd_workspace_floats", B, G, ns, lds, device=dev)
        gp = (ctypes.c_void_p * P)(*[t.data_ptr() for t in gxs])
        _mix_call("dctr_gate_mix_bwd", xs, P, dim, B, gates, (gp, i64s([dim] * P), ptr(work)), dev)
        live = [g is not None for g in gos]
        ret_h = [ghs[g] if live[g] else None for g in range(G)]
        ret_W = [(gWs[g][:, :Ws[g][0].shape[1]] if Ws[g][1] != Ws[g][0].shape[1] else gWs[g]) if live[g] else None
                 for g in range(G)]
        return (None,) + tuple(gxs) + tuple(ret_h) + tuple(ret_W)


def gate_mix_torch(experts, gate_inputs, gate_weights, members):
    """The reference's formulation as torch ops: Linear -> softmax -> stack -> matmul per gate."""
    outs = []
    for h, W, m in zip(gate_inputs, gate_weights, members):
        w = torch.nn.functional.linear(h, W).softmax(1)
        outs.append(torch.matmul(w.unsqueeze(1), torch.stack([experts[e] for e in m], 1)).squeeze(1))
    return outs


def gate_mix_fused(experts, gate_inputs, gate_weights, members):
    """True when ``gate_mix`` takes csrc/gate_mix.hip for these operands: the switch DCTR_GATE_MIX is not ``0``, everything
    is a 2-D float32 tensor on the GPU, and the shape lies inside the kernels' envelope (include/dctr.h: at most 32 pool
    members, 8 gates, 16 members per gate, ``dim`` and every ``H`` at most 1152)."""
    if os.environ.get("DCTR_GATE_MIX", "1") == "0":
        return False
    ts = list(experts) + list(gate_inputs) + list(gate_weights)
    if not ts or any(t.dim() != 2 or t.dtype != torch.float32 or not t.is_cuda for t in ts):
        return False
    G = len(members)
    if G == 0 or any(len(m) == 0 for m in members):
        return False
    if G > L.GATE_MAX_GATES or len(experts) > L.GATE_MAX_POOL:      # (the host arrays below hold no more)
        return False
    return bool(L.lib().dctr_gate_mix_supported(len(experts), experts[0].shape[1], G, i32s([len(m) for m in members]),
                                                i32s([h.shape[1] for h in gate_inputs])))


def gate_mix(experts, gate_inputs, gate_weights, members):
    """Every gate that draws on one pool of expert outputs -- all gates of an MMOE, one CGC level of a PLE:
    ``out_g = sum_j softmax(h_g W_g^T)[:, j] * experts[members[g][j]]`` as a list of G ``[B, dim]`` tensors.
    ``experts``: P tensors ``[B, dim]``; ``gate_inputs[g]``: ``[B, H_g]``; ``gate_weights[g]``: ``[n_g, H_g]`` (bias-free);
    ``members[g]``: n_g indices into ``experts`` in the order of the reference's ``torch.stack``.  Row-strided views (what
    ``_hip.mlp.tower(dnn, None, x)`` returns) are read in place.  One launch per direction (csrc/gate_mix.hip) inside
    the envelope; outside it, or with ``DCTR_GATE_MIX=0``, the same formula as torch ops on the GPU."""
    experts, gate_inputs, gate_weights = list(experts), list(gate_inputs), list(gate_weights)
    members = [tuple(int(e) for e in m) for m in members]
    if not (len(gate_inputs) == len(gate_weights) == len(members)):
        raise ValueError("gate_mix: one input, one weight and one member list per gate")
    for m, W, h in zip(members, gate_weights, gate_inputs):
        if W.shape[0] != len(m) or W.shape[1] != h.shape[1] or any(e < 0 or e >= len(experts) for e in m):
            raise ValueError("gate_mix: a gate's weight must be [len(members), H] over members inside the pool")
    L.require_gpu(experts[0], "expert output")
    if not gate_mix_fused(experts, gate_inputs, gate_weights, members):
        return gate_mix_torch(experts, gate_inputs, gate_weights, members)
    ts = experts + gate_inputs + gate_weights
    keep = torch.is_grad_enabled() and any(t.requires_grad for t in ts)
    return list(GateMixFunction.apply(_MixMeta(len(experts), members, keep), *ts))
