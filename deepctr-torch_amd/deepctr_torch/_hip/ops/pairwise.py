"""Pairwise field interactions: SENET, the bilinear and inner products of FiBiNET / PNN (csrc/pairwise.hip)."""
import os

import torch

from .. import lib as L
from ..marshal import call, ptr, rows2, rows3, workspace


class SENETFunction(torch.autograd.Function):
    """V = E * relu(W2 relu(W1 mean_d(E)))  (interaction.py:93-101)."""

    @staticmethod
    def forward(ctx, E, W1, W2):
        E, lde = rows3(E, "SENET input")
        B, F, D = E.shape
        R = W1.shape[0]
        W1, W2 = W1.contiguous(), W2.contiguous()
        V = torch.empty((B, F, D), dtype=torch.float32, device=E.device)
        a = torch.empty((B, F), dtype=torch.float32, device=E.device)
        a1 = torch.empty((B, R), dtype=torch.float32, device=E.device)
        call("dctr_senet_fwd", ptr(E), lde, B, F, D, ptr(W1), ptr(W2), R, ptr(V), ptr(a), ptr(a1),
             L.stream_handle(E.device))
        ctx.save_for_backward(E, W1, W2, a, a1)
        return V

    @staticmethod
    def backward(ctx, gV):
        E, W1, W2, a, a1 = ctx.saved_tensors
        E, lde = rows3(E, "SENET input")
        B, F, D = E.shape
        R = W1.shape[0]
        gV = gV.contiguous().float()
        gE = torch.empty((B, F, D), dtype=torch.float32, device=E.device)
        gW1, gW2 = torch.empty_like(W1), torch.empty_like(W2)
        ws = workspace("dctr_senet_bwd_workspace_floats", B, F, R, device=E.device)
        call("dctr_senet_bwd", ptr(gV), ptr(E), lde, B, F, D, ptr(W1), ptr(W2), R, ptr(a), ptr(a1), ptr(gE),
             ptr(gW1), ptr(gW2), ptr(ws), L.stream_handle(E.device))
        return gE, gW1, gW2


def tournament_schedule(F, bilinear_type):
    """Pairs (i < j) of F fields in round-robin-tournament order: every round is a perfect matching, so workers
    handling different slots of a round never share a field.  Returns (rows [n, 4] = {i, j, w, k}, slots per round,
    pair_w [P], n_w).  k is the reference's pair index (itertools.combinations order)."""
    n = F + (F & 1)
    ring = list(range(n))
    rows = []
    for _ in range(n - 1):
        for s in range(n // 2):
            a, b = ring[s], ring[n - 1 - s]
            i, j = min(a, b), max(a, b)
            if j >= F:       # the dummy of an odd field count: idle slot
                rows.append((-1, -1, 0, 0))
                continue
            k = i * F - i * (i + 1) // 2 + (j - i - 1)
            w = 0 if bilinear_type == "all" else (i if bilinear_type == "each" else k)
            rows.append((i, j, w, k))
        ring = [ring[0]] + [ring[-1]] + ring[1:-1]
    P = F * (F - 1) // 2
    pair_w = [0] * P
    for (i, j, w, k) in rows:
        if i >= 0:
            pair_w[k] = w
    n_w = 1 if bilinear_type == "all" else (F if bilinear_type == "each" else P)
    return rows, n // 2, pair_w, n_w


def disjoint_groups(rows, width=8):
    """The pairs of a tournament schedule re-dealt in groups of ``width`` field-disjoint pairs (one per wave of a
    workgroup, a barrier per group): ``[n_groups][width][4]`` rows ``{i, j, w, k}``, ``i = -1`` for an idle entry.
    Greedy over the tournament order -- a round is a perfect matching, so only groups that straddle two rounds have to
    look ahead; deterministic."""
    rest = [r for r in rows if r[0] >= 0]
    groups = []
    while rest:
        used, grp, keep = set(), [], []
        for r in rest:
            if len(grp) < width and r[0] not in used and r[1] not in used:
                grp.append(r)
                used.update((r[0], r[1]))
            else:
                keep.append(r)
        rest = keep
        groups.append(grp + [(-1, -1, 0, 0)] * (width - len(grp)))
    return groups


def slab_ld(width):
    """Row stride (floats) of a wide [B, width] slab whose rows should start on 128-byte lines (DCTR_SLAB_ALIGN=0: dense)."""
    if os.environ.get("DCTR_SLAB_ALIGN", "1") == "0" or width < 1024:
        return int(width)
    return (int(width) + 31) // 32 * 32


class BilinearFunction(torch.autograd.Function):
    """(x_i W^T) * x_j for every pair, on E and optionally on a second input V with the same weights; the result is
    written in the DNN-input layout ``[V pairs | E pairs | dense]`` (fibinet.py:82-87)."""

    @staticmethod
    def forward(ctx, meta, E, V, dense, *weights):
        E, lde = rows3(E, "Bilinear input")
        B, F, D = E.shape
        if D > 16:
            raise NotImplementedError("the gfx950 bilinear kernels support embedding_dim <= 16 (got %d)" % D)
        ldv = 0
        if V is not None:
            V, ldv = rows3(V, "Bilinear second input")
        Wf = meta.flat_weights(weights)
        P = F * (F - 1) // 2
        npass = 2 if V is not None else 1
        n_dense = dense.shape[1] if dense is not None else 0
        if dense is not None:
            dense, _ = rows2(dense, "Bilinear dense input")
        width = npass * P * D + n_dense
        # rows of the product slab start on a 128-byte line (round 6): a pair's D floats per sample are one 64-byte piece, and
        # with rows of 10 413 floats (41 652 bytes) every piece straddled two lines -- twice the memory requests in this
        # kernel's stores and in the backward kernels' reads of the gradient slab (mlp.WideLinearFunction returns it with the
        # same row stride).  The GEMMs behind take the view with its leading dimension.
        ld_out = slab_ld(width)
        out = torch.empty((B, ld_out), dtype=torch.float32, device=E.device)[:, :width]
        sched = meta.device_tables(E.device)
        call("dctr_bilinear_fwd", ptr(E), lde, ptr(V), ldv, ptr(Wf), ptr(sched[2]), sched[2].shape[0], P, F, D, B,
             ptr(out), ld_out, ptr(dense), dense.stride(0) if dense is not None else 0, n_dense, npass * P * D,
             L.stream_handle(E.device))
        ctx.meta, ctx.n_w_in = meta, len(weights)
        ctx.has_v, ctx.has_dense = V is not None, dense is not None
        ctx.save_for_backward(E, V, Wf)
        return out

    @staticmethod
    def backward(ctx, gout):
        meta = ctx.meta
        E, V, Wf = ctx.saved_tensors
        E, lde = rows3(E, "Bilinear input")
        B, F, D = E.shape
        ldv = 0
        if V is not None:
            V, ldv = rows3(V, "Bilinear second input")
        P = F * (F - 1) // 2
        npass = 2 if V is not None else 1
        gout, _ = rows2(gout, "Bilinear gradient")
        dev = E.device
        gE = torch.empty((B, F, D), dtype=torch.float32, device=dev)
        gV = torch.empty((B, F, D), dtype=torch.float32, device=dev) if V is not None else None
        gW = torch.empty((meta.n_w, D, D), dtype=torch.float32, device=dev)
        ws = workspace("dctr_bilinear_bwd_workspace_floats", B, P, D, device=dev)
        sched = meta.device_tables(dev)
        call("dctr_bilinear_bwd", ptr(E), lde, ptr(V), ldv, ptr(Wf), ptr(sched[0]), meta.n_sched, meta.slots,
             ptr(sched[1]), meta.n_w, P, F, D, B, ptr(gout), gout.stride(0), ptr(gE), ptr(gV), ptr(gW), ptr(ws),
             ptr(sched[2]), sched[2].shape[0], L.stream_handle(dev))
        g_dense = gout[:, npass * P * D:] if ctx.has_dense else None
        return (None, gE, gV, g_dense) + tuple(gW[i] for i in range(ctx.n_w_in))


class BilinearStackedFunction(torch.autograd.Function):
    """``(x_i W_k^T) * x_j`` for every pair k with the weights given as ONE ``[n_w, D, D]`` tensor (no per-weight
    parameters to re-seat): the bilinear kernels of csrc/pairwise.hip behind OutterProductLayer's 'mat' kernel."""

    @staticmethod
    def forward(ctx, meta, E, Wf):
        E, lde = rows3(E, "pairwise input")
        B, F, D = E.shape
        if D > 16:
            raise NotImplementedError("the gfx950 bilinear kernels support embedding_dim <= 16 (got %d)" % D)
        Wf = Wf.detach().float().contiguous()
        P = F * (F - 1) // 2
        out = torch.empty((B, P * D), dtype=torch.float32, device=E.device)
        sched = meta.device_tables(E.device)
        call("dctr_bilinear_fwd", ptr(E), lde, None, 0, ptr(Wf), ptr(sched[2]), sched[2].shape[0], P, F, D, B,
             ptr(out), P * D, None, 0, 0, P * D, L.stream_handle(E.device))
        ctx.meta = meta
        ctx.save_for_backward(E, Wf)
        return out

    @staticmethod
    def backward(ctx, gout):
        meta = ctx.meta
        E, Wf = ctx.saved_tensors
        E, lde = rows3(E, "pairwise input")
        B, F, D = E.shape
        P = F * (F - 1) // 2
        gout, _ = rows2(gout, "Bilinear gradient")
        dev = E.device
        gE = torch.empty((B, F, D), dtype=torch.float32, device=dev)
        gW = torch.empty((meta.n_w, D, D), dtype=torch.float32, device=dev)
        ws = workspace("dctr_bilinear_bwd_workspace_floats", B, P, D, device=dev)
        sched = meta.device_tables(dev)
        call("dctr_bilinear_bwd", ptr(E), lde, None, 0, ptr(Wf), ptr(sched[0]), meta.n_sched, meta.slots,
             ptr(sched[1]), meta.n_w, P, F, D, B, ptr(gout), gout.stride(0), ptr(gE), None, ptr(gW), ptr(ws),
             ptr(sched[2]), sched[2].shape[0], L.stream_handle(dev))
        return None, gE, gW


class BilinearMeta(object):
    """Host-side tables of a BilinearInteraction layer: the tournament schedule and the flat weight slab."""

    def __init__(self, F, bilinear_type):
        rows, self.slots, pair_w, self.n_w = tournament_schedule(F, bilinear_type)
        self.n_sched = len(rows)
        self._rows, self._pair_w = rows, pair_w
        self._dev = None
        self._slab = None

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_dev"] = None
        d["_slab"] = None
        d["_wide"] = None
        return d

    def device_tables(self, device):
        if self._dev is None or self._dev[0].device != torch.device(device):
            # [2]: the forward's order -- by output position k: the four waves of a workgroup then write neighbouring
            # 64-byte pieces of a sample's row at about the same time, and L2 evicts whole lines (the tournament order
            # scattered them: measured 126 us for the 170 MB of FiBiNET's DNN input at the Criteo shape)
            by_k = sorted((r for r in self._rows if r[0] >= 0), key=lambda r: r[3])
            self._dev = (torch.tensor(self._rows, dtype=torch.int32, device=device).reshape(-1, 4).contiguous(),
                         torch.tensor(self._pair_w, dtype=torch.int32, device=device),
                         torch.tensor(by_k, dtype=torch.int32, device=device).reshape(-1, 4).contiguous())
        return self._dev

    def wide_tables(self, device):
        """(groups ``[n_groups, 8, 4]`` int32, pair_w) on ``device`` for dctr_bilinear_wide_bwd."""
        dev = getattr(self, "_wide", None)
        if dev is None or dev[0].device != torch.device(device):
            groups = disjoint_groups(self._rows)
            self._wide = (torch.tensor(groups, dtype=torch.int32, device=device).reshape(-1, 8, 4).contiguous(),
                          self.device_tables(device)[1])
        return self._wide

    def flat_weights(self, weights):
        """``[n_w, D, D]`` slab holding the layer's nn.Linear weights.  The parameters are re-seated ONCE as slices of
        one contiguous slab (values preserved), after which this is a pointer check; the slab pointer stays stable
        (hipGraph-safe) until someone re-allocates the parameters (``.to()``), which is detected here."""
        slab = self._slab
        D = weights[0].shape[0]
        step = D * D * 4
        if slab is not None and slab.shape[0] == len(weights) and slab.device == weights[0].device and \
                all(w.data_ptr() == slab.data_ptr() + i * step for i, w in enumerate(weights)):
            return slab
        slab = torch.stack([w.detach() for w in weights]).contiguous()
        for i, w in enumerate(weights):
            w.data = slab[i]
        self._slab = slab
        return slab


class InnerProductFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, E, reduce_sum):
        E, lde = rows3(E, "InnerProduct input")
        B, F, D = E.shape
        P = F * (F - 1) // 2
        per = 1 if reduce_sum else D
        out = torch.empty((B, P, per), dtype=torch.float32, device=E.device)
        if P > 0:
            call("dctr_inner_product_fwd", ptr(E), lde, B, F, D, int(bool(reduce_sum)), ptr(out), P * per,
                 L.stream_handle(E.device))
        ctx.reduce_sum = bool(reduce_sum)
        ctx.save_for_backward(E)
        return out

    @staticmethod
    def backward(ctx, gp):
        (E,) = ctx.saved_tensors
        E, lde = rows3(E, "InnerProduct input")
        B, F, D = E.shape
        P = F * (F - 1) // 2
        per = 1 if ctx.reduce_sum else D
        gp = gp.contiguous().float()
        gE = torch.zeros((B, F, D), dtype=torch.float32, device=E.device)
        if P > 0:
            call("dctr_inner_product_bwd", ptr(E), lde, B, F, D, int(ctx.reduce_sum), ptr(gp), P * per, ptr(gE),
                 F * D, L.stream_handle(E.device))
        return gE, None

