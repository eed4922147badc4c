"""MLR's piece-wise linear mixture over a wide-only per-field plan whose wide side spans several ``Linear`` modules
(``EmbeddingPlan(wide_sides=...)``; csrc/mlr.hip, include/dctr.h ``dctr_mlr_fwd`` / ``dctr_mlr_bwd``).

``MLRHeads`` is the host mirror of ``dctr_mlr_t``; ``MLRFunction`` the one autograd node of the fused route: the forward is
one launch, the backward one launch (+ a fixed-order reduce) that writes the per-field ``g_wide`` rows and the dense-weight
gradients, then the table update ``plan.update`` selects -- exactly what ``EmbedFunction.backward`` does with its rows.
``mlr_composed`` is the other route (``DCTR_MLR=0``, and plans outside the kernel's envelope): ONE per-field gather through
``dctr_embed_fwd`` on the same plan, then the reference's operations as torch ops."""
import ctypes
import os

import numpy as np
import torch

from .. import lib as L
from ..marshal import call, ptr, rows2
from .embed import _update_tables, embed


class MLRHeads(object):
    """``dctr_mlr_t`` of a plan built with ``wide_sides``: heads 0 .. R - 1 are the regions, head R (``has_bias``) the bias.
    ``weights[h]``: head h's ``Linear.weight`` ([n, 1]) or None when the head has no dense columns."""

    def __init__(self, plan, weights, n_regions, has_bias, task):
        if plan.head_of is None or len(plan.side_dense_cols) != n_regions + int(bool(has_bias)):
            raise ValueError("MLRHeads needs a plan built with wide_sides, one side per head")
        self.plan, self.weights = plan, list(weights)
        self.n_regions, self.has_bias = int(n_regions), bool(has_bias)
        self.task = {"binary": L.MLR_BINARY, "regression": L.MLR_REGRESSION}[task]
        self.n_heads = self.n_regions + int(self.has_bias)
        self.dense_cols = [list(c) for c in plan.side_dense_cols]
        for h, cols in enumerate(self.dense_cols):
            w = self.weights[h]
            if bool(cols) != (w is not None) or (w is not None and w.numel() != len(cols)):
                raise ValueError("head %d: %d dense columns do not match its Linear.weight" % (h, len(cols)))
        self.dense_off = [0]
        for cols in self.dense_cols:
            self.dense_off.append(self.dense_off[-1] + len(cols))
        self.n_dense = self.dense_off[-1]
        self._reset()

    def _reset(self):
        self._key, self._dev, self.c = None, {}, L.Mlr()

    def __getstate__(self):
        d = dict(self.__dict__)
        for k in ("_key", "_dev", "c"):
            d.pop(k, None)
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)
        self._reset()

    def dense_params(self):
        return [w for w in self.weights if w is not None]

    def bind(self, device):
        """``ctypes.byref(dctr_mlr_t)`` valid for the weights' CURRENT device pointers."""
        device = torch.device(device)
        key = (str(device),) + tuple(w.data_ptr() if w is not None else 0 for w in self.weights)
        if key != self._key:
            for w in self.dense_params():
                L.require_gpu(w, "Linear.weight")
                if w.dtype != torch.float32 or not w.is_contiguous():
                    raise RuntimeError("Linear.weight must be contiguous float32")

            def up(values, dtype):
                return torch.from_numpy(np.asarray(values or [0], dtype=dtype)).to(device)
            flat = [c for cols in self.dense_cols for c in cols]
            self._dev = {"head_of": up(self.plan.head_of, np.int32), "cols": up(flat, np.int32),
                         "off": up(self.dense_off, np.int32), "w": up(list(key[1:]), np.int64)}
            c = self.c
            c.head_of, c.dense_cols = self._dev["head_of"].data_ptr(), self._dev["cols"].data_ptr()
            c.dense_off, c.dense_w = self._dev["off"].data_ptr(), self._dev["w"].data_ptr()
            c.n_regions, c.has_bias, c.task, c.n_dense = self.n_regions, int(self.has_bias), self.task, self.n_dense
            self._key = key
        return ctypes.byref(self.c)

    def supported(self, device):
        return bool(L.lib().dctr_mlr_supported(self.plan.bind(device), self.bind(device)))


class MLRFunction(torch.autograd.Function):
    """``y [B]`` of the mixture for model input ``X``: ``dctr_mlr_fwd``; the backward runs ``dctr_mlr_bwd`` and hands the
    per-field ``g_wide`` to the plan's table update.  The heads' dense weights enter as inputs (``*weights``, the non-None
    entries of ``heads.weights`` in head order) so that autograd gets their gradients; the tables never do."""

    @staticmethod
    def forward(ctx, plan, heads, X, anchor, for_backward, *weights):
        X, _ = rows2(X, "model input X")
        if X.shape[1] < plan.n_xcols:
            raise ValueError("X has %d columns, the feature columns need %d" % (X.shape[1], plan.n_xcols))
        B = X.shape[0]
        cplan, cmlr = plan.bind(X.device), heads.bind(X.device)
        lazy = plan.lazy if plan.update[0] == "lazy" else None
        if lazy is not None:
            if for_backward and lazy.plan is plan:
                lazy.catchup(X)
            else:
                lazy.flush()
        ids_t = parts_t = den_t = amax = None
        ctx.seg_event = None
        stream = L.stream_handle(X.device)
        if for_backward and plan.table_params and plan.update_kernel_ok(B):
            ids_t = torch.empty((plan.n_vcols, B), dtype=torch.int32, device=X.device)
            parts_t = torch.empty((plan.n_vcols, B), dtype=torch.int16, device=X.device)
            den_t, amax = plan.step_buffers(B, X.device)
        plan.point_step_buffers(den_t, amax)
        fused_ids = ids_t is not None and plan.gen is None     # (a general unit spans several X columns: dctr_embed_ids)
        if ids_t is not None and not fused_ids:
            call("dctr_embed_ids", cplan, plan.units_ptr(), plan.n_grid_units, ptr(X), X.stride(0), B, ptr(ids_t),
                 ptr(parts_t), stream)
        y = torch.empty((B,), dtype=torch.float32, device=X.device)
        z = torch.empty((B, heads.n_heads), dtype=torch.float32, device=X.device)
        err = plan.err_flag(X.device)
        call("dctr_mlr_fwd", cplan, cmlr, ptr(X), X.stride(0), B, ptr(y), ptr(z), z.stride(0), ptr(err),
             ptr(ids_t) if fused_ids else None, ptr(parts_t) if fused_ids else None, plan.units_ptr(),
             plan.n_grid_units, stream)
        if ids_t is not None and plan.segments_enabled():
            ctx.seg_event = plan.launch_segments(ids_t, parts_t, B)
        ctx.plan, ctx.heads = plan, heads
        ctx.save_for_backward(X, z, ids_t, parts_t, den_t, amax)
        ctx.set_materialize_grads(False)
        return y

    @staticmethod
    def backward(ctx, g_y):
        plan, heads = ctx.plan, ctx.heads
        X, z, ids_t, parts_t, den_t, amax = ctx.saved_tensors
        none = (None,) * (5 + len(heads.dense_params()))
        if g_y is None:
            return none
        B = X.shape[0]
        plan.point_step_buffers(den_t, amax)
        g_y = g_y.reshape(B).float().contiguous()
        g_wide = torch.empty((B, plan.ld_wide), dtype=torch.float32, device=X.device) if plan.wide else None
        g_dense = torch.empty((heads.n_dense,), dtype=torch.float32, device=X.device) if heads.n_dense else None
        ws = None
        if heads.n_dense:
            n = int(L.lib().dctr_mlr_bwd_workspace_floats(heads.bind(X.device), B))
            ws = torch.empty((max(n, 1),), dtype=torch.float32, device=X.device)
        call("dctr_mlr_bwd", plan.bind(X.device), heads.bind(X.device), ptr(X), X.stride(0), B, ptr(g_y), ptr(z),
             z.stride(0), ptr(g_wide), plan.ld_wide, ptr(g_dense), ptr(ws), L.stream_handle(X.device))
        if g_wide is not None and plan.table_params:
            _update_tables(plan, X, ids_t, parts_t, ctx.seg_event, None, 0, None, None, None, g_wide, None, None, den_t,
                           amax)
        grads = []
        for h, w in enumerate(heads.weights):
            if w is not None:
                grads.append(g_dense[heads.dense_off[h]:heads.dense_off[h + 1]].reshape(w.shape))
        return (None, None, None, None, None) + tuple(grads)


def mlr_route():
    """"fused" (csrc/mlr.hip) unless ``DCTR_MLR=0`` selects the composed route."""
    return "composed" if os.environ.get("DCTR_MLR", "1") == "0" else "fused"


def _select(heads, device, key):
    """per head: the LongTensor of its wide fields' columns in the per-field ``wide`` buffer (``key`` "select") or of its
    dense features' columns in X ("dense"); cached on ``heads``"""
    hit = heads._dev.get(key)
    if hit is None:
        lists = [[f for f, hf in enumerate(heads.plan.head_of) if hf == h] for h in range(heads.n_heads)] \
            if key == "select" else heads.dense_cols
        hit = heads._dev[key] = [torch.tensor(v, dtype=torch.long, device=device) for v in lists]
    return hit


def mlr_composed(plan, heads, X):
    """The mixture as the reference composes it, over ONE per-field gather on the same plan: per-head sums of the gathered
    first-order weights (``head_of``), the dense halves as ``X_dense @ weight``, then softmax, sigmoid, mul and sum.  The
    tables are updated by the gather's own backward (``EmbedFunction``)."""
    B = X.shape[0]
    heads.bind(X.device)
    wide = embed(plan, X)[1] if plan.wide else None          # [B, n_wide + 1]
    cols = _select(heads, X.device, "select")
    zs = []
    for h in range(heads.n_heads):
        zh = torch.zeros((B, 1), dtype=torch.float32, device=X.device)
        if cols[h].numel():
            zh = zh + wide.index_select(1, cols[h]).sum(dim=1, keepdim=True)
        if heads.weights[h] is not None:
            dc = heads.dense_cols[h]
            xd = X[:, dc[0]:dc[-1] + 1] if dc == list(range(dc[0], dc[-1] + 1)) else \
                X.index_select(1, _select(heads, X.device, "dense")[h])
            zh = zh + xd.matmul(heads.weights[h])
        zs.append(zh)
    R = heads.n_regions
    region = torch.cat(zs[:R], dim=-1)
    learner = torch.sigmoid(region) if heads.task == L.MLR_BINARY else region
    y = torch.sum(torch.softmax(region, dim=-1) * learner, dim=-1)
    if heads.has_bias:
        y = y * torch.sigmoid(zs[R]).squeeze(1)
    return y


def mlr(plan, heads, X):
    """``y [B]``: the fused kernels when the route is "fused" and they take this plan, else the composed route."""
    L.require_gpu(X, "model input X")
    if getattr(plan, "sharder", None) is not None or getattr(plan, "exchange", None) is not None:
        raise NotImplementedError("the piece-wise linear mixture (MLR) is not wired into the multi-GPU trainers")
    plan.bind(X.device)
    if mlr_route() == "fused" and heads.supported(X.device):
        return MLRFunction.apply(plan, heads, X, plan.anchor, torch.is_grad_enabled(), *heads.dense_params())
    return mlr_composed(plan, heads, X)
