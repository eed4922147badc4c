"""The fused lookup and its table update (csrc/embed.hip, pair_embed.hip, update.hip, lazy.hip).

Embedding tables never enter autograd as inputs: the reference's dense ``[V, D]`` gradient
(``aten::embedding_dense_backward``, triggered from basemodel.py:261) is replaced by an O(batch)
scatter executed inside ``EmbedFunction.backward``.  What that scatter does is selected by
``plan.update``:

  ``("dense",)``            add the row gradients into the table's zero-at-rest ``gacc`` slab and expose
                            it as ``param.grad`` -- bit-for-bit the tensor the reference hands to ANY
                            optimizer / regulariser (default; O(V) only if the optimizer is).
  ``("sgd", lr)``           ``table[row] -= lr * g`` straight from the scatter kernel.
  ``("adagrad", lr, eps)``  scatter into ``gacc``, then ``dctr_embed_apply`` consumes the touched rows.
"""
import contextlib
import ctypes
import os

import torch

from .. import lib as L
from ..marshal import call, padded_rows, ptr, r4, rows2
from ..plan import EmbeddingPlan


class EmbedFunction(torch.autograd.Function):
    """Fused lookup: see ``dctr_embed_fwd`` / ``dctr_embed_bwd`` in include/dctr.h."""

    @staticmethod
    def forward(ctx, plan, X, anchor, wdense_w, want_fm, for_backward=False):
        X, _ = rows2(X, "model input X")
        if X.shape[1] < plan.n_xcols:
            raise ValueError("X has %d columns, the feature columns need %d" % (X.shape[1], plan.n_xcols))
        B = X.shape[0]
        cplan = plan.bind(X.device)
        out = torch.empty((B, plan.ld_out), dtype=torch.float32, device=X.device) if plan.has_lookup else None
        # (a per-field-wide plan: [B, ld_wide] -- column f = wide field f, the last column the dense half of Linear)
        wide = torch.empty((B, plan.ld_wide) if plan.wide_per_field else (B,), dtype=torch.float32,
                           device=X.device) if plan.has_wide else None
        fm = torch.empty((B,), dtype=torch.float32, device=X.device) if want_fm else None
        if want_fm and (plan.emb_dim <= 0 or not plan.deep):
            raise ValueError("FM needs sparse features that share one embedding_dim")
        # exact lazy regularised / Adam update (csrc/lazy.hip): a training gather first replays the batch's rows to
        # the current step; any other reader of the tables gets them flushed
        lazy = plan.lazy if plan.update[0] == "lazy" else None
        if lazy is not None:
            if for_backward and lazy.plan is plan:
                lazy.catchup(X)
            else:
                lazy.flush()
        # side outputs for the deterministic fused update (only when a backward can follow)
        ids_t = parts_t = fm_s = den_t = amax = None
        ld_s = 0
        if for_backward and plan.table_params and plan.update_kernel_ok(B):
            ids_t = torch.empty((plan.n_vcols, B), dtype=torch.int32, device=X.device)
            # each entry's partition of the update kernel (a 16-bit tag: its workgroups compare instead of dividing)
            parts_t = torch.empty((plan.n_vcols, B), dtype=torch.int16, device=X.device)
            if want_fm:
                ld_s = r4(plan.emb_dim)
                fm_s = torch.empty((B, ld_s), dtype=torch.float32, device=X.device)
            # general units (pooled VarLen fields, shared tables): mean pooling's divisors (written with the ids) and
            # max pooling's arg-max positions (written by the gather) are this step's side buffers
            den_t, amax = plan.step_buffers(B, X.device)
        plan.point_step_buffers(den_t, amax)
        # The part of the update that needs only the ids -- finding and sorting every partition's entries -- runs on a
        # side stream, under the tower.  In the fused train step with in-kernel optimizer that stream also computes the
        # ids itself (from X, ahead of the gather) and later runs the update: its chain then waits for the main
        # stream once (for the tower's gradients) and the main chain -- gather, tower, weight gradients -- for nothing.
        sink = getattr(plan, "dense_sink", None)
        segs = ids_t is not None and plan.segments_enabled() and getattr(plan, "exchange", None) is None
        own_ids = segs and X.is_cuda and sink is not None and getattr(sink, "inline", None) is not None
        ctx.seg_event = None
        err = plan.err_flag(X.device)

        def gather(stream, with_ids):
            fused_ids = with_ids and plan.gen is None      # (a general unit spans several X columns: dctr_embed_ids)
            call("dctr_embed_fwd", cplan, ptr(X), X.stride(0), B, ptr(out), plan.ld_out, ptr(wide), plan.ld_wide,
                 ptr(fm), ptr(err), plan.units_ptr(), plan.n_grid_units, ptr(ids_t) if fused_ids else None,
                 ptr(parts_t) if fused_ids else None, ptr(fm_s), ld_s, stream)
            if with_ids and not fused_ids and ids_t is not None:
                call("dctr_embed_ids", cplan, plan.units_ptr(), plan.n_grid_units, ptr(X), X.stride(0), B, ptr(ids_t),
                     ptr(parts_t), stream)

        if own_ids:
            ctx.seg_event = plan.launch_segments(ids_t, parts_t, B, X=X)
            if ctx.seg_event[0] is not True:              # (True: the CPU stand-in, no streams)
                sink.update_stream = ctx.seg_event[0]     # where this step's update will run (see backward)
        gather(L.stream_handle(X.device), not own_ids)
        ctx.plan, ctx.want_fm = plan, want_fm
        if segs and not own_ids:
            ctx.seg_event = plan.launch_segments(ids_t, parts_t, B)
        ctx.save_for_backward(X, out if (want_fm or plan.gen is not None) else None, ids_t, fm_s, parts_t, den_t, amax)
        ctx.set_materialize_grads(False)
        outs = (out if out is not None else X.new_zeros((B, 0)),
                wide if wide is not None else X.new_zeros((B, plan.ld_wide) if plan.wide_per_field else (B,)),
                fm if fm is not None else X.new_zeros((B,)))
        return outs

    @staticmethod
    def backward(ctx, g_out, g_wide, g_fm):
        plan = ctx.plan
        X, out, ids_t, fm_s, parts_t, den_t, amax = ctx.saved_tensors
        plan.point_step_buffers(den_t, amax)
        if not plan.has_lookup:
            g_out = None
        if not plan.has_wide:
            g_wide = None
        if not ctx.want_fm:
            g_fm = None
        g_wide, g_wd, g_w = _wide_dense_grad(plan, X, g_wide, ids_t, ctx.needs_input_grad[3])
        if g_fm is not None:
            g_fm = g_fm.contiguous()
        ld_g = 0
        if g_out is not None:
            g_out, ld_g = padded_rows(g_out, 0, plan.vec)
        if (g_out is None and g_fm is None and g_wide is None) or not plan.table_params:
            return None, None, None, g_w, None, None
        _update_tables(plan, X, ids_t, parts_t, ctx.seg_event, g_out, ld_g, out, fm_s, g_fm, g_wide, g_wd, g_w, den_t, amax)
        return None, None, None, g_w, None, None


def _wide_dense_grad(plan, X, g_wide, ids_t, need_w):
    """The ``Linear.weight`` side of a lookup's backward: ``(g_wide contiguous | None, g_wd, g_w)`` -- ``g_wd`` is the buffer
    the deterministic update kernel writes the gradient into (None: it does not), ``g_w`` what autograd gets."""
    g_wd = None
    g_w = None
    if g_wide is not None:
        g_wide = g_wide.contiguous()
        if plan.wide_dense_weight is not None and need_w:
            # d wide / d Linear.weight = X_dense^T g  (basemodel.py:88-90): an extra workgroup of the
            # deterministic update kernel when that runs, else a GEMV
            if ids_t is not None and getattr(plan, "exchange", None) is None and plan.table_params:
                sink = getattr(plan, "dense_sink", None)
                g_wd = sink.grad_of(plan.wide_dense_weight) if sink is not None else None
                if g_wd is None:
                    g_wd = torch.empty((len(plan.wdense_cols), 1), dtype=torch.float32, device=X.device)
                    g_w = g_wd
            else:
                g_dense = g_wide[:, len(plan.wide)] if plan.wide_per_field else g_wide
                g_w = plan.dense_matrix(X, plan.wdense_cols).t().mv(g_dense).unsqueeze(1)
    return g_wide, g_wd, g_w


def _update_tables(plan, X, ids_t, parts_t, seg_event, g_out, ld_g, out, fm_s, g_fm, g_wide, g_wd, g_w, den_t, amax):
    """What a lookup's backward does with the row gradients, selected by ``plan.update`` (module docstring): hand them to
    the data-parallel exchange, the lazy regularised / Adam step (fused into the sorted update, or two passes), the
    deterministic sorted update with the optimizer fused in (sgd / adagrad / dense-accumulate), or the atomic scatter
    (+ consume pass).  ``g_out [B, ld_g]`` holds field f's gradient at ``plan.deep[f].out_off`` (EmbedFunction: the
    gradient of its output rows; PairEmbedFunction: the row gradients its backward kernel wrote).  ``ids_t`` /
    ``parts_t`` / ``seg_event`` / ``den_t`` / ``amax`` are the forward's side outputs (None: the batch is outside what the
    sorted update takes)."""
    B = X.shape[0]
    if getattr(plan, "exchange", None) is not None:
        # data-parallel: the trainer all-gathers the row gradients and applies the global update
        plan.exchange(X=X, g_out=g_out, out=out, fm_s=fm_s, g_fm=g_fm, g_wide=g_wide, amax=amax)
        return

    update = plan.update
    kind = update[0]
    stream = L.stream_handle(X.device)

    if kind == "lazy":
        lazy = plan.lazy
        if lazy is None or lazy.plan is not plan or ids_t is None:
            raise NotImplementedError("the lazy regularised / Adam table update needs lookups through the model's "
                                      "own plan and a batch the deterministic update kernel supports "
                                      "(DCTR_LAZY_UPDATE=0 selects the exact dense path)")
        lazy._ensure(X.device)
        cplan = plan.bind(X.device)
        ws, ws_n, pre = plan.update_workspace_for(ids_t, seg_event, B)
        # round 6: with pre-sorted entries the regularised / Adam step runs at the row, inside the sorted update (no
        # gradient slab, no second pass over the batch's rows: csrc/update_kernels.hpp DCTR_UPD_LAZY)
        if pre and lazy.update_fused(plan, cplan, ids_t, parts_t, B, g_out, ld_g, out, fm_s, g_fm, g_wide, X, g_wd, ws,
                                     ws_n):
            return
        call("dctr_embed_update", cplan, plan.units_ptr(), plan.n_grid_units, plan.max_vocab, ptr(ids_t),
             ptr(parts_t), B, ptr(g_out), ld_g, ptr(out), plan.ld_out, ptr(fm_s),
             fm_s.stride(0) if fm_s is not None else 0, ptr(g_fm), ptr(g_wide), plan.ld_wide, L.UPD_ACCUM, 0.0, 0.0,
             ptr(X), X.stride(0), ptr(g_wd), None, ptr(ws), ws_n, pre, stream)
        lazy.apply(ids_t)
        return

    if ids_t is not None:
        # deterministic single-pass path (csrc/update.hip): no atomics, optimizer fused in
        if kind == "dense":
            plan.ensure_gacc()
            plan.prepare_dense_grads()
            opt, lr, eps = L.UPD_ACCUM, 0.0, 0.0
        elif kind == "sgd":
            opt, lr, eps = L.UPD_SGD, float(update[1]), 0.0
        elif kind == "adagrad":
            opt, lr, eps = L.UPD_ADAGRAD, float(update[1]), float(update[2])
        else:
            raise RuntimeError("unknown sparse update mode %r" % (kind,))
        cplan = plan.bind(X.device)
        sink = getattr(plan, "dense_sink", None)
        # (armed AND carried out by the tower + head kernel of this step: only then has its event been recorded and
        # does nobody else step Linear.weight)
        inline = getattr(sink, "inline", None) if (sink is not None and getattr(sink, "inline_done", False)) else None
        side = None
        if inline is not None and X.is_cuda and seg_event is not None and seg_event[0] is not True and \
                sink.update_stream is seg_event[0]:
            # fused train step with in-kernel optimizer: the update leaves the critical chain -- it runs on the
            # pre-pass's side stream, behind the pre-pass and behind the tower kernel that produced its gradients,
            # beside the tower's weight-gradient kernels (which stay on the main stream).  DenseSlab.join() brings
            # the streams together at the end of the step.
            side = seg_event[0]      # (already waiting for the tower + head launch: mlp.TowerHeadFunction)
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            ws, ws_n, pre = plan.update_workspace_for(ids_t, seg_event, B)
            wd = ctypes.byref(inline) if (inline is not None and g_wd is not None and g_w is None) else None
            call("dctr_embed_update", cplan, plan.units_ptr(), plan.n_grid_units, plan.max_vocab, ptr(ids_t),
                 ptr(parts_t), B, ptr(g_out), ld_g, ptr(out), plan.ld_out, ptr(fm_s),
                 fm_s.stride(0) if fm_s is not None else 0, ptr(g_fm), ptr(g_wide), plan.ld_wide, opt, lr, eps,
                 ptr(X), X.stride(0), ptr(g_wd), wd, ptr(ws), ws_n, pre, L.stream_handle(X.device))
        if side is not None:
            # (everything the side-stream kernels touch stays allocated until the join)
            sink.forked(side, (X, out, ids_t, parts_t, fm_s, g_out, g_fm, g_wide, g_wd, ws, den_t, amax))
        return

    # general path (pooled VarLen fields, shared tables, very large batches): atomic scatter (+ consume pass)
    if kind == "sgd" and not plan.has_maxpool:
        cplan = plan.bind(X.device)
        call("dctr_embed_bwd", cplan, ptr(X), X.stride(0), B, ptr(g_out), ld_g, ptr(out), plan.ld_out, ptr(g_fm),
             ptr(g_wide), L.BWD_SGD, float(update[1]), stream)
        return

    plan.ensure_gacc()
    if kind == "dense":
        plan.prepare_dense_grads()
    cplan = plan.bind(X.device)
    call("dctr_embed_bwd", cplan, ptr(X), X.stride(0), B, ptr(g_out), ld_g, ptr(out), plan.ld_out, ptr(g_fm),
         ptr(g_wide), L.BWD_ACCUM, 0.0, stream)
    if kind == "sgd":
        call("dctr_embed_apply", cplan, ptr(X), X.stride(0), B, L.OPT_SGD, float(update[1]), 0.0, stream)
    elif kind == "adagrad":
        call("dctr_embed_apply", cplan, ptr(X), X.stride(0), B, L.OPT_ADAGRAD, float(update[1]), float(update[2]),
             stream)
    elif kind != "dense":
        raise RuntimeError("unknown sparse update mode %r" % (kind,))


def embed(plan, X, want_fm=False, full=False):
    """(out [B, width] view, wide [B], fm [B]) for model input ``X`` under ``plan``.  ``full`` returns the
    un-sliced ``[B, ld_out]`` buffer (the MFMA tower reads the first ``plan.width`` columns of it and hands back
    a gradient of the same shape, so no slice / zero-fill kernels appear in the autograd graph)."""
    L.require_gpu(X, "model input X")
    sharder = getattr(plan, "sharder", None)
    if sharder is not None:          # table-sharded multi-GPU training (parallel.ShardedTrainer)
        return sharder.embed(X, want_fm, full)
    owner = getattr(plan, "_owner", None)
    if owner is not None and getattr(owner, "sharder", None) is not None and torch.is_grad_enabled():
        # A SECONDARY plan over tables that a ShardedTrainer has sharded (gather_columns / input_from_feature_columns /
        # Linear.forward next to the model's own fused lookup: IFM / DIFM-style models): this rank's copy of a table it
        # does not own is stale and the local update below would fork it -- training would diverge silently (round-3
        # advisor finding).  Only lookups through the model plan go through the exchange.
        raise NotImplementedError("this lookup reads tables that are sharded across ranks (ShardedTrainer) through a "
                                  "secondary plan: only the model's own fused lookup is routed through the exchange; "
                                  "train this model with DataParallelTrainer")
    plan.bind(X.device)
    out, wide, fm = EmbedFunction.apply(plan, X, plan.anchor, plan.wide_dense_weight, bool(want_fm),
                                        torch.is_grad_enabled())
    if plan.has_lookup and not full:
        out = out[:, :plan.width]
    return out, wide, fm


# ---- ONN's pair lookup (models/onn.py:98-120; csrc/pair_embed.hip) ---------------------------------------------------
class PairEmbedFunction(torch.autograd.Function):
    """Lookup through a pair plan (``EmbeddingPlan(pair=True)``): ``out [B, ld_out]`` = the P products ``emb1_p[id_i] *
    emb2_p[id_j]`` followed by the dense block, ``wide [B]`` the first-order logit -- ``dctr_pair_embed_fwd``.  The backward
    turns the gradient of ``out`` into row gradients (``dctr_pair_embed_bwd``: ``g_rows [B, ld_rows]``, field f's slice at
    its ``out_off``) and hands them to the update ``plan.update`` selects, exactly as ``EmbedFunction.backward`` does."""

    @staticmethod
    def forward(ctx, plan, X, anchor, wdense_w, for_backward=False):
        X, _ = rows2(X, "model input X")
        if X.shape[1] < plan.n_xcols:
            raise ValueError("X has %d columns, the feature columns need %d" % (X.shape[1], plan.n_xcols))
        B = X.shape[0]
        cplan = plan.bind(X.device)
        out = torch.empty((B, plan.ld_out), dtype=torch.float32, device=X.device) if plan.has_lookup else None
        wide = torch.empty((B,), dtype=torch.float32, device=X.device) if plan.has_wide else None
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
        if ids_t is not None:
            call("dctr_embed_ids", cplan, plan.units_ptr(), plan.n_grid_units, ptr(X), X.stride(0), B, ptr(ids_t),
                 ptr(parts_t), stream)
            if plan.segments_enabled():
                ctx.seg_event = plan.launch_segments(ids_t, parts_t, B)
        err = plan.err_flag(X.device)
        call("dctr_pair_embed_fwd", cplan, ptr(X), X.stride(0), B, ptr(out), plan.ld_out, ptr(wide), 1, ptr(err),
             stream)
        ctx.plan = plan
        ctx.save_for_backward(X, ids_t, parts_t, den_t, amax)
        ctx.set_materialize_grads(False)
        return (out if out is not None else X.new_zeros((B, 0)), wide if wide is not None else X.new_zeros((B,)))

    @staticmethod
    def backward(ctx, g_out, g_wide):
        plan = ctx.plan
        X, ids_t, parts_t, den_t, amax = ctx.saved_tensors
        B = X.shape[0]
        plan.point_step_buffers(den_t, amax)
        if not plan.deep:
            g_out = None
        if not plan.has_wide:
            g_wide = None
        g_wide, g_wd, g_w = _wide_dense_grad(plan, X, g_wide, ids_t, ctx.needs_input_grad[3])
        if (g_out is None and g_wide is None) or not plan.table_params:
            return None, None, None, g_w, None
        g_rows, ld_rows = None, 0
        if g_out is not None:
            g_out, ld_g = padded_rows(g_out, 0, plan.vec)
            ld_rows = plan.ld_rows
            g_rows = torch.empty((B, ld_rows), dtype=torch.float32, device=X.device)
            call("dctr_pair_embed_bwd", plan.bind(X.device), ptr(X), X.stride(0), B, ptr(g_out), ld_g, ptr(g_rows),
                 ld_rows, L.stream_handle(X.device))
        _update_tables(plan, X, ids_t, parts_t, ctx.seg_event, g_rows, ld_rows, None, None, None, g_wide, g_wd, g_w, den_t,
                       amax)
        return None, None, None, g_w, None


def pair_embed(plan, X, full=False):
    """(out [B, width] view, wide [B]) of ONN's pair lookup for model input ``X`` under the pair plan ``plan``; ``full``
    returns the un-sliced ``[B, ld_out]`` buffer (what the MFMA tower reads in place)."""
    L.require_gpu(X, "model input X")
    if not getattr(plan, "pair", False):
        raise ValueError("pair_embed needs a pair plan (EmbeddingPlan(pair=True))")
    if getattr(plan, "sharder", None) is not None or getattr(plan, "exchange", None) is not None:
        raise NotImplementedError("the pair lookup (ONN) is not wired into the multi-GPU trainers")
    plan.bind(X.device)
    out, wide = PairEmbedFunction.apply(plan, X, plan.anchor, plan.wide_dense_weight, torch.is_grad_enabled())
    if plan.has_lookup and not full:
        out = out[:, :plan.width]
    return out, wide


_PLAN_CACHE_ATTR = "_dctr_plans"


class SplitGatheredFunction(torch.autograd.Function):
    """``full [B, ld]`` (``embed(..., full=True)``) -> (``full[:, :W].view(B, F, D)``, ``full[:, W:W + nd]``): the two views every
    interaction model takes of the gather's output.  As plain slices their backward is three zero-fills, three copies and
    an add of [B, ld] tensors (7 launches, ~30 us at the Criteo shape); here it is two copies into one buffer."""

    @staticmethod
    def forward(ctx, full, W, F, D, nd):
        ctx.dims = (full.shape[0], full.shape[1], int(W), int(nd))
        emb = full[:, :W].view(full.shape[0], F, D)
        return emb, full[:, W:W + nd]

    @staticmethod
    def backward(ctx, g_emb, g_dense):
        B, ld, W, nd = ctx.dims
        ref = g_emb if g_emb is not None else g_dense
        g = torch.empty((B, ld), dtype=ref.dtype, device=ref.device)
        if ref.is_cuda and ref.dtype == torch.float32 and W % 4 == 0 and ld % 4 == 0 and \
                os.environ.get("DCTR_GLUE_KERNELS", "1") != "0":
            # one launch (csrc/head.hip k_rows_join) instead of two copies and a fill
            ge = padded_rows(g_emb.reshape(B, W))[0] if g_emb is not None else None
            gd = rows2(g_dense, "dense gradient")[0] if (g_dense is not None and nd > 0) else None
            call("dctr_rows_join", ptr(ge), ge.stride(0) if ge is not None else 0, None, 0, W, ptr(gd),
                 gd.stride(0) if gd is not None else 0, nd if gd is not None else 0, ptr(g), ld, B,
                 L.stream_handle(ref.device))
            return g, None, None, None, None
        if g_emb is not None:
            g[:, :W].copy_(g_emb.reshape(B, W))
        else:
            g[:, :W].zero_()
        if g_dense is not None and nd > 0:
            g[:, W:W + nd].copy_(g_dense)
            if ld > W + nd:
                g[:, W + nd:].zero_()
        elif ld > W:
            g[:, W:].zero_()
        return g, None, None, None, None


def split_gathered(full, plan):
    """(emb [B, F, D] view, dense [B, n_dense] view or None) of ``embed(plan, X, full=True)[0]``."""
    nd = len(plan.dense_cols)
    if not full.requires_grad or full.stride(1) != 1:
        emb = full[:, :plan.emb_width].reshape(full.shape[0], len(plan.deep), plan.emb_dim)
        return emb, (full[:, plan.emb_width:plan.emb_width + nd] if nd else None)
    emb, dense = SplitGatheredFunction.apply(full, plan.emb_width, len(plan.deep), plan.emb_dim, nd)
    return emb, (dense if nd else None)


def gather_columns(X, embedding_dict, feature_index, columns, pooled=True):
    """Per-column embeddings as views of ONE fused gather: ``[B, 1, D]`` per SparseFeat (and per pooled
    VarLenSparseFeat), ``[B, maxlen, D]`` per un-pooled VarLenSparseFeat.  Backs the reference-shaped
    helpers (``embedding_lookup``, ``varlen_embedding_lookup``, ``input_from_feature_columns``)."""
    cache = embedding_dict.__dict__.setdefault(_PLAN_CACHE_ATTR, {})
    key = (tuple(c.name for c in columns), bool(pooled), id(feature_index))
    plan = cache.get(key)
    if plan is None:
        plan = EmbeddingPlan(feature_index, deep_columns=list(columns), deep_tables=embedding_dict,
                             unpooled=not pooled, with_dense=False)
        owner = getattr(embedding_dict, "_dctr_owner_plan", None)
        if owner is not None:
            plan.share_update_with(owner)
        cache[key] = plan
    out, _, _ = embed(plan, X)
    B = X.shape[0]
    sparse_cols = [c for c in columns if not hasattr(c, "maxlen")]
    varlen_cols = [c for c in columns if hasattr(c, "maxlen")]
    views, off = {}, 0
    for c in sparse_cols:
        d = embedding_dict[c.embedding_name].weight.shape[1]
        views[c.name] = out[:, off:off + d].unsqueeze(1)
        off += d
    for c in varlen_cols:
        d = embedding_dict[c.embedding_name].weight.shape[1]
        t = 1 if pooled else c.maxlen
        views[c.name] = out[:, off:off + t * d].reshape(B, t, d)
        off += t * d
    return [views[c.name] for c in columns]


