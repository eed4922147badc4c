# -*- coding: utf-8 -*-
"""DIN -- Deep Interest Network (reference models/din.py:15-130): the user's behaviour sequences are pooled by an
attention unit that scores every behaviour against the candidate item, and the result joins the other embeddings in front
of the DNN.

Forward = ONE fused gather with the history columns un-pooled (``EmbeddingPlan(unpooled=names)``: every position is a
fixed field of the row), ONE kernel for the whole ``AttentionSequencePoolingLayer`` reading the query and the keys in
place from that row (csrc/din.hip), one concatenation, the MFMA tower.  The attention unit's parameters live outside the
tower, so training takes autograd + ``torch.optim`` around the kernels, as CCPM's does; the tables are shared between the
candidate and the history columns, so their update runs on general units."""
import torch
import torch.nn as nn

from .basemodel import BaseModel
from ..inputs import SparseFeat, VarLenSparseFeat
from ..layers import DNN, AttentionSequencePoolingLayer


class DIN(BaseModel):
    """Same arguments as the reference (models/din.py:38-42)."""

    def __init__(self, dnn_feature_columns, history_feature_list, dnn_use_bn=False, dnn_hidden_units=(256, 128),
                 dnn_activation='relu', att_hidden_size=(64, 16), att_activation='Dice', att_weight_normalization=False,
                 l2_reg_dnn=0.0, l2_reg_embedding=1e-6, dnn_dropout=0, init_std=0.0001, seed=1024, task='binary',
                 device='cpu', gpus=None):
        super(DIN, self).__init__([], dnn_feature_columns, l2_reg_linear=0, l2_reg_embedding=l2_reg_embedding,
                                  init_std=init_std, seed=seed, task=task, device=device, gpus=gpus)
        cols = list(dnn_feature_columns) if dnn_feature_columns else []
        self.sparse_feature_columns = [c for c in cols if isinstance(c, SparseFeat)]
        self.varlen_sparse_feature_columns = [c for c in cols if isinstance(c, VarLenSparseFeat)]
        self.history_feature_list = history_feature_list
        self.history_fc_names = ["hist_" + name for name in history_feature_list]
        self.history_feature_columns = [c for c in self.varlen_sparse_feature_columns if c.name in self.history_fc_names]
        self.sparse_varlen_feature_columns = [c for c in self.varlen_sparse_feature_columns
                                              if c.name not in self.history_fc_names]
        self._unpooled_columns = tuple(c.name for c in self.history_feature_columns)
        self._length_names = [c.length_name for c in self.varlen_sparse_feature_columns if c.length_name is not None]
        # (generator order decides the weights a seed gives: the attention unit, the tower, its projection.  The tower
        # takes the DNN's own default init_std and l2_reg_dnn adds no regularisation group, as in the reference)
        self.attention = AttentionSequencePoolingLayer(att_hidden_units=att_hidden_size,
                                                       embedding_dim=self._compute_interest_dim(),
                                                       att_activation=att_activation, return_score=False,
                                                       supports_masking=False,
                                                       weight_normalization=att_weight_normalization)
        self.dnn = DNN(inputs_dim=self.compute_input_dim(dnn_feature_columns), hidden_units=dnn_hidden_units,
                       activation=dnn_activation, dropout_rate=dnn_dropout, l2_reg=l2_reg_dnn, use_bn=dnn_use_bn)
        self.dnn_linear = nn.Linear(dnn_hidden_units[-1], 1, bias=False).to(device)
        self.to(device)

    def _compute_interest_dim(self):
        return sum(c.embedding_dim for c in self.sparse_feature_columns if c.name in self.history_feature_list)

    def _layout(self):
        """Where the attention's operands lie in the gathered row: ``(segs, T, sparse width, pooled (lo, hi))`` with one
        ``(dim, q_off, k_off, k_step)`` per history feature (candidate column j against history column j, both in
        declaration order), or ``segs = None`` when the columns do not pair up position by position."""
        plan = self.model_plan()
        hit = self.__dict__.get("_layout_cache")
        if hit is not None and hit[0] is plan:                 # constant per plan: kept beside it
            return hit[1]
        off = dict((f.name, f.out_off) for f in plan.deep)
        n_sparse = len(self.sparse_feature_columns)
        sparse_w = sum(f.dim for f in plan.deep[:n_sparse])
        pooled = plan.deep[plan.n_deep_fixed:]
        pooled_lo = pooled[0].out_off if pooled else plan.emb_width
        queries = [c for c in self.sparse_feature_columns if c.name in self.history_feature_list]
        keys = self.history_feature_columns
        T = keys[0].maxlen if keys else 0
        segs = None
        if keys and len(queries) == len(keys) and all(k.maxlen == T for k in keys) and \
                all(q.embedding_dim == k.embedding_dim for q, k in zip(queries, keys)):
            segs = [(q.embedding_dim, off[q.name], off[k.name + "[0]"], k.embedding_dim) for q, k in zip(queries, keys)]
        out = (segs, T, sparse_w, (pooled_lo, plan.emb_width), queries, keys, off)
        self.__dict__["_layout_cache"] = (plan, out)
        return out

    def logit_parts(self, X):
        names = self._length_names
        if len(names) == 0:
            raise ValueError('please add max length column for VarLenSparseFeat of DIN/DIEN input')
        plan = self.model_plan()
        segs, T, sparse_w, (plo, phi), queries, keys, off = self._layout()
        gathered, _, _ = self.fused_inputs(X)
        B = X.shape[0]
        lengths = X[:, self.feature_index[names[0]][0]]
        att = self.attention
        needs_grad = torch.is_grad_enabled() and (gathered.requires_grad or
                                                   any(p.requires_grad for p in att.local_att.parameters()))
        act = att.kernel_route(T, [s[0] for s in segs], (gathered,), needs_grad) if segs is not None else None
        if act is not None:
            hist = att.fused(gathered, None, segs, T, lengths.to(torch.int32).contiguous(), None, act)
        else:
            q = torch.cat([gathered[:, off[c.name]:off[c.name] + c.embedding_dim] for c in queries], dim=-1)
            k = torch.cat([gathered[:, off[c.name + "[0]"]:off[c.name + "[0]"] + c.maxlen * c.embedding_dim]
                          .reshape(B, c.maxlen, c.embedding_dim) for c in keys], dim=-1)
            hist = att(q.unsqueeze(1), k, lengths.long().reshape(-1, 1)).squeeze(1)
        parts = [gathered[:, :sparse_w], gathered[:, plo:phi], hist]
        if plan.dense_cols:
            parts.append(gathered[:, plan.dense_off:plan.dense_off + len(plan.dense_cols)])
        return [self.tower_logit(torch.cat(parts, dim=-1))]
