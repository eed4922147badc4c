# -*- coding: utf-8 -*-
"""DIEN -- Deep Interest Evolution Network (reference models/dien.py:16-381): a GRU extracts an interest state from
every behaviour, an attention unit scores the states against the candidate item, and a second recurrence -- a GRU
followed by attention pooling, or a GRU whose input (AIGRU), update gate (AUGRU) or whole update (AGRU) is driven by the
scores -- evolves them into one vector that joins the other embeddings in front of the DNN.

Forward = ONE fused gather with the history columns (and, under negative sampling, the negative history columns)
un-pooled, the extractor GRU reading the history positions in place from that row, the evolution recurrence, one
concatenation, the MFMA tower.  Every recurrence is one kernel per direction (csrc/gru_seq.hip) that reads the lengths
on the device: nothing travels to the host, so ``fit()`` replays the step as a hipGraph.  The recurrent and attention
parameters live outside the tower, so training takes autograd + ``torch.optim`` around the kernels, as DIN's does.

One deliberate difference from the reference: a batch in which EVERY length is 0 raises ``ValueError: not enough values
to unpack`` there (its extractor returns a 1-tuple); here such a batch gives ``hist = 0`` and an auxiliary loss of 0,
which is what every row of length 0 gives in any other batch."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .basemodel import BaseModel
from .._hip import lib as _L
from .._hip import mlp as _mlp
from ..inputs import DenseFeat, SparseFeat, VarLenSparseFeat
from ..layers import DNN, AttentionSequencePoolingLayer, DynamicGRU
from ..layers.sequence import gru_sequence


def _gru_weights(gru):
    return gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0


class InterestExtractor(nn.Module):
    """The interest extractor layer (reference models/dien.py:181-273; same constructor and ``state_dict`` keys).
    ``nn.GRU`` holds the parameters -- construction consumes the generator exactly as the reference's does -- and the
    recurrence runs through ``gru_sequence`` on padded tensors.

    ``forward(keys [B, T, H], keys_length [B], neg_keys [B, T, H] | None) -> (interests [B, T, H], aux_loss [1])``: all B
    rows stay in place (the reference drops the rows of length 0 and puts zeros back later); ``interests`` is 0 beyond a
    row's length."""

    def __init__(self, input_size, use_neg=False, init_std=0.001, device='cpu'):
        super(InterestExtractor, self).__init__()
        self.use_neg = use_neg
        self.gru = nn.GRU(input_size=input_size, hidden_size=input_size, batch_first=True)
        if self.use_neg:
            self.auxiliary_net = DNN(input_size * 2, [100, 50, 1], 'sigmoid', init_std=init_std, device=device)
        for name, tensor in self.gru.named_parameters():
            if 'weight' in name:
                nn.init.normal_(tensor, mean=0, std=init_std)
        self.to(device)

    def states(self, X, segs, T, lengths):
        """``[B, T, H]`` interest states from rows that hold the key segments ``[(dim, x_off, x_step)]``"""
        return gru_sequence(X, segs, T, lengths, None, 'GRU', *_gru_weights(self.gru), want_states=True,
                            want_last=False)[0]

    def auxiliary_loss(self, states, click_seq, noclick_seq, lengths):
        """Mean BCE of ``auxiliary_net`` over ``[h_t, e_{t+1}]`` (target 1) and ``[h_t, neg_{t+1}]`` (target 0) for every
        ``t < n - 1`` of every row with ``n >= 2``; 0 when there is none.  ``states``: h_t for t < T - 1; ``click_seq`` /
        ``noclick_seq``: the positions 1..T-1.  Every row of ``[B, T - 1]`` is evaluated and the invalid ones are weighted
        0 (the net has no BatchNorm, so the valid rows' values are those of evaluating them alone): nothing depends on
        how many there are, and the count stays on the device.  (Evaluating only the valid rows would make the row
        count depend on the data: a host synchronisation per step, and no hipGraph replay.  The price is the net's
        arithmetic on the invalid rows.)"""
        B, T1, H = states.shape
        valid = (torch.arange(T1, device=states.device).unsqueeze(0) < (lengths.reshape(-1, 1) - 1)).to(states.dtype)
        p1 = self.auxiliary_net(torch.cat([states, click_seq], dim=-1).reshape(B * T1, 2 * H)).reshape(B, T1)
        p0 = self.auxiliary_net(torch.cat([states, noclick_seq], dim=-1).reshape(B * T1, 2 * H)).reshape(B, T1)
        bce = F.binary_cross_entropy(p1, torch.ones_like(p1), reduction='none') + \
            F.binary_cross_entropy(p0, torch.zeros_like(p0), reduction='none')
        return ((bce * valid).sum() / (2.0 * valid.sum()).clamp(min=1.0)).reshape(1)

    def forward(self, keys, keys_length, neg_keys=None):
        B, T, H = keys.shape
        interests = self.states(keys.reshape(B, T * H), [(H, 0, H)], T, keys_length)
        aux_loss = torch.zeros((1,), device=keys.device)
        if self.use_neg and neg_keys is not None:
            aux_loss = self.auxiliary_loss(interests[:, :-1, :], keys[:, 1:, :], neg_keys[:, 1:, :], keys_length)
        return interests, aux_loss


class InterestEvolving(nn.Module):
    """The interest evolving layer (reference models/dien.py:276-381; same constructor, errors and ``state_dict`` keys).

    ``forward(query [B, H], keys [B, T, H], keys_length [B]) -> [B, H]``, 0 for a row of length 0.  ``GRU``: a second
    recurrence over the states, then attention pooling of its states (``csrc/din.hip``).  ``AIGRU`` / ``AGRU`` /
    ``AUGRU``: the attention scores (torch ops: ``return_score``) drive ONE recurrence whose last state is the result."""
    __SUPPORTED_GRU_TYPE__ = ['GRU', 'AIGRU', 'AGRU', 'AUGRU']

    def __init__(self, input_size, gru_type='GRU', use_neg=False, init_std=0.001, att_hidden_size=(64, 16),
                 att_activation='sigmoid', att_weight_normalization=False):
        super(InterestEvolving, self).__init__()
        if gru_type not in InterestEvolving.__SUPPORTED_GRU_TYPE__:
            raise NotImplementedError("gru_type: {gru_type} is not supported")
        self.gru_type = gru_type
        self.use_neg = use_neg
        self.attention = AttentionSequencePoolingLayer(embedding_dim=input_size, att_hidden_units=att_hidden_size,
                                                       att_activation=att_activation,
                                                       weight_normalization=att_weight_normalization,
                                                       return_score=gru_type != 'GRU')
        if gru_type in ('GRU', 'AIGRU'):
            self.interest_evolution = nn.GRU(input_size=input_size, hidden_size=input_size, batch_first=True)
        else:
            self.interest_evolution = DynamicGRU(input_size=input_size, hidden_size=input_size, gru_type=gru_type)
        for name, tensor in self.interest_evolution.named_parameters():
            if 'weight' in name:
                nn.init.normal_(tensor, mean=0, std=init_std)

    def forward(self, query, keys, keys_length, mask=None):
        B, T, H = keys.shape
        lengths = keys_length.reshape(-1).to(keys.device)        # (user code may hold them on the host)
        rows, segs = keys.reshape(B, T * H), [(H, 0, H)]
        if self.gru_type == 'GRU':
            interests = gru_sequence(rows, segs, T, lengths, None, 'GRU', *_gru_weights(self.interest_evolution),
                                     want_states=True, want_last=False)[0]
            # (a row of length 0 has interests == 0, so whatever weights it gets -- 1/T under a softmax -- give 0)
            return self.attention(query.unsqueeze(1), interests, lengths.reshape(-1, 1)).squeeze(1)
        scores = self.attention(query.unsqueeze(1), keys, lengths.reshape(-1, 1)).squeeze(1)          # [B, T]
        if self.gru_type == 'AIGRU':
            return gru_sequence(rows, segs, T, lengths, scores, 'AIGRU', *_gru_weights(self.interest_evolution),
                                want_states=False, want_last=True)[1]
        return self.interest_evolution.fused(rows, scores, lengths, segs, T, want_states=False, want_last=True)[1]


class DIEN(BaseModel):
    """Same arguments as the reference (models/dien.py:42-48)."""

    def __init__(self, dnn_feature_columns, history_feature_list, gru_type="GRU", use_negsampling=False, alpha=1.0,
                 use_bn=False, dnn_hidden_units=(256, 128), dnn_activation='relu', att_hidden_units=(64, 16),
                 att_activation="relu", att_weight_normalization=True, l2_reg_dnn=0, l2_reg_embedding=1e-6, dnn_dropout=0,
                 init_std=0.0001, seed=1024, task='binary', device='cpu', gpus=None):
        super(DIEN, self).__init__([], dnn_feature_columns, l2_reg_linear=0, l2_reg_embedding=l2_reg_embedding,
                                   init_std=init_std, seed=seed, task=task, device=device, gpus=gpus)
        self.item_features = history_feature_list
        self.use_negsampling = use_negsampling
        self.alpha = alpha
        cols = list(dnn_feature_columns) if dnn_feature_columns else []
        self.sparse_feature_columns = [c for c in cols if isinstance(c, SparseFeat)]
        self.dense_feature_columns = [c for c in cols if isinstance(c, DenseFeat)]
        self.varlen_sparse_feature_columns = [c for c in cols if isinstance(c, VarLenSparseFeat)]
        hist_names = ["hist_" + name for name in history_feature_list]
        neg_names = ["neg_" + name for name in hist_names]
        self.history_feature_columns = [c for c in self.varlen_sparse_feature_columns if c.name in hist_names]
        self.neg_history_feature_columns = [c for c in self.varlen_sparse_feature_columns if c.name in neg_names]
        unpooled = self.history_feature_columns + (self.neg_history_feature_columns if use_negsampling else [])
        self._unpooled_columns = tuple(c.name for c in unpooled)
        self._length_names = [c.length_name for c in self.varlen_sparse_feature_columns if c.length_name is not None]
        self._check_slots(unpooled)

        input_size = self._compute_interest_dim()
        # (generator order decides the weights a seed gives: extractor, evolution, tower, projection)
        self.interest_extractor = InterestExtractor(input_size=input_size, use_neg=use_negsampling, init_std=init_std)
        self.interest_evolution = InterestEvolving(input_size=input_size, gru_type=gru_type, use_neg=use_negsampling,
                                                   init_std=init_std, att_hidden_size=att_hidden_units,
                                                   att_activation=att_activation,
                                                   att_weight_normalization=att_weight_normalization)
        self.dnn = DNN(self._compute_dnn_dim() + input_size, dnn_hidden_units, dnn_activation, l2_reg_dnn, dnn_dropout,
                       use_bn, init_std=init_std, seed=seed)
        self.linear = nn.Linear(dnn_hidden_units[-1], 1, bias=False)
        nn.init.normal_(self.linear.weight, mean=0, std=init_std)
        self.to(device)

    def _check_slots(self, unpooled):
        """Every un-pooled position is an update slot of its table's unit, beside the candidate column's own and those of
        every other column over the same table; a unit holds DCTR_MAX_UNIT_SLOTS of them."""
        names = set(c.embedding_name for c in unpooled)
        for name in names:
            slots = sum(1 for c in self.sparse_feature_columns if c.embedding_name == name) + \
                sum(c.maxlen for c in self.varlen_sparse_feature_columns if c.embedding_name == name)
            if slots > _L.MAX_UNIT_SLOTS:
                raise ValueError(
                    "DIEN: the columns over embedding table '%s' feed %d update slots, more than DCTR_MAX_UNIT_SLOTS = %d: "
                    "a history that shares the candidate's table is bounded by T <= %d (T <= %d with negative sampling)"
                    % (name, slots, _L.MAX_UNIT_SLOTS, _L.MAX_UNIT_SLOTS - 1, (_L.MAX_UNIT_SLOTS - 1) // 2))

    def _compute_interest_dim(self):
        return sum(c.embedding_dim for c in self.sparse_feature_columns if c.name in self.item_features)

    def _compute_dnn_dim(self):
        return sum(c.embedding_dim for c in self.sparse_feature_columns) + sum(c.dimension for c in self.dense_feature_columns)

    def _graph_safe_step(self):
        # The auxiliary loss is recomputed on the device by every forward and the lengths never leave it: no host-side
        # value enters a launch, so the rule that keeps a model with an auxiliary loss off the replay does not bind here.
        keep = self.__dict__.get("_aux_default", True)
        self._aux_default = True
        try:
            return super(DIEN, self)._graph_safe_step()
        finally:
            self._aux_default = keep

    def _layout(self):
        """Where the operands lie in the gathered row: ``(key segs, negative key segs, T, sparse width, offsets)`` with one
        ``(dim, x_off, x_step)`` per history column in declaration order."""
        plan = self.model_plan()
        hit = self.__dict__.get("_layout_cache")
        if hit is not None and hit[0] is plan:
            return hit[1]
        off = dict((f.name, f.out_off) for f in plan.deep)
        sparse_w = sum(f.dim for f in plan.deep[:len(self.sparse_feature_columns)])
        keys = self.history_feature_columns
        T = keys[0].maxlen if keys else 0
        segs = [(c.embedding_dim, off[c.name + "[0]"], c.embedding_dim) for c in keys]
        negs = [(c.embedding_dim, off[c.name + "[0]"], c.embedding_dim) for c in self.neg_history_feature_columns] \
            if self.use_negsampling else []
        out = (segs, negs, T, sparse_w, off)
        self.__dict__["_layout_cache"] = (plan, out)
        return out

    @staticmethod
    def _positions(gathered, segs, lo, hi):
        """the positions lo..hi-1 of the segments as one ``[B, hi - lo, H]`` tensor"""
        B = gathered.shape[0]
        return torch.cat([gathered[:, o + lo * st:o + hi * st].reshape(B, hi - lo, d) for d, o, st in segs], dim=-1)

    def logit_parts(self, X):
        names = self._length_names
        if len(names) == 0:
            raise ValueError('please add max length column for VarLenSparseFeat of DIN/DIEN input')
        # The auxiliary loss of the step before still holds that step's autograd graph, AccumulateGrad nodes included.  A node
        # that is alive is reused: inside a hipGraph capture the parameters' gradients would then be accumulated on the
        # stream of the eager step that created it, and the capture ends with unjoined work.  Let go of it first.
        self.aux_loss = self.aux_loss.detach()
        plan = self.model_plan()
        segs, negs, T, sparse_w, off = self._layout()
        gathered, _, _ = self.fused_inputs(X)
        lengths = X[:, self.feature_index[names[0]][0]].to(torch.int32)
        ext = self.interest_extractor
        states = ext.states(gathered, segs, T, lengths)                                   # keys read in place
        aux_loss = torch.zeros((1,), device=gathered.device)
        if self.use_negsampling and negs:
            aux_loss = ext.auxiliary_loss(states[:, :-1, :], self._positions(gathered, segs, 1, T),
                                          self._positions(gathered, negs, 1, T), lengths)
        self.add_auxiliary_loss(aux_loss, self.alpha)
        query = torch.cat([gathered[:, off[c.name]:off[c.name] + c.embedding_dim] for c in self.sparse_feature_columns
                           if c.name in self.item_features], dim=-1)
        hist = self.interest_evolution(query, states, lengths)
        parts = [hist, gathered[:, :sparse_w]]
        if plan.dense_cols:
            parts.append(gathered[:, plan.dense_off:plan.dense_off + len(plan.dense_cols)])
        return [_mlp.tower(self.dnn, self.linear, torch.cat(parts, dim=-1), None, sink=self._grad_sink)]
