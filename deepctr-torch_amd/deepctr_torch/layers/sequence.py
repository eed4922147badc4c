"""``SequencePoolingLayer``: sum / mean / max over the valid positions of an explicit ``[B, T, D]`` VarLen embedding
(the layer of reference layers/sequence.py:9-77, for code that pools tensors it built itself:
``inputs.get_varlen_pooling_list``, DIN-style user models).

The models of this package never instantiate it: their pooling happens inside the gather kernel
(``csrc/embed.hip: pool_field``) while the rows are still in registers.  This module states the same three reductions
with the kernel's conventions on a tensor: a position is valid when its mask bit is set (``supports_masking``) or its
index is below the row's length; ``mean`` divides by ``count + 1e-8``; ``max`` lowers every padded position by 1e9
before the reduction, so a row without valid positions yields its values minus 1e9, as the reference's does."""
import torch
import torch.nn as nn

_MODES = ('sum', 'mean', 'max')
_PAD_DROP = 1e9


def _valid_positions(lengths, T):
    """``[B, T]`` bool: position t of row b is valid when t < lengths[b] (lengths ``[B]`` or ``[B, 1]``)."""
    return torch.arange(T, device=lengths.device).unsqueeze(0) < lengths.reshape(-1, 1)


class SequencePoolingLayer(nn.Module):
    """``forward([seq [B, T, D], mask [B, T] bool])`` with ``supports_masking`` else ``forward([seq, lengths [B, 1]])``
    -> ``[B, 1, D]``."""

    def __init__(self, mode='mean', supports_masking=False, device='cpu'):
        super(SequencePoolingLayer, self).__init__()
        if mode not in _MODES:
            raise ValueError('parameter mode should in [sum, mean, max]')
        self.mode, self.supports_masking, self.device = mode, supports_masking, device
        self.eps = torch.FloatTensor([1e-8]).to(device)
        self.to(device)

    def forward(self, seq_value_len_list):
        seq, second = seq_value_len_list
        if self.supports_masking:
            valid = second.to(torch.bool)
            count = valid.sum(dim=1, keepdim=True).to(torch.float32)
        else:
            valid = _valid_positions(second, seq.shape[1])
            count = second.reshape(-1, 1).to(torch.float32)
        keep = valid.unsqueeze(-1).to(seq.dtype)                         # [B, T, 1], broadcast over D
        if self.mode == 'max':
            return (seq - (1.0 - keep) * _PAD_DROP).amax(dim=1, keepdim=True)
        total = (seq * keep).sum(dim=1, keepdim=True)                    # [B, 1, D]
        if self.mode == 'mean':
            total = total / (count + self.eps.to(count.device)).unsqueeze(-1)
        return total


_SOFTMAX_PAD = float(-2 ** 32 + 1)


class AttentionSequencePoolingLayer(nn.Module):
    """DIN's attention pooling (reference layers/sequence.py:80-154; same constructor): every behaviour is weighted by
    the local activation unit's score against the candidate and the weighted keys are summed.

    ``forward(query [B, 1, E], keys [B, T, E], keys_length [B, 1], mask=None) -> [B, 1, E]`` (``[B, 1, T]`` scores with
    ``return_score``).  Position t is valid when ``t < keys_length`` or, with ``supports_masking``, where ``mask [B, T]``
    is set.  Without ``weight_normalization`` an invalid position scores 0; with it, it scores ``-2**32 + 1`` in front of
    a softmax: weight exactly 0 -- unless the row has no valid position, which then weighs all T keys by 1/T.

    One kernel per direction (``csrc/din.hip``) when the inputs are float32 on the GPU, the shape is inside the kernel's
    envelope, the activation is linear / relu / sigmoid / prelu (or Dice in eval mode without a gradient: its BatchNorm
    is then a fixed per-unit affine map), ``return_score`` is off and the attention net has neither BatchNorm layers nor
    active dropout.  Everything else -- Dice in training, which normalises with the statistics of all B*T rows between
    the layers -- runs ``_forward_torch``."""

    def __init__(self, att_hidden_units=(80, 40), att_activation='sigmoid', weight_normalization=False,
                 return_score=False, supports_masking=False, embedding_dim=4, **kwargs):
        super(AttentionSequencePoolingLayer, self).__init__()
        from .core import LocalActivationUnit        # (this file also loads on its own, without the package around it)
        self.return_score = return_score
        self.weight_normalization = weight_normalization
        self.supports_masking = supports_masking
        self.local_att = LocalActivationUnit(hidden_units=att_hidden_units, embedding_dim=embedding_dim,
                                             activation=att_activation, dropout_rate=0, use_bn=False)

    def _valid(self, keys, keys_length, mask):
        if self.supports_masking:
            if mask is None:
                raise ValueError("When supports_masking=True,input must support masking")
            return mask.reshape(keys.shape[0], -1).to(torch.bool)
        return _valid_positions(keys_length, keys.shape[1])

    def kernel_route(self, T, dims, tensors, needs_grad):
        """The kernel's activation name when the fused route takes this call, else None."""
        from .._hip import ops as _ops
        if self.return_score or not all(t.is_cuda and t.dtype == torch.float32 for t in tensors):
            return None
        act = self.local_att.kernel_activation()
        if act is None or (act == "dice" and (self.training or needs_grad)):
            return None
        if self.local_att.dense.weight.dtype != torch.float32:          # (a module is converted as a whole)
            return None
        key = (int(T), tuple(dims), act)                                # the envelope: asked of the library once per shape
        cache = self.__dict__.setdefault("_route_cache", {})
        if key not in cache:
            hidden = [fc.out_features for fc in self.local_att.dnn.linears]
            cache[key] = _ops.din_attention_supported(T, list(dims), hidden, act)
        return act if cache[key] else None

    def fused(self, Q, K, segs, T, lengths=None, mask=None, act=None):
        """The kernel on rows that hold the query and key segments (``_hip/ops.DINAttentionFunction``) -> ``[B, E]``"""
        from .._hip import ops as _ops
        la = self.local_att
        params = la.packed_params(act)
        keep = torch.is_grad_enabled() and (Q.requires_grad or (K is not None and K.requires_grad) or params.requires_grad)
        hidden = tuple(fc.out_features for fc in la.dnn.linears)
        return _ops.DINAttentionFunction.apply(Q, K, params, tuple(segs), int(T), hidden, act,
                                               bool(self.weight_normalization), lengths, mask, keep)

    def forward(self, query, keys, keys_length, mask=None):
        B, T, E = keys.shape
        valid = self._valid(keys, keys_length, mask)
        needs_grad = torch.is_grad_enabled() and (query.requires_grad or keys.requires_grad or
                                                  any(p.requires_grad for p in self.local_att.parameters()))
        act = self.kernel_route(T, [E], (query, keys), needs_grad)
        if act is None:
            return self._forward_torch(query, keys, valid)
        if self.supports_masking:
            lengths, m8 = None, valid.to(torch.uint8).contiguous()
        else:
            lengths, m8 = keys_length.reshape(-1).to(torch.int32).contiguous(), None
        out = self.fused(query.reshape(B, E), keys.reshape(B, T * E), [(E, 0, 0, E)], T, lengths, m8, act)
        return out.unsqueeze(1)

    def _forward_torch(self, query, keys, valid):
        """the layer's formula as torch ops: scores, mask, optional softmax, weighted sum"""
        score = self.local_att(query, keys).transpose(1, 2)                              # [B, 1, T]
        fill = torch.full_like(score, _SOFTMAX_PAD) if self.weight_normalization else torch.zeros_like(score)
        score = torch.where(valid.unsqueeze(1), score, fill)
        if self.weight_normalization:
            score = torch.softmax(score, dim=-1)
        return score if self.return_score else torch.matmul(score, keys)


GRU_TYPES = ('GRU', 'AIGRU', 'AGRU', 'AUGRU')


def gru_sequence_torch(x, att, lengths, w_ih, w_hh, b_ih, b_hh, gru_type='GRU'):
    """The recurrence ``csrc/gru_seq.hip`` runs (include/dctr.h has the formulas), as torch ops on padded tensors:
    ``x [B, T, H]``, ``att [B, T] | None``, ``lengths [B]`` -> ``(states [B, T, H]`` with zeros beyond a row's length,
    ``last [B, H])``.  A row advances while ``t < clamp(length, 0, T)``; nothing leaves the device."""
    B, T, H = x.shape
    n = lengths.reshape(-1, 1).to(x.device)
    if gru_type == 'AIGRU':
        x = x * att.unsqueeze(-1)
    gi = torch.nn.functional.linear(x, w_ih, b_ih)                                   # off the sequential chain
    h = x.new_zeros((B, H))
    zero, out = h, []
    for t in range(T):
        gh = torch.nn.functional.linear(h, w_hh, b_hh)
        i_r, i_z, i_n = gi[:, t].chunk(3, 1)
        h_r, h_z, h_n = gh.chunk(3, 1)
        r = torch.sigmoid(i_r + h_r)
        c = torch.tanh(i_n + r * h_n)
        if gru_type == 'AGRU':
            u = att[:, t:t + 1]
            new = (1. - u) * h + u * c
        elif gru_type == 'AUGRU':
            u = att[:, t:t + 1] * torch.sigmoid(i_z + h_z)
            new = (1. - u) * h + u * c
        else:
            z = torch.sigmoid(i_z + h_z)
            new = (1. - z) * c + z * h
        on = t < n
        h = torch.where(on, new, h)
        out.append(torch.where(on, new, zero))
    return torch.stack(out, dim=1), h


def gru_sequence(X, segs, T, lengths, att, gru_type, w_ih, w_hh, b_ih, b_hh, want_states=True, want_last=True):
    """``(states [B, T, H] | None, last [B, H] | None)`` of one recurrence over the rows of ``X [B, ld]``, whose input
    segments ``segs = [(dim, x_off, x_step)]`` may lie inside a wider row (the model's gathered row, read in place).

    One kernel per direction (``csrc/gru_seq.hip``, ``_hip/ops.GRUSeqFunction``) when the tensors are float32 on the GPU,
    ``H <= 64``, ``T <= 128``, at most 4 segments and ``DCTR_GRU_SEQ`` is not ``0``; everything else runs
    ``gru_sequence_torch`` on the same operands."""
    import os
    from .._hip import ops as _ops
    dims = [s[0] for s in segs]
    tensors = [X, w_ih, w_hh, b_ih, b_hh] + ([att] if att is not None else [])
    if os.environ.get("DCTR_GRU_SEQ", "1") != "0" and all(t.is_cuda and t.dtype == torch.float32 for t in tensors) and \
            _ops.gru_seq_supported(T, dims, gru_type):
        params = torch.cat([w_ih.reshape(-1), w_hh.reshape(-1), b_ih.reshape(-1), b_hh.reshape(-1)])
        keep = torch.is_grad_enabled() and (X.requires_grad or params.requires_grad or
                                            (att is not None and att.requires_grad))
        return _ops.GRUSeqFunction.apply(X, att if gru_type != 'GRU' else None, params, tuple(tuple(s) for s in segs),
                                         int(T), gru_type, lengths.reshape(-1).to(device=X.device, dtype=torch.int32).contiguous(),
                                         bool(want_states), bool(want_last), keep)
    B = X.shape[0]
    x = torch.cat([torch.stack([X[:, o + t * st:o + t * st + d] for t in range(T)], dim=1) for d, o, st in segs], dim=-1) \
        if not (len(segs) == 1 and segs[0][1] == 0 and segs[0][2] == segs[0][0] and X.shape[1] == T * segs[0][0]) \
        else X.reshape(B, T, segs[0][0])
    states, last = gru_sequence_torch(x, att, lengths.reshape(-1), w_ih, w_hh, b_ih, b_hh, gru_type)
    return (states if want_states else None), (last if want_last else None)


class _AttentionalCell(nn.Module):
    """What AGRUCell and AUGRUCell share: the reference's parameters (``weight_ih | weight_hh [3H, H]``, gate order r, z,
    n; ``bias_ih | bias_hh [3H]`` zero-initialised; the weights are left uninitialised for the owner to fill)."""

    def __init__(self, input_size, hidden_size, bias=True, tie_bias=False):
        super(_AttentionalCell, self).__init__()
        self.input_size, self.hidden_size, self.bias = input_size, hidden_size, bias
        self.weight_ih = nn.Parameter(torch.Tensor(3 * hidden_size, input_size))
        self.weight_hh = nn.Parameter(torch.Tensor(3 * hidden_size, hidden_size))
        if bias:
            self.bias_ih = nn.Parameter(torch.zeros(3 * hidden_size))
            self.bias_hh = nn.Parameter(torch.zeros(3 * hidden_size))
            if tie_bias:
                # the reference registers bias_hh's tensor under the name bias_ih as well (sequence.py:262): ONE Parameter
                # behind both names -- state_dict() lists both keys, named_parameters() yields bias_ih only, and its
                # gradient is the sum of both uses
                self.register_parameter('bias_ih', self.bias_hh)
        else:
            self.register_parameter('bias_ih', None)
            self.register_parameter('bias_hh', None)

    def _gates(self, inputs, hx):
        gi = torch.nn.functional.linear(inputs, self.weight_ih, self.bias_ih)
        gh = torch.nn.functional.linear(hx, self.weight_hh, self.bias_hh)
        return gi.chunk(3, 1), gh.chunk(3, 1)


class AGRUCell(_AttentionalCell):
    """Attention based GRU cell (reference layers/sequence.py:192-235; same constructor): the attention score replaces
    the update gate, ``h' = (1 - a) h + a c``."""

    def __init__(self, input_size, hidden_size, bias=True):
        super(AGRUCell, self).__init__(input_size, hidden_size, bias)

    def forward(self, inputs, hx, att_score):
        (i_r, _, i_n), (h_r, _, h_n) = self._gates(inputs, hx)
        c = torch.tanh(i_n + torch.sigmoid(i_r + h_r) * h_n)
        a = att_score.view(-1, 1)
        return (1. - a) * hx + a * c


class AUGRUCell(_AttentionalCell):
    """GRU cell with attentional update gate (reference layers/sequence.py:238-282; same constructor, the tied bias
    included): ``u = a z; h' = (1 - u) h + u c``."""

    def __init__(self, input_size, hidden_size, bias=True):
        super(AUGRUCell, self).__init__(input_size, hidden_size, bias, tie_bias=True)

    def forward(self, inputs, hx, att_score):
        (i_r, i_z, i_n), (h_r, h_z, h_n) = self._gates(inputs, hx)
        c = torch.tanh(i_n + torch.sigmoid(i_r + h_r) * h_n)
        u = att_score.view(-1, 1) * torch.sigmoid(i_z + h_z)
        return (1. - u) * hx + u * c


class DynamicGRU(nn.Module):
    """AGRU / AUGRU over a sequence (reference layers/sequence.py:285-320; same constructor).

    ``forward(PackedSequence, PackedSequence)`` is the reference's interface for user code and runs the cell step by step
    as torch ops.  The models call ``fused`` on padded tensors: one kernel per direction (``gru_sequence``)."""

    def __init__(self, input_size, hidden_size, bias=True, gru_type='AGRU'):
        super(DynamicGRU, self).__init__()
        self.input_size, self.hidden_size, self.gru_type = input_size, hidden_size, gru_type
        if gru_type == 'AGRU':
            self.rnn = AGRUCell(input_size, hidden_size, bias)
        elif gru_type == 'AUGRU':
            self.rnn = AUGRUCell(input_size, hidden_size, bias)

    def fused(self, X, att, lengths, segs=None, T=None, want_states=False, want_last=True):
        """``X [B, T, H]`` (or rows ``[B, ld]`` with ``segs`` and ``T``), ``att [B, T]``, ``lengths [B]`` ->
        ``(states | None, last | None)``"""
        if segs is None:
            B, T, H = X.shape
            X, segs = X.reshape(B, T * H), [(H, 0, H)]
        c = self.rnn
        zero = c.weight_ih.new_zeros(3 * self.hidden_size)
        return gru_sequence(X, segs, T, lengths, att, self.gru_type, c.weight_ih, c.weight_hh,
                            c.bias_ih if c.bias_ih is not None else zero, c.bias_hh if c.bias_hh is not None else zero,
                            want_states, want_last)

    def forward(self, inputs, att_scores=None, hx=None):
        from torch.nn.utils.rnn import PackedSequence
        if not isinstance(inputs, PackedSequence) or not isinstance(att_scores, PackedSequence):
            raise NotImplementedError("DynamicGRU only supports packed input and att_scores")
        data, batch_sizes, sorted_indices, unsorted_indices = inputs
        scores = att_scores.data
        if hx is None:
            hx = data.new_zeros((int(batch_sizes[0]), self.hidden_size))
        out, begin = [], 0
        for batch in batch_sizes.tolist():
            hx = self.rnn(data[begin:begin + batch], hx[:batch], scores[begin:begin + batch])
            out.append(hx)
            begin += batch
        return PackedSequence(torch.cat(out, dim=0), batch_sizes, sorted_indices, unsorted_indices)


class KMaxPooling(nn.Module):
    """The ``k`` largest values along ``axis``, largest first (the layer of reference layers/sequence.py:157-189; same
    constructor, same two ``ValueError`` texts).  ``ConvLayer`` fuses it with the convolution in front of it
    (``csrc/ccpm.hip``, where equal values keep their order along the axis) and calls this ``forward`` only for inputs
    outside that kernel."""

    def __init__(self, k, axis, device='cpu'):
        super(KMaxPooling, self).__init__()
        self.k, self.axis = k, axis
        self.to(device)

    def forward(self, inputs):
        rank = inputs.dim()
        if not 0 <= self.axis < rank:
            raise ValueError("axis must be 0~%d,now is %d" % (rank - 1, self.axis))
        size = inputs.shape[self.axis]
        if not 1 <= self.k <= size:
            raise ValueError("k must be in 1 ~ %d,now k is %d" % (size, self.k))
        return inputs.topk(self.k, dim=self.axis, largest=True, sorted=True).values
