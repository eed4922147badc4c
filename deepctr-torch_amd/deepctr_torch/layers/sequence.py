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
