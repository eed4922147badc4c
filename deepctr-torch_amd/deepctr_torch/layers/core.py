"""MLP tower and prediction head (boundary: PyTorch-ROCm ``nn.Linear`` -> hipBLASLt fp32).
Same parameters / ``state_dict`` keys as the reference (layers/core.py:67-160)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .activation import activation_layer


class DNN(nn.Module):
    """``hidden_units`` fully connected layers: Linear -> [BatchNorm] -> activation -> Dropout
    (reference layers/core.py:67-134).  Weights N(0, init_std); biases keep nn.Linear's default."""

    def __init__(self, inputs_dim, hidden_units, activation='relu', l2_reg=0, dropout_rate=0, use_bn=False,
                 init_std=0.0001, dice_dim=3, seed=1024, device='cpu'):
        super(DNN, self).__init__()
        if len(hidden_units) == 0:
            raise ValueError("hidden_units is empty!!")
        self.dropout_rate, self.seed, self.l2_reg, self.use_bn = dropout_rate, seed, l2_reg, use_bn
        self.dropout = nn.Dropout(dropout_rate)
        widths = [inputs_dim] + list(hidden_units)
        self.linears = nn.ModuleList(nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))
        if use_bn:
            self.bn = nn.ModuleList(nn.BatchNorm1d(b) for b in widths[1:])
        self.activation_layers = nn.ModuleList(activation_layer(activation, b, dice_dim) for b in widths[1:])
        for name, tensor in self.linears.named_parameters():
            if 'weight' in name:
                nn.init.normal_(tensor, mean=0, std=init_std)
        self.to(device)

    def forward(self, inputs):
        h = inputs
        for i, fc in enumerate(self.linears):
            h = fc(h)
            if self.use_bn:
                h = self.bn[i](h)
            h = self.dropout(self.activation_layers[i](h))
        return h


class LocalActivationUnit(nn.Module):
    """DIN's local activation unit (reference layers/core.py:10-64; same constructor, defaults and ``state_dict`` keys):
    every behaviour ``k_t`` is scored against the candidate ``q`` by a small MLP on ``[q, k_t, q - k_t, q * k_t]`` and a
    1-unit ``dense``.  ``forward(query [B, 1, E], user_behavior [B, T, E]) -> [B, T, 1]`` states that formula as torch
    ops; ``AttentionSequencePoolingLayer`` runs it fused with the mask, the softmax and the weighted sum
    (``csrc/din.hip``) and reads this module's parameters through ``packed_params``."""

    def __init__(self, hidden_units=(64, 32), embedding_dim=4, activation='sigmoid', dropout_rate=0, dice_dim=3,
                 l2_reg=0, use_bn=False):
        super(LocalActivationUnit, self).__init__()
        self.dnn = DNN(inputs_dim=4 * embedding_dim, hidden_units=hidden_units, activation=activation, l2_reg=l2_reg,
                       dropout_rate=dropout_rate, dice_dim=dice_dim, use_bn=use_bn)
        self.dense = nn.Linear(hidden_units[-1], 1)

    def forward(self, query, user_behavior):
        q = query.expand(-1, user_behavior.size(1), -1)
        return self.dense(self.dnn(torch.cat([q, user_behavior, q - user_behavior, q * user_behavior], dim=-1)))

    def kernel_activation(self):
        """The kernel's name for this unit's activation (``_hip/ops.DIN_ACT``) or None when it has none for it, the
        attention net has BatchNorm layers or dropout is active.  ``'dice'`` is the FROZEN form: the caller may take it
        only in eval mode and when no gradient is needed."""
        from .activation import Dice, Identity
        if self.dnn.use_bn or (self.dnn.dropout_rate > 0 and self.training):
            return None
        kinds = set(type(m) for m in self.dnn.activation_layers)
        if len(kinds) != 1:
            return None
        name = {nn.Sigmoid: "sigmoid", nn.ReLU: "relu", Identity: "linear", nn.PReLU: "prelu", Dice: "dice"}.get(kinds.pop())
        if name == "prelu" and any(m.weight.numel() != 1 for m in self.dnn.activation_layers):
            return None
        if name == "dice" and any(m.dim != 3 for m in self.dnn.activation_layers):
            return None
        return name

    def packed_params(self, act):
        """The one vector ``dctr_din_attn_fwd`` reads (include/dctr.h): per hidden layer the weight, the bias and the
        activation's own -- prelu's slope, or for frozen Dice ``alpha | s | t`` with BatchNorm's running statistics,
        affine pair and eps folded into ``sigmoid(s * z + t)`` -- then ``dense.weight`` and ``dense.bias``."""
        parts = []
        for fc, a in zip(self.dnn.linears, self.dnn.activation_layers):
            parts += [fc.weight.reshape(-1), fc.bias]
            if act == "prelu":
                parts.append(a.weight.reshape(-1))
            elif act == "dice":
                bn = a.bn
                s = (bn.weight if bn.affine else torch.ones_like(bn.running_var)) / torch.sqrt(bn.running_var + bn.eps)
                t = (bn.bias if bn.affine else torch.zeros_like(bn.running_mean)) - bn.running_mean * s
                parts += [a.alpha.reshape(-1), s, t]
        parts += [self.dense.weight.reshape(-1), self.dense.bias]
        return torch.cat(parts)


class PredictionLayer(nn.Module):
    """``sigmoid(logit + bias)`` for task='binary', ``logit + bias`` otherwise
    (reference layers/core.py:137-160)."""

    def __init__(self, task='binary', use_bias=True, **kwargs):
        if task not in ["binary", "multiclass", "regression"]:
            raise ValueError("task must be binary,multiclass or regression")
        super(PredictionLayer, self).__init__()
        self.use_bias, self.task = use_bias, task
        if use_bias:
            self.bias = nn.Parameter(torch.zeros((1,)))

    def forward(self, X):
        out = X + self.bias if self.use_bias else X
        return torch.sigmoid(out) if self.task == "binary" else out


def same_padding(size, kernel, stride=1, dilation=1):
    """``(before, after)`` zeros along one axis under TensorFlow's 'SAME' rule: as many as a window of ``kernel`` taps
    needs to produce ``ceil(size / stride)`` outputs, split evenly, the odd one going AFTER the data."""
    outputs = -(-size // stride)
    total = max((outputs - 1) * stride + (kernel - 1) * dilation + 1 - size, 0)
    return total // 2, total - total // 2


class Conv2dSame(nn.Conv2d):
    """``nn.Conv2d`` under 'SAME' padding (the layer of reference layers/core.py:163-185; same constructor -- its
    ``padding`` argument is accepted and unused, as there): the zeros of ``same_padding`` are put around the input, then
    the unpadded convolution runs.  Construction draws ``nn.Conv2d``'s own initialisation and then ``xavier_uniform_`` on
    the weight, the order in which the reference consumes the generator.  ``ConvLayer`` runs its whole stack as one kernel
    and calls this ``forward`` only for inputs outside it."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True):
        nn.Conv2d.__init__(self, in_channels, out_channels, kernel_size, stride=stride, padding=0, dilation=dilation,
                           groups=groups, bias=bias)
        nn.init.xavier_uniform_(self.weight)

    def forward(self, x):
        rows, cols = (same_padding(x.shape[ax - 2], self.kernel_size[ax], self.stride[ax], self.dilation[ax])
                      for ax in (0, 1))
        if any(rows + cols):
            x = F.pad(x, cols + rows)                     # (F.pad lists the last axis first)
        return self._conv_forward(x, self.weight, self.bias)
