# -*- coding: utf-8 -*-
"""MMOE -- Multi-gate Mixture-of-Experts (reference models/multitask/mmoe.py): ``num_experts`` expert DNNs over the
embeddings, one softmax gate per task mixing them, one tower and head per task.

Every DNN runs on the MFMA tower kernels; ALL gates are one launch per direction (csrc/gate_mix.hip through
``_hip.ops.gate_mix``): the reference's Linear / softmax / stack / matmul per gate and its ``[B, experts, dim]`` copy
of the expert outputs do not exist here.

The reference's ``.squeeze()`` on the mixed output collapses a batch of one (its ``predict()`` then cannot concatenate
such a tail chunk); here a batch of one gives ``[1, num_tasks]``."""
import torch.nn as nn

from ._base import MultiTaskModel, dnn_weights
from ..._hip import ops as _ops


class MMOE(MultiTaskModel):
    """Same arguments as the reference (models/multitask/mmoe.py:41-45)."""

    def __init__(self, dnn_feature_columns, num_experts=3, expert_dnn_hidden_units=(256, 128),
                 gate_dnn_hidden_units=(64,), tower_dnn_hidden_units=(64,), l2_reg_linear=0.00001,
                 l2_reg_embedding=0.00001, l2_reg_dnn=0, init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu',
                 dnn_use_bn=False, task_types=('binary', 'binary'), task_names=('ctr', 'ctcvr'), device='cpu', gpus=None):
        super(MMOE, self).__init__([], dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                                   l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, device=device,
                                   gpus=gpus)
        self.num_tasks = len(task_names)
        if self.num_tasks <= 1:
            raise ValueError("num_tasks must be greater than 1")
        if num_experts <= 1:
            raise ValueError("num_experts must be greater than 1")
        self._check_columns_and_types(dnn_feature_columns, task_types)
        self.num_experts = num_experts
        self.task_names = task_names
        self.input_dim = self.compute_input_dim(dnn_feature_columns)
        self.expert_dnn_hidden_units = expert_dnn_hidden_units
        self.gate_dnn_hidden_units = gate_dnn_hidden_units
        self.tower_dnn_hidden_units = tower_dnn_hidden_units
        self._l2_reg_dnn = l2_reg_dnn

        def mk(inputs_dim, hidden_units):
            return self._block(inputs_dim, hidden_units, dnn_activation, l2_reg_dnn, dnn_dropout, dnn_use_bn, init_std,
                               device)
        # (generator order decides the weights a seed gives: experts, gate DNNs, gate projections, towers, projections)
        self.expert_dnn = nn.ModuleList([mk(self.input_dim, expert_dnn_hidden_units) for _ in range(num_experts)])
        gate_in = self.input_dim
        if len(gate_dnn_hidden_units) > 0:
            self.gate_dnn = nn.ModuleList([mk(self.input_dim, gate_dnn_hidden_units) for _ in range(self.num_tasks)])
            self.add_regularization_weight(dnn_weights(self.gate_dnn), l2=l2_reg_dnn)
            gate_in = gate_dnn_hidden_units[-1]
        self.gate_dnn_final_layer = nn.ModuleList([nn.Linear(gate_in, num_experts, bias=False)
                                                   for _ in range(self.num_tasks)])
        self._towers_and_heads(expert_dnn_hidden_units[-1], tower_dnn_hidden_units, task_types, mk)
        for module in (self.expert_dnn, self.gate_dnn_final_layer, self.tower_dnn_final_layer):
            self.add_regularization_weight(dnn_weights(module), l2=l2_reg_dnn)
        self.to(device)

    def forward(self, X):
        x, K = self.dnn_input(X)
        experts = [self.run_dnn(dnn, None, x, K) for dnn in self.expert_dnn]
        if len(self.gate_dnn_hidden_units) > 0:
            gate_in = [self.run_dnn(dnn, None, x, K) for dnn in self.gate_dnn]
        else:
            gate_in = [x[:, :K]] * self.num_tasks
        every = tuple(range(self.num_experts))
        mixed = _ops.gate_mix(experts, gate_in, [fc.weight for fc in self.gate_dnn_final_layer],
                              [every] * self.num_tasks)
        return self.task_outputs(mixed)
