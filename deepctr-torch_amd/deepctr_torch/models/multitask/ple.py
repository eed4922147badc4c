# -*- coding: utf-8 -*-
"""PLE -- Progressive Layered Extraction (reference models/multitask/ple.py): ``num_levels`` levels of Customized Gate
Control.  A level holds ``specific_expert_num`` experts per task and ``shared_expert_num`` shared ones; the gate of task
i mixes task i's experts with the shared ones, the shared gate mixes them all; level l + 1 reads level l's outputs.

Every DNN runs on the MFMA tower kernels.  The ``num_tasks + 1`` gates of a level draw on one pool of expert outputs and
are ONE launch per direction (csrc/gate_mix.hip through ``_hip.ops.gate_mix``), an expert row read once for all the gates
that mix it.  The shared gate of the last level feeds nothing: as in the reference its parameters get no gradient.

Kept from the reference: ``shared_experts`` holds ``specific_expert_num`` modules per level (so the ``state_dict`` keys are
the reference's), and ``forward`` fails with the reference's ``IndexError`` when ``shared_expert_num`` is larger.

The reference's ``.squeeze()`` on the mixed output collapses a batch of one (its ``predict()`` then cannot concatenate
such a tail chunk); here a batch of one gives ``[1, num_tasks]``."""
import torch.nn as nn

from ._base import MultiTaskModel, dnn_weights
from ..._hip import ops as _ops


class PLE(MultiTaskModel):
    """Same arguments as the reference (models/multitask/ple.py:43-47)."""

    def __init__(self, dnn_feature_columns, shared_expert_num=1, specific_expert_num=1, num_levels=2,
                 expert_dnn_hidden_units=(256, 128), gate_dnn_hidden_units=(64,), tower_dnn_hidden_units=(64,),
                 l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0, init_std=0.0001, seed=1024,
                 dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False, task_types=('binary', 'binary'),
                 task_names=('ctr', 'ctcvr'), device='cpu', gpus=None):
        super(PLE, self).__init__([], dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                                  l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, device=device, gpus=gpus)
        self.num_tasks = len(task_names)
        if self.num_tasks <= 1:
            raise ValueError("num_tasks must be greater than 1!")
        self._check_columns_and_types(dnn_feature_columns, task_types)
        self.specific_expert_num = specific_expert_num
        self.shared_expert_num = shared_expert_num
        self.num_levels = num_levels
        self.task_names = task_names
        self.input_dim = self.compute_input_dim(dnn_feature_columns)
        self.expert_dnn_hidden_units = expert_dnn_hidden_units
        self.gate_dnn_hidden_units = gate_dnn_hidden_units
        self.tower_dnn_hidden_units = tower_dnn_hidden_units
        self._l2_reg_dnn = l2_reg_dnn
        T, dim = self.num_tasks, expert_dnn_hidden_units[-1]

        def mk(inputs_dim, hidden_units):
            return self._block(inputs_dim, hidden_units, dnn_activation, l2_reg_dnn, dnn_dropout, dnn_use_bn, init_std,
                               device)

        def level_in(level):
            return self.input_dim if level == 0 else dim

        def grid(groups, per_group, hidden_units):      # [level][group][member]
            return nn.ModuleList([nn.ModuleList([nn.ModuleList([mk(level_in(lv), hidden_units) for _ in range(per_group)])
                                                 for _ in range(groups)]) for lv in range(num_levels)])
        # (generator order decides the weights a seed gives)
        self.specific_experts = grid(T, specific_expert_num, expert_dnn_hidden_units)
        self.shared_experts = grid(1, specific_expert_num, expert_dnn_hidden_units)
        has_gate_dnn = len(gate_dnn_hidden_units) > 0

        def gate_in(level):
            return gate_dnn_hidden_units[-1] if has_gate_dnn else level_in(level)
        if has_gate_dnn:
            self.specific_gate_dnn = grid(T, 1, gate_dnn_hidden_units)
            self.add_regularization_weight(dnn_weights(self.specific_gate_dnn), l2=l2_reg_dnn)
        self.specific_gate_dnn_final_layer = nn.ModuleList(
            [nn.ModuleList([nn.Linear(gate_in(lv), specific_expert_num + shared_expert_num, bias=False) for _ in range(T)])
             for lv in range(num_levels)])
        if has_gate_dnn:
            self.shared_gate_dnn = nn.ModuleList([mk(level_in(lv), gate_dnn_hidden_units) for lv in range(num_levels)])
            self.add_regularization_weight(dnn_weights(self.shared_gate_dnn), l2=l2_reg_dnn)
        self.shared_gate_dnn_final_layer = nn.ModuleList(
            [nn.Linear(gate_in(lv), T * specific_expert_num + shared_expert_num, bias=False) for lv in range(num_levels)])
        self._towers_and_heads(dim, tower_dnn_hidden_units, task_types, mk)
        for module in (self.specific_experts, self.shared_experts, self.specific_gate_dnn_final_layer,
                       self.shared_gate_dnn_final_layer, self.tower_dnn_final_layer):
            self.add_regularization_weight(dnn_weights(module), l2=l2_reg_dnn)
        self.to(device)

    def cgc_net(self, inputs, level_num, K=None):
        """One CGC level: ``inputs`` = one tensor per task + the shared one -> the same for the next level."""
        T, S, Sh = self.num_tasks, self.specific_expert_num, self.shared_expert_num
        pool = [self.run_dnn(self.specific_experts[level_num][i][j], None, inputs[i], K)
                for i in range(T) for j in range(S)]
        pool += [self.run_dnn(self.shared_experts[level_num][0][k], None, inputs[-1], K) for k in range(Sh)]
        shared = tuple(range(T * S, T * S + Sh))
        members = [tuple(range(i * S, (i + 1) * S)) + shared for i in range(T)] + [tuple(range(T * S + Sh))]
        weights = [fc.weight for fc in self.specific_gate_dnn_final_layer[level_num]] + \
            [self.shared_gate_dnn_final_layer[level_num].weight]
        if len(self.gate_dnn_hidden_units) > 0:
            dnns = [self.specific_gate_dnn[level_num][i][0] for i in range(T)] + [self.shared_gate_dnn[level_num]]
            gate_in = [self.run_dnn(dnn, None, x, K) for dnn, x in zip(dnns, inputs)]
        else:
            gate_in = [x if K is None else x[:, :K] for x in inputs]
        return _ops.gate_mix(pool, gate_in, weights, members)

    def forward(self, X):
        x, K = self.dnn_input(X)
        level = [x] * (self.num_tasks + 1)
        for lv in range(self.num_levels):
            level = self.cgc_net(level, lv, K if lv == 0 else None)
        return self.task_outputs(level)
