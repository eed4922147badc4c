# -*- coding: utf-8 -*-
"""ESMM -- Entire Space Multi-task Model (reference models/multitask/esmm.py): a CTR and a CVR tower over the same
embeddings, one shared head, ``ctcvr = ctr * cvr``.  Both towers run on the MFMA tower kernels with their projections.

A batch of one gives ``[1, 2]``."""
import torch
import torch.nn as nn

from ._base import MultiTaskModel, dnn_weights


class ESMM(MultiTaskModel):
    """Same arguments as the reference (models/multitask/esmm.py:38-41)."""

    def __init__(self, dnn_feature_columns, tower_dnn_hidden_units=(256, 128), l2_reg_linear=0.00001,
                 l2_reg_embedding=0.00001, l2_reg_dnn=0, init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu',
                 dnn_use_bn=False, task_types=('binary', 'binary'), task_names=('ctr', 'ctcvr'), device='cpu', gpus=None):
        super(ESMM, self).__init__([], dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                                   l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, task='binary',
                                   device=device, gpus=gpus)
        self.num_tasks = len(task_names)
        if self.num_tasks != 2:
            raise ValueError("the length of task_names must be equal to 2")
        self._check_columns_and_types(dnn_feature_columns, task_types, allowed=('binary',),
                                      message="task must be binary in ESMM, {} is illegal")
        input_dim = self.compute_input_dim(dnn_feature_columns)
        self.ctr_dnn, self.cvr_dnn = (self._block(input_dim, tower_dnn_hidden_units, dnn_activation, None, dnn_dropout,
                                                  dnn_use_bn, init_std, device) for _ in range(2))
        self.ctr_dnn_final_layer = nn.Linear(tower_dnn_hidden_units[-1], 1, bias=False)
        self.cvr_dnn_final_layer = nn.Linear(tower_dnn_hidden_units[-1], 1, bias=False)
        self.add_regularization_weight(dnn_weights(self.ctr_dnn), l2=l2_reg_dnn)
        self.add_regularization_weight(dnn_weights(self.cvr_dnn), l2=l2_reg_dnn)
        self.add_regularization_weight(self.ctr_dnn_final_layer.weight, l2=l2_reg_dnn)
        self.add_regularization_weight(self.cvr_dnn_final_layer.weight, l2=l2_reg_dnn)
        self.to(device)

    def forward(self, X):
        x, K = self.dnn_input(X)
        ctr = self.out(self.run_dnn(self.ctr_dnn, self.ctr_dnn_final_layer, x, K))
        cvr = self.out(self.run_dnn(self.cvr_dnn, self.cvr_dnn_final_layer, x, K))
        return torch.cat([ctr, ctr * cvr], -1)
