# -*- coding: utf-8 -*-
"""SharedBottom (reference models/multitask/sharedbottom.py): one bottom DNN, one tower and head per task.  Every DNN
runs on the MFMA tower kernels, each tower together with its 1-unit projection.

A batch of one gives ``[1, num_tasks]`` (the reference, too, for this model)."""
from ._base import MultiTaskModel, dnn_weights


class SharedBottom(MultiTaskModel):
    """Same arguments as the reference (models/multitask/sharedbottom.py:39-42)."""

    def __init__(self, dnn_feature_columns, bottom_dnn_hidden_units=(256, 128), tower_dnn_hidden_units=(64,),
                 l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0, init_std=0.0001, seed=1024,
                 dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False, task_types=('binary', 'binary'),
                 task_names=('ctr', 'ctcvr'), device='cpu', gpus=None):
        super(SharedBottom, self).__init__([], dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                                           l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, device=device,
                                           gpus=gpus)
        self.num_tasks = len(task_names)
        if self.num_tasks <= 1:
            raise ValueError("num_tasks must be greater than 1")
        self._check_columns_and_types(dnn_feature_columns, task_types)
        self.task_names = task_names
        self.input_dim = self.compute_input_dim(dnn_feature_columns)
        self.bottom_dnn_hidden_units = bottom_dnn_hidden_units
        self.tower_dnn_hidden_units = tower_dnn_hidden_units
        self._l2_reg_dnn = l2_reg_dnn

        def mk(inputs_dim, hidden_units):     # (the reference leaves these DNNs' own l2_reg at its default)
            return self._block(inputs_dim, hidden_units, dnn_activation, None, dnn_dropout, dnn_use_bn, init_std, device)
        self.bottom_dnn = mk(self.input_dim, bottom_dnn_hidden_units)
        self._towers_and_heads(bottom_dnn_hidden_units[-1], tower_dnn_hidden_units, task_types, mk)
        self.add_regularization_weight(dnn_weights(self.bottom_dnn), l2=l2_reg_dnn)
        self.add_regularization_weight(dnn_weights(self.tower_dnn_final_layer), l2=l2_reg_dnn)
        self.to(device)

    def forward(self, X):
        x, K = self.dnn_input(X)
        bottom = self.run_dnn(self.bottom_dnn, None, x, K)
        return self.task_outputs([bottom] * self.num_tasks)
