# -*- coding: utf-8 -*-
"""What the four multi-task models share: the task checks of their constructors, the DNN blocks on the MFMA tower kernels,
the heads, and the refusal of the distributed ``fit()``."""
import torch
import torch.nn as nn

from ..basemodel import BaseModel
from ..._hip import mlp as _mlp
from ...layers import DNN, PredictionLayer


def dnn_weights(module):
    """the parameters a DNN block's L2 term covers: every weight that is not a BatchNorm's"""
    return [kv for kv in module.named_parameters() if 'weight' in kv[0] and 'bn' not in kv[0]]


class MultiTaskModel(BaseModel):
    """``BaseModel`` without a wide part (``linear_feature_columns=[]``) and with ``num_tasks`` outputs.  The train step
    is BaseModel's autograd route: one loss per task, summed (``compile(optimizer, [loss_0, loss_1, ...])``)."""

    def _check_columns_and_types(self, dnn_feature_columns, task_types, allowed=('binary', 'regression'),
                                 message="task must be binary or regression, {} is illegal"):
        if len(dnn_feature_columns) == 0:
            raise ValueError("dnn_feature_columns is null!")
        if len(task_types) != self.num_tasks:
            raise ValueError("num_tasks must be equal to the length of task_types")
        for task_type in task_types:
            if task_type not in allowed:
                raise ValueError(message.format(task_type))

    def _block(self, inputs_dim, hidden_units, activation, l2_reg, dropout, use_bn, init_std, device):
        """a DNN block; ``l2_reg`` None leaves the DNN's own ``l2_reg`` at its default, as SharedBottom and ESMM do"""
        return DNN(inputs_dim, hidden_units, activation=activation, dropout_rate=dropout, use_bn=use_bn,
                   init_std=init_std, device=device, **({"l2_reg": l2_reg} if l2_reg is not None else {}))

    def _towers_and_heads(self, in_features, tower_dnn_hidden_units, task_types, mk):
        """``tower_dnn`` (when it has layers, with its L2 group), ``tower_dnn_final_layer`` and ``out``, constructed in the
        reference's order."""
        if len(tower_dnn_hidden_units) > 0:
            self.tower_dnn = nn.ModuleList([mk(in_features, tower_dnn_hidden_units) for _ in range(self.num_tasks)])
            self.add_regularization_weight(dnn_weights(self.tower_dnn), l2=self._l2_reg_dnn)
        self.tower_dnn_final_layer = nn.ModuleList(
            [nn.Linear(tower_dnn_hidden_units[-1] if len(tower_dnn_hidden_units) > 0 else in_features, 1, bias=False)
             for _ in range(self.num_tasks)])
        self.out = nn.ModuleList([PredictionLayer(task) for task in task_types])

    def dnn_input(self, X):
        """(the gathered ``[B, ld]`` buffer, K): its first K columns are the reference's ``combined_dnn_input``.  The
        towers read the buffer in place, so the embedding update sees ONE summed gradient of its shape."""
        plan = self.model_plan()
        x, _, _ = self.fused_inputs(X, full=True)
        return x, plan.width

    @staticmethod
    def run_dnn(dnn, final, x, K=None):
        """``final(dnn(x[:, :K]))`` -- ``dnn(x[:, :K])`` without ``final`` -- on the tower kernels (the modules themselves
        under BatchNorm, active dropout or another activation than relu)."""
        return _mlp.tower(dnn, final, x, K)

    def task_outputs(self, task_inputs):
        """towers, 1-unit projections and heads over one ``[B, dim]`` tensor per task -> ``[B, num_tasks]``"""
        outs = []
        for i in range(self.num_tasks):
            if len(self.tower_dnn_hidden_units) > 0:
                logit = self.run_dnn(self.tower_dnn[i], self.tower_dnn_final_layer[i], task_inputs[i])
            else:
                logit = self.tower_dnn_final_layer[i](task_inputs[i])
            outs.append(self.out[i](logit))
        return torch.cat(outs, -1)

    def fit(self, *args, **kwargs):
        from ... import distributed_fit as _dfit
        if _dfit.context() is not None:      # (looks at WORLD_SIZE / an existing group only: creates nothing)
            raise NotImplementedError(
                "%s.fit() under several ranks (WORLD_SIZE > 1) is not implemented: the table-sharded and the replicated "
                "trainers step one binary task; train a multi-task model in one process" % type(self).__name__)
        return super(MultiTaskModel, self).fit(*args, **kwargs)
