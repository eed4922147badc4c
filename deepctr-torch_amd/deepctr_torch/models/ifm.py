# -*- coding: utf-8 -*-
"""IFM (reference models/ifm.py:16-87): FM whose embeddings AND first-order weights are re-weighted per sample by an
input-aware factor ``m_x = F * softmax(P . DNN(embeddings))``.

One lookup through the model's own plan in per-field-wide mode (deep rows, per-field first-order weights, the dense half
of Linear), the factor estimating tower on the MFMA kernels reading the gather buffer in place, ``P`` as a library GEMM,
then ONE kernel per direction (csrc/iafm.hip) for the softmax, the two re-weightings, FM and the refined wide sum.  The
tables take the model plan's sparse / lazy update like every other model's."""
import torch.nn as nn

from .basemodel import BaseModel
from .._hip import mlp as _mlp
from .._hip import ops as _ops
from ..inputs import SparseFeat, VarLenSparseFeat
from ..layers import DNN


def _n_sparse(columns):
    return len([c for c in columns if isinstance(c, (SparseFeat, VarLenSparseFeat))]) if len(columns) else 0


class InputAwareFM(BaseModel):
    """What IFM and DIFM share: the per-field-wide model plan, the check of the linear side and the last step."""

    _wide_per_field = True

    def _check_linear_side(self, linear_feature_columns, dnn_feature_columns):
        self.sparse_feat_num = _n_sparse(dnn_feature_columns)
        n_lin = _n_sparse(linear_feature_columns)
        if n_lin not in (0, self.sparse_feat_num):
            # (the reference dies in a broadcast at its first forward: cat of n_lin weights * m_x of sparse_feat_num)
            raise ValueError("linear_feature_columns has %d sparse features, dnn_feature_columns has %d: the input-aware "
                             "factor re-weights them one to one (all or none)" % (n_lin, self.sparse_feat_num))

    def _gather(self, X):
        """(plan, gather buffer [B, ld], per-field wide buffer [B, n + 1] | None, F, D)"""
        plan = self.model_plan()
        if not plan.deep:
            raise ValueError("there are no sparse features")
        if plan.emb_dim <= 0:
            raise ValueError("embedding_dim of SparseFeat and VarlenSparseFeat must be same in this model!")
        full, wide, _ = _ops.embed(plan, X, full=True)
        return plan, full, (wide if plan.has_wide else None), len(plan.deep), plan.emb_dim

    def _estimate(self, net, full, plan):
        """``net(embeddings)``: the tower reads the first F * D columns of the gather buffer (no dense features)."""
        return _mlp.tower(net, None, full, plan.emb_width, sink=self._grad_sink)


class IFM(InputAwareFM):
    """Same arguments as the reference (models/ifm.py:37-42)."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(256, 128), l2_reg_linear=0.00001,
                 l2_reg_embedding=0.00001, l2_reg_dnn=0, init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu',
                 dnn_use_bn=False, task='binary', device='cpu', gpus=None):
        super(IFM, self).__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                                  l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, task=task,
                                  device=device, gpus=gpus)
        if not len(dnn_hidden_units) > 0:
            raise ValueError("dnn_hidden_units is null!")
        self._check_linear_side(linear_feature_columns, dnn_feature_columns)
        self.factor_estimating_net = DNN(self.compute_input_dim(dnn_feature_columns, include_dense=False),
                                         dnn_hidden_units, activation=dnn_activation, l2_reg=l2_reg_dnn,
                                         dropout_rate=dnn_dropout, use_bn=dnn_use_bn, init_std=init_std, device=device)
        self.transform_weight_matrix_P = nn.Linear(dnn_hidden_units[-1], self.sparse_feat_num, bias=False).to(device)
        self.add_regularization_weight(
            [kv for kv in self.factor_estimating_net.named_parameters() if 'weight' in kv[0] and 'bn' not in kv[0]],
            l2=l2_reg_dnn)
        self.add_regularization_weight(self.transform_weight_matrix_P.weight, l2=l2_reg_dnn)
        self.to(device)

    def logit_parts(self, X):
        plan, full, wl, F, D = self._gather(X)
        z = self.transform_weight_matrix_P(self._estimate(self.factor_estimating_net, full, plan))      # m'_x
        y_lin, y_fm = _ops.iafm(full, wl, z, None, True, F, D)
        return [y_lin, y_fm]
