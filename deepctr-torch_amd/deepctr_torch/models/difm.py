# -*- coding: utf-8 -*-
"""DIFM (reference models/difm.py:16-106): IFM with a dual input-aware factor ``m_x = m_vec + m_bit`` -- a vector-wise
part from multi-head self-attention over the fields and a bit-wise part from a DNN.

The lookup, the bit-wise tower and the last step are IFM's (models/ifm.py); the vector-wise part is the InteractingLayer
kernel of AutoInt (csrc/interact.hip) on the gather buffer's field block, the two ``P`` projections are library GEMMs."""
import torch.nn as nn

from .ifm import InputAwareFM
from .._hip import ops as _ops
from ..layers import DNN, InteractingLayer


class DIFM(InputAwareFM):
    """Same arguments as the reference (models/difm.py:39-44)."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, att_head_num=4, att_res=True,
                 dnn_hidden_units=(256, 128), l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0,
                 init_std=0.0001, seed=1024, dnn_dropout=0, dnn_activation='relu', dnn_use_bn=False, task='binary',
                 device='cpu', gpus=None):
        super(DIFM, self).__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                                   l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, task=task,
                                   device=device, gpus=gpus)
        if not len(dnn_hidden_units) > 0:
            raise ValueError("dnn_hidden_units is null!")
        self._check_linear_side(linear_feature_columns, dnn_feature_columns)
        self.vector_wise_net = InteractingLayer(self.embedding_size, att_head_num, att_res, scaling=True, device=device)
        self.bit_wise_net = DNN(self.compute_input_dim(dnn_feature_columns, include_dense=False), dnn_hidden_units,
                                activation=dnn_activation, l2_reg=l2_reg_dnn, dropout_rate=dnn_dropout, use_bn=dnn_use_bn,
                                init_std=init_std, device=device)
        self.transform_matrix_P_vec = nn.Linear(self.sparse_feat_num * self.embedding_size, self.sparse_feat_num,
                                                bias=False).to(device)
        self.transform_matrix_P_bit = nn.Linear(dnn_hidden_units[-1], self.sparse_feat_num, bias=False).to(device)
        self.add_regularization_weight(
            [kv for kv in self.vector_wise_net.named_parameters() if 'weight' in kv[0] and 'bn' not in kv[0]],
            l2=l2_reg_dnn)
        self.add_regularization_weight(
            [kv for kv in self.bit_wise_net.named_parameters() if 'weight' in kv[0] and 'bn' not in kv[0]], l2=l2_reg_dnn)
        self.add_regularization_weight(self.transform_matrix_P_vec.weight, l2=l2_reg_dnn)
        self.add_regularization_weight(self.transform_matrix_P_bit.weight, l2=l2_reg_dnn)
        self.to(device)

    def logit_parts(self, X):
        plan, full, wl, F, D = self._gather(X)
        att = self.vector_wise_net(full[:, :plan.emb_width].reshape(X.shape[0], F, D))
        m_vec = self.transform_matrix_P_vec(att.reshape(X.shape[0], F * D))
        m_bit = self.transform_matrix_P_bit(self._estimate(self.bit_wise_net, full, plan))
        y_lin, y_fm = _ops.iafm(full, wl, m_vec, m_bit, False, F, D)
        return [y_lin, y_fm]
