# -*- coding: utf-8 -*-
"""CCPM -- Convolutional Click Prediction Model (reference models/ccpm.py:21-83): the embeddings stacked as a
``[F, D]`` image, convolved along the field axis with k-max pooling between the layers, then the DNN.

Forward = the fused gather (embeddings + linear logit), ONE kernel for the whole ``ConvLayer`` (csrc/ccpm.hip) and the MFMA
tower on its flattened output."""
from .basemodel import BaseModel
from ..inputs import DenseFeat
from ..layers import ConvLayer


class CCPM(BaseModel):
    """Same arguments as the reference (models/ccpm.py:42-45)."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, conv_kernel_width=(6, 5), conv_filters=(4, 4),
                 dnn_hidden_units=(256,), l2_reg_linear=1e-5, l2_reg_embedding=1e-5, l2_reg_dnn=0, dnn_dropout=0,
                 init_std=0.0001, seed=1024, task='binary', device='cpu', dnn_use_bn=False, dnn_activation='relu',
                 gpus=None):
        super(CCPM, self).__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                                   l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, task=task,
                                   device=device, gpus=gpus)
        if any(isinstance(c, DenseFeat) for c in dnn_feature_columns):   # reference: support_dense=False, ccpm.py:71-72
            raise ValueError("DenseFeat is not supported in dnn_feature_columns")
        if len(conv_kernel_width) != len(conv_filters):
            raise ValueError("conv_kernel_width must have same element with conv_filters")
        # (generator order decides the weights a seed gives: the conv stack, then the tower, then its projection)
        n_fields = self.compute_input_dim(dnn_feature_columns, include_dense=False, feature_group=True)
        self.conv_layer = ConvLayer(n_fields, conv_kernel_width, conv_filters, device=device)
        self.dnn_input_dim = conv_filters[-1] * self.conv_layer.filed_shape * self.embedding_size   # [C_L, k_L, D] flattened
        self._make_tower(self.dnn_input_dim, dnn_hidden_units, activation=dnn_activation, l2_reg_dnn=l2_reg_dnn,
                         dropout=dnn_dropout, use_bn=dnn_use_bn, init_std=init_std, device=device)
        self.to(device)

    def logit_parts(self, X):
        plan = self.model_plan()
        if len(plan.deep) == 0:
            raise ValueError("must have the embedding feature,now the embedding feature is None!")
        if plan.emb_dim <= 0:
            raise ValueError("embedding_dim of SparseFeat and VarlenSparseFeat must be same in this model!")
        gathered, logit, _ = self.fused_inputs(X)
        emb = gathered[:, :plan.emb_width].reshape(X.shape[0], 1, len(plan.deep), plan.emb_dim)
        pooled = self.conv_layer(emb)
        return [logit, self.tower_logit(pooled.reshape(X.shape[0], -1))]
