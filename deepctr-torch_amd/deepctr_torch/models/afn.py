# -*- coding: utf-8 -*-
"""AFN -- Adaptive Factorization Network, the non-ensembled version (reference models/afn.py:17-74): the embeddings go
through the logarithmic transformation layer, whose neurons are products of powers of the fields, then a DNN with
BatchNorm and a biased 1-unit projection.

Forward = the fused gather (embeddings + linear logit), ``LogTransformLayer`` on the gathered rows in place
(csrc/log_transform.hip), then ``afn_dnn`` / ``afn_dnn_linear`` as the modules they are (the tower has BatchNorm)."""
import torch.nn as nn

from .basemodel import BaseModel
from ..layers import DNN, LogTransformLayer


class AFN(BaseModel):
    """Same arguments as the reference (models/afn.py:40-45).  Dense ``dnn_feature_columns`` are ignored, as there."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, ltl_hidden_size=256, afn_dnn_hidden_units=(256, 128),
                 l2_reg_linear=0.00001, l2_reg_embedding=0.00001, l2_reg_dnn=0, init_std=0.0001, seed=1024,
                 dnn_dropout=0, dnn_activation='relu', task='binary', device='cpu', gpus=None):
        super(AFN, self).__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                                  l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, task=task,
                                  device=device, gpus=gpus)
        # (generator order decides the weights a seed gives: the transformation layer, the tower, its projection)
        self.ltl = LogTransformLayer(len(self.embedding_dict), self.embedding_size, ltl_hidden_size)
        self.afn_dnn = DNN(self.embedding_size * ltl_hidden_size, afn_dnn_hidden_units, activation=dnn_activation,
                           l2_reg=l2_reg_dnn, dropout_rate=dnn_dropout, use_bn=True, init_std=init_std, device=device)
        self.afn_dnn_linear = nn.Linear(afn_dnn_hidden_units[-1], 1)
        self.to(device)

    def logit_parts(self, X):
        plan = self.model_plan()
        n_fields = len(plan.deep)
        if n_fields == 0:
            raise ValueError('Sparse embeddings not provided. AFN only accepts sparse embeddings as input.')
        if n_fields != len(self.embedding_dict):
            raise ValueError("AFN needs one embedding table per embedded field: %d fields share %d tables (a column with "
                             "embedding_name set to another's)" % (n_fields, len(self.embedding_dict)))
        gathered, logit, _ = self.fused_inputs(X)
        emb = gathered[:, :plan.emb_width].view(X.shape[0], n_fields, plan.emb_dim)
        hidden = self.afn_dnn(self.ltl(emb))
        return [logit, self.afn_dnn_linear(hidden)]
