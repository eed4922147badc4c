# -*- coding: utf-8 -*-
"""ONN -- Operation-aware Neural Networks, also known as NFFM (reference models/onn.py:14-158): every ordered pair
(i < j) of sparse features owns two tables, ``emb1`` indexed by feature i's id and ``emb2`` by feature j's; the DNN reads
the concatenation of the P = F (F - 1) / 2 elementwise products followed by the dense values.

The reference runs 2 P ``nn.Embedding`` calls, P multiplies and a ``cat`` (and 2 P dense ``[V, D]`` gradients backward);
here the model plan is a PAIR plan over the 2 P tables and the first-order tables, and ONE launch per direction
(csrc/pair_embed.hip) reads a sample's ids once, fetches both rows of every pair and writes only their product -- in the
DNN-input layout the MFMA tower reads in place.  The backward hands row gradients to the same sorted / lazy table updates
every other model's lookup uses.  ``embedding_dict`` exists (``BaseModel`` creates it, ``state_dict`` carries it, L2 counts
it) but, as in the reference, the output never depends on it: it is never looked up."""
import torch.nn as nn

from .basemodel import BaseModel
from .._hip import ops as _ops
from .._hip.plan import EmbeddingPlan
from ..inputs import DenseFeat, SparseFeat
from ..layers import DNN


class Interac(nn.Module):
    """Parameter holder of one pair (reference models/onn.py:14-34): ``emb1`` / ``emb2`` with the reference's
    initialisation -- both drawn N(0, 1) by ``nn.Embedding``, then ``emb1`` re-drawn with ``std = init_std``."""

    def __init__(self, first_size, second_size, emb_size, init_std, sparse=False):
        super(Interac, self).__init__()
        self.emb1 = nn.Embedding(first_size, emb_size, sparse=sparse)
        self.emb2 = nn.Embedding(second_size, emb_size, sparse=sparse)
        nn.init.normal_(self.emb1.weight, mean=0, std=init_std)

    def forward(self, first, second):
        return self.emb1(first) * self.emb2(second)


def _sparse_columns(feature_columns):
    # (isinstance, like the reference: a VarLenSparseFeat is no SparseFeat -- the second order ignores it)
    return [c for c in feature_columns if isinstance(c, SparseFeat)] if len(feature_columns) else []


class ONN(BaseModel):
    """Same arguments as the reference (models/onn.py:58-62)."""

    def __init__(self, linear_feature_columns, dnn_feature_columns, dnn_hidden_units=(128, 128), l2_reg_embedding=1e-5,
                 l2_reg_linear=1e-5, l2_reg_dnn=0, dnn_dropout=0, init_std=0.0001, seed=1024, dnn_use_bn=False,
                 dnn_activation='relu', task='binary', device='cpu', gpus=None):
        super(ONN, self).__init__(linear_feature_columns, dnn_feature_columns, l2_reg_linear=l2_reg_linear,
                                  l2_reg_embedding=l2_reg_embedding, init_std=init_std, seed=seed, task=task,
                                  device=device, gpus=gpus)
        sparse = _sparse_columns(dnn_feature_columns)
        names = [c.embedding_name for c in sparse]
        # The reference keys both the pair tables and its ``feature_index`` lookups by embedding_name: a column whose
        # embedding_name is not its name dies there with a KeyError at the first forward, two columns sharing one
        # silently share (and overwrite) pair tables.
        if any(c.embedding_name != c.name for c in sparse) or len(set(names)) != len(names):
            raise ValueError("ONN needs every SparseFeat of dnn_feature_columns to have an embedding_name of its own "
                             "equal to its name (the pair tables are keyed by it)")
        embedding_size = self.embedding_size
        # (init_std of the pair tables is the helper's default in the reference, models/onn.py:122 -- not the model's)
        pairs = nn.ModuleDict()
        for i in range(len(sparse) - 1):
            for j in range(i + 1, len(sparse)):
                pairs[names[i] + "+" + names[j]] = Interac(sparse[i].vocabulary_size, sparse[j].vocabulary_size,
                                                           emb_size=embedding_size, init_std=0.0001)
        self.second_order_embedding_dict = pairs.to(device)
        self.add_regularization_weight(self.second_order_embedding_dict.parameters(), l2=l2_reg_embedding)
        self._n_embedding_reg_groups = 3        # (embedding_dict, linear_model, the pair tables)
        self._pair_columns = [(names[i], names[j]) for i in range(len(sparse) - 1) for j in range(i + 1, len(sparse))]
        dense_dim = sum(c.dimension for c in dnn_feature_columns if isinstance(c, DenseFeat)) \
            if len(dnn_feature_columns) else 0
        dim = int(len(sparse) * (len(sparse) - 1) / 2 * embedding_size + dense_dim)
        self.dnn = DNN(dim, dnn_hidden_units, activation=dnn_activation, l2_reg=l2_reg_dnn, dropout_rate=dnn_dropout,
                       use_bn=dnn_use_bn, init_std=init_std, device=device)
        self.dnn_linear = nn.Linear(dnn_hidden_units[-1], 1, bias=False).to(device)
        self.add_regularization_weight(
            [kv for kv in self.dnn.named_parameters() if 'weight' in kv[0] and 'bn' not in kv[0]], l2=l2_reg_dnn)
        self.add_regularization_weight(self.dnn_linear.weight, l2=l2_reg_dnn)
        self.to(device)

    def _build_plan(self):
        """The PAIR plan: deep side = ``emb1`` / ``emb2`` of every pair (fields 2p / 2p + 1, reference pair order) over
        the X columns of the pair's two features, wide side = ``linear_feature_columns`` as for every model.  Its tables --
        the pair tables and the first-order tables -- are what the update paths see; of the ModuleDicts only the first-order
        one holds tables of it (``embedding_dict`` is never looked up)."""
        lm = self.linear_model
        fields = []
        for a, b in self._pair_columns:
            mod = self.second_order_embedding_dict[a + "+" + b]
            fields.append((a + "+" + b + ".emb1", mod.emb1.weight, self.feature_index[a][0]))
            fields.append((a + "+" + b + ".emb2", mod.emb2.weight, self.feature_index[b][0]))
        plan = EmbeddingPlan(self.feature_index, deep_columns=self.dnn_feature_columns, deep_fields=fields,
                             wide_columns=self._linear_feature_columns, wide_tables=lm.embedding_dict,
                             wide_dense_weight=getattr(lm, "weight", None), pair=True)
        return plan, (lm.embedding_dict,)

    def logit_parts(self, X):
        plan = self.model_plan()
        use_dnn = len(self.dnn_feature_columns) > 0
        if not plan.has_lookup:
            if use_dnn:
                raise NotImplementedError      # (combined_dnn_input of nothing, inputs.py:126-138)
            return [self.linear_model(X)]
        dnn_input, wide = _ops.pair_embed(plan, X, full=True)
        return [wide.unsqueeze(1), self.tower_logit(dnn_input, plan.width)]
