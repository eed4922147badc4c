# -*- coding: utf-8 -*-
"""MLR -- Mixed Logistic Regression / LS-PLM (reference models/mlr.py:17-100): ``region_num`` ``Linear`` modules form a
softmax gate and, read a second time, are the learners; an optional bias ``Linear`` scales the mixture.

The reference runs 2 R + 1 ``Linear`` calls and a dozen glue operators forward, R + 1 dense table gradients backward.  Here
the model plan is wide-only and per-field over the R region sides plus the bias side (``EmbeddingPlan(wide_sides=...)``), and
ONE launch per direction (csrc/mlr.hip) reads a sample's ids once, fetches every head's first-order weights, and computes
gate, learners and bias factor; the backward hands per-field gradients to the sorted / lazy table updates every other
model's lookup uses.  ``DCTR_MLR=0`` (and a plan outside the kernel's envelope) composes the same value from one per-field
gather and torch ops.

Reproduced as the reference runs: the learners read ``region_linear_model`` (``base_linear_model`` exists, is in
``state_dict`` and never moves); ``BaseModel``'s ``embedding_dict`` / ``linear_model`` over the region columns are never
looked up but stay L2-regularised (1e-5) dense parameters; ``l2_reg_linear`` and ``seed`` are stored and never applied
(``BaseModel`` seeds with its default); ``forward`` returns the mixture directly -- ``self.out`` is never called."""
import torch.nn as nn

from .basemodel import BaseModel, Linear
from .._hip import ops as _ops
from .._hip.plan import EmbeddingPlan
from .._hip.update_paths import regularizers
from ..inputs import build_input_features
from ..layers import PredictionLayer


class MLR(BaseModel):
    """Same arguments as the reference (models/mlr.py:34-36)."""

    def __init__(self, region_feature_columns, base_feature_columns=None, bias_feature_columns=None, region_num=4,
                 l2_reg_linear=1e-5, init_std=0.0001, seed=1024, task='binary', device='cpu', gpus=None):
        super(MLR, self).__init__(region_feature_columns, region_feature_columns, task=task, device=device, gpus=gpus)
        if region_num <= 1:
            raise ValueError("region_num must > 1")
        self.l2_reg_linear = l2_reg_linear
        self.init_std = init_std
        self.seed = seed
        self.device = device
        self.region_num = region_num
        self.region_feature_columns = region_feature_columns
        self.base_feature_columns = base_feature_columns
        self.bias_feature_columns = bias_feature_columns
        if base_feature_columns is None or len(base_feature_columns) == 0:
            self.base_feature_columns = region_feature_columns
        if bias_feature_columns is None:
            self.bias_feature_columns = []
        self.feature_index = build_input_features(
            self.region_feature_columns + self.base_feature_columns + self.bias_feature_columns)
        self.region_linear_model = nn.ModuleList([Linear(
            self.region_feature_columns, self.feature_index, self.init_std, self.device) for _ in range(self.region_num)])
        self.base_linear_model = nn.ModuleList([Linear(
            self.base_feature_columns, self.feature_index, self.init_std, self.device) for _ in range(self.region_num)])
        if self.bias_feature_columns is not None and len(self.bias_feature_columns) > 0:
            self.bias_model = nn.Sequential(
                Linear(self.bias_feature_columns, self.feature_index, self.init_std, self.device),
                PredictionLayer(task='binary', use_bias=False))
        self.prediction_layer = PredictionLayer(task=task, use_bias=False)
        self._mlr_task = task
        self._heads = None
        self.to(self.device)

    def _has_bias(self):
        return self.bias_feature_columns is not None and len(self.bias_feature_columns) > 0

    def _head_modules(self):
        """the Linear modules the output depends on, in head order: the R regions, then the bias"""
        return list(self.region_linear_model) + ([self.bias_model[0]] if self._has_bias() else [])

    def _build_plan(self):
        """Wide-only, per-field, over the R region sides plus the bias side; every table a parameter of its own.  The dense
        halves (``Linear.weight`` of every head) belong to the mixture kernel, not to the plan.  ``base_linear_model``,
        ``embedding_dict`` and ``linear_model`` are in no plan: nothing looks them up."""
        columns = [self.region_feature_columns] * self.region_num + ([self.bias_feature_columns] if self._has_bias() else [])
        mods = self._head_modules()
        plan = EmbeddingPlan(self.feature_index, wide_sides=[(c, m.embedding_dict) for c, m in zip(columns, mods)],
                             wide_per_field=True)
        return plan, tuple(m.embedding_dict for m in mods)

    def mlr_heads(self):
        plan = self.model_plan()
        if self._heads is None or self._heads.plan is not plan:
            self._heads = _ops.MLRHeads(plan, [getattr(m, "weight", None) for m in self._head_modules()],
                                        self.region_num, self._has_bias(), self._mlr_task)
        return self._heads

    def _embedding_reg_active(self):
        # BaseModel's first two groups are the dead embedding_dict / linear_model (L2 1e-5, never looked up): what decides
        # between the in-kernel and the lazy table update is a regulariser on the PLAN's tables, and MLR puts none there
        tables = set(id(p) for p in self._plan.table_params)
        return any((l1 > 0 or l2 > 0) and id(p) in tables for p, l1, l2 in regularizers(self))

    def forward(self, X):
        return _ops.mlr(self.model_plan(), self.mlr_heads(), X).unsqueeze(1)

    def fit(self, *args, **kwargs):
        from .. import distributed_fit as _dfit
        if _dfit.context() is not None:      # (looks at WORLD_SIZE / an existing group only: creates nothing)
            raise NotImplementedError(
                "MLR.fit() under several ranks (WORLD_SIZE > 1) is not implemented: the table-sharded and the replicated "
                "trainers exchange one model-wide lookup, not the mixture's per-head rows; train MLR in one process")
        return super(MLR, self).fit(*args, **kwargs)
