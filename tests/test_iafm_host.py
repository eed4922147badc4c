"""CPU, no library needed: IFM / DIFM exist with the reference's constructor behaviour and same-seed initial weights
(tests/golden/iafm/init.npz: the six configurations of the reference's own IFM / DIFM tests), the per-field-wide plan mode
carries its bit and leading dimension, and what cannot honour it refuses it."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, feature_columns


def _init_configs():
    z = np.load(os.path.join(GOLDEN_DIR, "iafm", "init.npz"), allow_pickle=False)
    out = []
    for i, spec in enumerate(json.loads(str(z["configs"]))):
        pre = "%d/param/" % i
        out.append((spec, {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}))
    return out


def _id(c):
    spec = c[0]
    return "%s-%ds-%s" % (spec["model"], len([x for x in spec["dnn_columns"] if x["kind"] == "sparse"]),
                          ",".join("%s=%s" % kv for kv in sorted(spec["kwargs"].items())).replace(" ", ""))


def test_models_are_exported():
    import deepctr_torch.models as M
    from deepctr_torch.models import DIFM, IFM
    assert M.IFM is IFM and M.DIFM is DIFM and "IFM" in M.__all__ and "DIFM" in M.__all__


@pytest.mark.parametrize("c", _init_configs(), ids=_id)
def test_same_seed_initial_weights_are_the_references(c):
    import deepctr_torch.models as M
    spec, params = c
    cols = feature_columns(spec["dnn_columns"])
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in spec["kwargs"].items()}
    m = getattr(M, spec["model"])(cols, cols, device="cpu", **kw)
    sd = m.state_dict()
    assert list(sd) == list(params)
    for k, v in params.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert np.array_equal(sd[k].numpy(), v), k


@pytest.mark.parametrize("model", ["IFM", "DIFM"])
def test_constructor_errors(model):
    import deepctr_torch.models as M
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    cls = getattr(M, model)
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4), DenseFeat("x", 1)]
    with pytest.raises(ValueError, match="dnn_hidden_units is null!"):
        cls(cols, cols, dnn_hidden_units=(), device="cpu")
    with pytest.raises(ValueError):
        cls(cols[:1] + cols[2:], cols, dnn_hidden_units=(4,), device="cpu")       # 1 linear sparse column against 2
    cls(cols[2:], cols, dnn_hidden_units=(4,), device="cpu")                        # dense columns only: fine
    cls([], cols, dnn_hidden_units=(4,), device="cpu")                              # no linear side: fine


@pytest.mark.parametrize("model", ["IFM", "DIFM"])
def test_no_sparse_features_raises_at_forward(mock, model):
    import deepctr_torch.models as M
    from deepctr_torch.inputs import DenseFeat
    cols = [DenseFeat("x", 1), DenseFeat("y", 2)]
    kw = {"att_head_num": 1} if model == "DIFM" else {}
    try:
        m = getattr(M, model)(cols, cols, dnn_hidden_units=(4,), device="cpu", **kw)
    except Exception as e:          # (the reference's DIFM dies in its constructor on such columns; IFM builds)
        assert model == "DIFM", e
        return
    with pytest.raises(ValueError, match="there are no sparse features"):
        m(torch.rand(3, 3))


def _plan(per_field):
    from deepctr_torch._hip.plan import EmbeddingPlan
    from deepctr_torch.inputs import DenseFeat, SparseFeat, VarLenSparseFeat, build_input_features, \
        create_embedding_matrix
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4), DenseFeat("x", 2),
            VarLenSparseFeat(SparseFeat("h", 6, 4, embedding_name="b"), 3, "mean")]
    fi = build_input_features(cols)
    deep = create_embedding_matrix(cols, 0.1, sparse=False, device="cpu")
    wide = create_embedding_matrix(cols, 0.1, linear=True, sparse=False, device="cpu")
    w = torch.nn.Parameter(torch.zeros(2, 1))
    return EmbeddingPlan(fi, deep_columns=cols, deep_tables=deep, wide_columns=cols, wide_tables=wide,
                         wide_dense_weight=w, wide_per_field=per_field)


def test_plan_mode_carries_the_bit(mock):
    from deepctr_torch._hip import lib as L
    assert L.PLAN_WIDE_PER_FIELD == 8
    p = _plan(True)
    p.bind("cpu")
    assert p.wide_per_field and p.cplan.flags & L.PLAN_WIDE_PER_FIELD
    assert p.ld_wide == len(p.wide) + 1 == 4 and p.ld_wide >= p.cplan.n_wide + 1
    # general units name each slot's wide field: its column of a per-field gradient row
    assert p.gen is not None and sorted(set(s["wfield"] for s in p.gen["slots"])) == [0, 1, 2]
    q = _plan(False)
    q.bind("cpu")
    assert not q.wide_per_field and not (q.cplan.flags & L.PLAN_WIDE_PER_FIELD) and q.ld_wide == 1
    import pickle
    r = pickle.loads(pickle.dumps(p))
    assert r.wide_per_field and r.ld_wide == 4


def test_model_plan_is_per_field_only_for_these_models():
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    from deepctr_torch.models import DIFM, IFM, DeepFM
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4), DenseFeat("x", 1)]
    assert IFM(cols, cols, dnn_hidden_units=(4,)).model_plan().wide_per_field
    assert DIFM(cols, cols, dnn_hidden_units=(4,)).model_plan().wide_per_field
    assert not DeepFM(cols, cols, dnn_hidden_units=(4,)).model_plan().wide_per_field


def test_multi_gpu_trainers_refuse_the_mode(monkeypatch):
    import torch.distributed as dist
    from deepctr_torch import distributed_fit, parallel
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    from deepctr_torch.models import IFM
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4), DenseFeat("x", 1)]
    m = IFM(cols, cols, dnn_hidden_units=(4,), l2_reg_linear=0, l2_reg_embedding=0)
    m.compile("adagrad", "binary_crossentropy")
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    for cls in (parallel.DataParallelTrainer, parallel.ShardedTrainer):
        with pytest.raises(NotImplementedError, match="per-field first-order weights"):
            cls(m)
    with pytest.raises(NotImplementedError, match="per-field first-order weights"):
        distributed_fit.fit(m, torch.zeros(4, 3), torch.zeros(4), 2, 1, 0, 0, False, None, None, False, None)
