"""CPU: DIN through the real Python stack over the stand-in for the library (tests/mock_lib.py + mock_ops.py, extended by
tests/mock_din.py with the attention kernel's entry points), against the reference's golden values (tests/golden/din,
tools/golden/make_din_golden.py): logits within 1e-5, every parameter gradient within 2e-5 x max|g_ref|, 3-step
trajectories.  Plus what needs no library at all: same-seed initial weights, state_dict keys, the constructors' errors, the
plan's row layout for named un-pooled columns, which route a call takes, the trainers' refusal.  The kernels themselves are
checked by tests/test_gpu_din_kernel.py, the model on the GPU by tests/test_gpu_din_models.py."""
import os

import numpy as np
import pytest
import torch

import din_helpers as H
import mock_din
from helpers import GOLDEN_DIR, feature_columns, golden_names, load_golden, max_abs

DEV = "cpu"


@pytest.fixture()
def din_mock(mock):
    return mock_din.extend(mock)


def _din_calls(mock):
    return [c for c in mock.calls if c.startswith("din_")]


def test_model_and_layers_are_exported():
    import deepctr_torch.layers as Ly
    import deepctr_torch.models as M
    from deepctr_torch.layers import AttentionSequencePoolingLayer, LocalActivationUnit
    from deepctr_torch.models import DIN
    assert M.DIN is DIN and "DIN" in M.__all__
    assert Ly.AttentionSequencePoolingLayer is AttentionSequencePoolingLayer and Ly.LocalActivationUnit is LocalActivationUnit


def test_fixture_set():
    assert golden_names("din/") == sorted(H.ALL + ["init"])
    for name in H.ALL + ["init"]:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, "din", name + ".npz")) < 1 << 20
    for name in H.ALL:
        g = load_golden("din/" + name)
        B, fi = g["X"].shape[0], None
        assert 16 <= B <= 40
        from deepctr_torch.inputs import build_input_features
        fi = build_input_features(feature_columns(g["spec"]["dnn_columns"]))
        T = [c["maxlen"] for c in g["spec"]["dnn_columns"] if c["name"].startswith("hist_")][0]
        lens = g["X"][:, fi["seq_length"][0]]
        assert set([0, 1, T - 1, T]) <= set(int(v) for v in lens), name


# ---- the stand-in itself against float64 autograd --------------------------------------------------------------------
@pytest.mark.parametrize("act", ["linear", "relu", "sigmoid", "prelu"])
@pytest.mark.parametrize("softmax", [False, True])
def test_stand_in_matches_float64_autograd(act, softmax):
    from deepctr_torch.layers import AttentionSequencePoolingLayer
    torch.manual_seed(3)
    B, T, E = 7, 5, 6
    layer = AttentionSequencePoolingLayer((8, 4), act, weight_normalization=softmax, embedding_dim=E).double()
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn_like(p) * 0.5)
    q = torch.randn(B, 1, E, dtype=torch.float64, requires_grad=True)
    k = torch.randn(B, T, E, dtype=torch.float64, requires_grad=True)
    lens = torch.tensor([[0], [1], [4], [5], [7], [-1], [3]])
    out = layer(q, k, lens)
    g = torch.randn_like(out)
    la = layer.local_att
    params = la.packed_params(act)
    order = []                                                     # the module's parameters in the packed order
    for fc, a in zip(la.dnn.linears, la.dnn.activation_layers):
        order += [fc.weight, fc.bias] + ([a.weight] if act == "prelu" else [])
    order += [la.dense.weight, la.dense.bias]
    gq, gk = torch.autograd.grad(out, [q, k], g, retain_graph=True)
    gp = torch.cat([t.reshape(-1) for t in torch.autograd.grad(out, order, g)])
    valid = (np.arange(T)[None, :] < lens.numpy())
    y, _, _ = mock_din.forward(q.detach().numpy()[:, 0], k.detach().numpy(), valid, params.detach().numpy(), [8, 4], act,
                               softmax)
    mq, mk, mp = mock_din.backward(q.detach().numpy()[:, 0], k.detach().numpy(), valid, params.detach().numpy(), [8, 4],
                                   act, softmax, g.numpy()[:, 0])
    assert max_abs(y, out.detach().numpy()) <= 1e-12
    assert max_abs(mq, gq.numpy()) <= 1e-12 and max_abs(mk, gk.numpy()) <= 1e-12 and max_abs(mp, gp.numpy()) <= 1e-12


# ---- the model over the stand-in -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.ALL)
def test_forward_matches_reference(din_mock, name):
    g, m = H.loaded(name, DEV)
    train = name != "din_dice_eval"
    H.check_forward(g, m, DEV, train)
    dice = g["spec"]["kwargs"].get("att_activation", "Dice") == "Dice"
    # (no gradient is needed here: no weights buffer.  Dice in train mode normalises with the batch: torch ops)
    assert _din_calls(din_mock) == ([] if dice and train else ["din_fwd:0"])


@pytest.mark.parametrize("name", H.ALL)
def test_gradients_match_reference(din_mock, name):
    g, m = H.loaded(name, DEV)
    H.check_gradients(g, m, DEV, name != "din_dice_eval")
    # Dice: torch ops whenever a gradient is needed, in eval mode too
    assert _din_calls(din_mock) == (["din_fwd:1", "din_bwd"] if name in H.KERNEL_TRAIN else [])


@pytest.mark.parametrize("name", H.STEPS)
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adagradp"])
def test_optimizer_trajectory(din_mock, name, opt):
    g, m = H.loaded(name, DEV)
    H.check_trajectory(g, m, DEV, opt)
    plan = m.model_plan()
    att = set(id(p) for p in m.attention.parameters())
    assert att and not att & set(id(p) for p in plan.table_params)        # the attention unit: the dense optimizer's
    assert not getattr(m, "_fused_step_ok", False)
    assert _din_calls(din_mock).count("din_bwd") == 3


def test_default_kwargs_adam_trajectory(din_mock):
    g = load_golden("din/din_default_adam")
    m = H.build_din(g["spec"], DEV, l2=1e-6)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    H.check_trajectory(g, m, DEV, "adam")
    assert _din_calls(din_mock) == []                # default Dice in train mode


@pytest.mark.parametrize("name", H.ALL)
def test_state_dict_keys_are_the_references(name):
    g = load_golden("din/" + name)
    assert list(H.build_din(g["spec"], DEV).state_dict()) == list(g["params"])


def test_init_fixture_exists():
    assert len(H.init_configs()) == 2


@pytest.mark.parametrize("c", H.init_configs(), ids=lambda c: "dropout" if c[0]["kwargs"] else "default")
def test_same_seed_initial_weights_are_the_references(c):
    spec, params = c
    sd = H.build_din(spec, DEV, l2=1e-6).state_dict()
    assert list(sd) == list(params)
    for k, v in params.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert np.array_equal(sd[k].numpy(), v), k


def test_model_takes_the_autograd_step_and_adds_no_dnn_regularisation():
    g = load_golden("din/din_sigmoid")
    m = H.build_din(dict(g["spec"], kwargs=dict(g["spec"]["kwargs"], l2_reg_dnn=0.5)), DEV, l2=1e-6)
    assert len(m.regularization_weight) == 2 and not getattr(m, "_fused_step_ok", False)
    assert m.model_plan().unpooled_columns == ("hist_item_id", "hist_cate_id") and not m.model_plan().simple_units
    assert m.model_plan().unit_path


# ---- constructors and errors -----------------------------------------------------------------------------------------
def test_layer_constructors_and_keys():
    from deepctr_torch.layers import AttentionSequencePoolingLayer, LocalActivationUnit
    la = LocalActivationUnit()
    assert [tuple(fc.weight.shape) for fc in la.dnn.linears] == [(64, 16), (32, 64)] and tuple(la.dense.weight.shape) == (1, 32)
    assert list(la.state_dict()) == ["dnn.linears.0.weight", "dnn.linears.0.bias", "dnn.linears.1.weight",
                                     "dnn.linears.1.bias", "dense.weight", "dense.bias"]
    at = AttentionSequencePoolingLayer()
    assert [fc.out_features for fc in at.local_att.dnn.linears] == [80, 40] and at.local_att.dnn.linears[0].in_features == 16
    assert not at.weight_normalization and not at.return_score and not at.supports_masking
    init = dict(H.init_configs()[1][1])
    dice = AttentionSequencePoolingLayer((64, 16), "Dice", embedding_dim=12)
    assert ["attention." + k for k in dice.state_dict()] == [k for k in init if k.startswith("attention.")]
    with pytest.raises(ValueError, match="hidden_units is empty"):
        LocalActivationUnit(hidden_units=())
    with pytest.raises(NotImplementedError):
        LocalActivationUnit(activation="tanh")


def test_masking_error_and_mask_route(din_mock):
    from deepctr_torch.layers import AttentionSequencePoolingLayer
    torch.manual_seed(0)
    at = AttentionSequencePoolingLayer((8, 4), "sigmoid", supports_masking=True, embedding_dim=4)
    q, k = torch.randn(3, 1, 4), torch.randn(3, 5, 4)
    with pytest.raises(ValueError, match="When supports_masking=True,input must support masking"):
        at(q, k, None)
    mask = torch.tensor([[1, 0, 1, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]], dtype=torch.bool)
    with torch.no_grad():
        y = at(q, k, None, mask=mask)
        ref = at._forward_torch(q, k, mask)
    assert _din_calls(din_mock) == ["din_fwd:0"] and tuple(y.shape) == (3, 1, 4)
    assert max_abs(y.numpy(), ref.numpy()) <= 1e-6


def test_model_errors(din_mock):
    from deepctr_torch.inputs import SparseFeat, VarLenSparseFeat
    from deepctr_torch.models import DIN
    cols = [SparseFeat("item", 5, 4), VarLenSparseFeat(SparseFeat("hist_item", 5, 4, embedding_name="item"), 3)]
    m = DIN(cols, ["item"], dnn_hidden_units=(4,), att_activation="sigmoid")
    with pytest.raises(ValueError, match="please add max length column"):
        m(torch.zeros(2, 4))


# ---- the plan --------------------------------------------------------------------------------------------------------
def _plan(unpooled):
    from deepctr_torch._hip.plan import EmbeddingPlan
    from deepctr_torch.inputs import DenseFeat, SparseFeat, VarLenSparseFeat, build_input_features, create_embedding_matrix
    cols = [VarLenSparseFeat(SparseFeat("tags", 8, 4), 3, "mean", "tags_length"), SparseFeat("user", 7, 4),
            SparseFeat("item", 9, 8), DenseFeat("price", 2),
            VarLenSparseFeat(SparseFeat("hist_item", 9, 8, embedding_name="item"), 4, "mean", "seq_length"),
            VarLenSparseFeat(SparseFeat("kw", 6, 2), 2, "sum")]
    fi = build_input_features(cols)
    return EmbeddingPlan(fi, deep_columns=cols, deep_tables=create_embedding_matrix(cols), unpooled=unpooled), fi


def _rows(plan):
    return [(f.name, f.col, f.len, f.pool, f.out_off) for f in plan.deep]


def test_plan_row_layout_for_named_unpooled_columns():
    p, fi = _plan(("hist_item",))
    h0 = fi["hist_item"][0]
    assert _rows(p) == [("user", fi["user"][0], 1, 0, 0), ("item", fi["item"][0], 1, 0, 4)] + \
        [("hist_item[%d]" % t, h0 + t, 1, 0, 12 + 8 * t) for t in range(4)] + \
        [("tags", fi["tags"][0], 3, 2, 44), ("kw", fi["kw"][0], 2, 1, 48)]
    assert p.n_deep_fixed == 6 and p.emb_width == 50 and p.dense_off == 50 and p.width == 52
    assert p.unpooled_columns == ("hist_item",) and not p.simple_units
    assert p.deep[4].param is p.deep[1].param                    # the history positions read the candidate's table


def test_plan_unpooled_true_and_false_are_unchanged():
    p, fi = _plan(False)
    assert [(n, ln, pool, off) for n, _, ln, pool, off in _rows(p)] == \
        [("user", 1, 0, 0), ("item", 1, 0, 4), ("tags", 3, 2, 12), ("hist_item", 4, 2, 16), ("kw", 2, 1, 24)]
    assert p.unpooled_columns == () and p.n_deep_fixed == 2 and p.emb_width == 26
    q, _ = _plan(True)
    names = ["user", "item"] + ["tags[%d]" % t for t in range(3)] + ["hist_item[%d]" % t for t in range(4)] + \
        ["kw[%d]" % t for t in range(2)]
    assert [f.name for f in q.deep] == names and q.n_deep_fixed == len(names)
    offs, o = [], 0
    for f in q.deep:
        offs.append(o)
        o += f.dim
    assert [f.out_off for f in q.deep] == offs and q.emb_width == o == 4 + 8 + 12 + 32 + 4
    assert q.unpooled_columns == ("tags", "hist_item", "kw")
    assert _plan(())[0].unpooled_columns == () and _rows(_plan(())[0]) == _rows(p)


def test_existing_models_get_the_plan_they_had():
    from deepctr_torch.models import BaseModel, DeepFM
    assert BaseModel._unpooled_columns == ()
    g = load_golden("deepfm_mixed")
    cols = feature_columns(g["spec"]["dnn_columns"])
    p = DeepFM(cols, cols, dnn_hidden_units=(4,)).model_plan()
    assert p.unpooled_columns == () and p.n_deep_fixed == 3 and len(p.deep) == 7


# ---- which route a call takes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,train,grad,fused", [
    ("sigmoid", True, True, True), ("relu", True, True, True), ("prelu", True, True, True), ("linear", True, True, True),
    ("sigmoid", False, False, True), ("Dice", True, True, False), ("Dice", True, False, False),
    ("Dice", False, True, False), ("Dice", False, False, True)])
def test_route_by_activation_and_mode(din_mock, act, train, grad, fused):
    from deepctr_torch.layers import AttentionSequencePoolingLayer
    torch.manual_seed(1)
    at = AttentionSequencePoolingLayer((8, 4), act, embedding_dim=4).train(train)
    q, k, n = torch.randn(5, 1, 4), torch.randn(5, 3, 4), torch.tensor([[0], [1], [2], [3], [3]])
    with torch.set_grad_enabled(grad):
        y = at(q, k, n)
    assert tuple(y.shape) == (5, 1, 4)
    assert _din_calls(din_mock) == ((["din_fwd:1"] if grad else ["din_fwd:0"]) if fused else [])
    if fused:
        with torch.no_grad():
            ref = at._forward_torch(q, k, at._valid(k, n, None))
        assert max_abs(y.detach().numpy(), ref.numpy()) <= 1e-6


def test_route_by_shape_dtype_and_options(din_mock):
    from deepctr_torch.layers import AttentionSequencePoolingLayer
    torch.manual_seed(1)
    n = torch.tensor([[1], [2]])

    def calls(layer, T=3, E=4, dtype=torch.float32):
        del din_mock.calls[:]
        with torch.no_grad():
            layer(torch.randn(2, 1, E, dtype=dtype), torch.randn(2, T, E, dtype=dtype), n)
        return _din_calls(din_mock)
    assert calls(AttentionSequencePoolingLayer((8, 4), "sigmoid", embedding_dim=4)) == ["din_fwd:0"]
    assert calls(AttentionSequencePoolingLayer((8, 4), "sigmoid", embedding_dim=4), T=128) == ["din_fwd:0"]
    assert calls(AttentionSequencePoolingLayer((8, 4), "sigmoid", embedding_dim=4), T=129) == []
    assert calls(AttentionSequencePoolingLayer((8, 4), "sigmoid", embedding_dim=65), E=65) == []
    assert calls(AttentionSequencePoolingLayer((8, 4), "sigmoid", embedding_dim=64), E=64) == ["din_fwd:0"]
    assert calls(AttentionSequencePoolingLayer((8, 4, 4, 4), "sigmoid", embedding_dim=4)) == []
    assert calls(AttentionSequencePoolingLayer((129,), "sigmoid", embedding_dim=4)) == []
    assert calls(AttentionSequencePoolingLayer((128, 128, 128), "sigmoid", embedding_dim=4)) == ["din_fwd:0"]
    assert calls(AttentionSequencePoolingLayer((8, 4), "sigmoid", return_score=True, embedding_dim=4)) == []
    assert calls(AttentionSequencePoolingLayer((8, 4), "sigmoid", embedding_dim=4).double(), dtype=torch.float64) == []
    bn = AttentionSequencePoolingLayer((8, 4), "sigmoid", embedding_dim=4)
    bn.local_att.dnn.use_bn = True
    bn.local_att.dnn.bn = torch.nn.ModuleList(torch.nn.BatchNorm1d(3) for _ in range(2))   # (BatchNorm1d over [B, T, H])
    assert calls(bn) == []
    drop = AttentionSequencePoolingLayer((8, 4), "sigmoid", embedding_dim=4)
    drop.local_att.dnn.dropout_rate, drop.local_att.dnn.dropout = 0.5, torch.nn.Dropout(0.5)
    assert calls(drop.train()) == [] and calls(drop.eval()) == ["din_fwd:0"]
    with torch.no_grad():
        s = AttentionSequencePoolingLayer((8, 4), "sigmoid", return_score=True, embedding_dim=4)(
            torch.randn(2, 1, 4), torch.randn(2, 3, 4), n)
    assert tuple(s.shape) == (2, 1, 3)


def test_layer_gradients_through_the_stand_in(din_mock):
    from deepctr_torch.layers import AttentionSequencePoolingLayer
    torch.manual_seed(5)
    for act, sm in (("prelu", False), ("sigmoid", True)):
        at = AttentionSequencePoolingLayer((8, 4), act, weight_normalization=sm, embedding_dim=6)
        with torch.no_grad():
            for p in at.parameters():
                p.copy_(torch.randn_like(p) * 0.5)
        q, k = torch.randn(6, 1, 6, requires_grad=True), torch.randn(6, 4, 6, requires_grad=True)
        n = torch.tensor([[0], [1], [3], [4], [9], [2]])
        y = at(q, k, n)
        g = torch.randn_like(y)
        got = torch.autograd.grad(y, [q, k] + list(at.parameters()), g)
        ref = torch.autograd.grad(at._forward_torch(q, k, at._valid(k, n, None)), [q, k] + list(at.parameters()), g,
                                  allow_unused=True)
        names = ["q", "k"] + [n_ for n_, _ in at.named_parameters()]
        scale = dict((n_, float(b.abs().max())) for n_, b in zip(names, ref))
        if sm:      # a softmax ignores a shift of every score: the exact gradient is 0 (din_helpers.grad_scale)
            scale["local_att.dense.bias"] = scale["local_att.dense.weight"]
        for n_, a, b in zip(names, got, ref):
            assert a.shape == b.shape and max_abs(a.numpy(), b.numpy()) <= 2e-5 * scale[n_], n_


# ---- multi-GPU trainers ----------------------------------------------------------------------------------------------
def test_multi_gpu_trainers_refuse_unpooled_plans(monkeypatch):
    import torch.distributed as dist
    from deepctr_torch import distributed_fit, parallel
    g = load_golden("din/din_sigmoid")
    m = H.build_din(g["spec"], DEV)
    m.compile("adagrad", "binary_crossentropy")
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    for cls in (parallel.DataParallelTrainer, parallel.ShardedTrainer):
        with pytest.raises(NotImplementedError, match="un-pooled behaviour sequences"):
            cls(m)
    with pytest.raises(NotImplementedError, match="un-pooled behaviour sequences"):
        distributed_fit.fit(m, torch.zeros(4, 6), torch.zeros(4), 2, 1, 0, 0, False, None, None, False, None)
