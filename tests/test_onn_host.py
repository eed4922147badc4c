"""CPU: ONN through the real Python stack over the stand-in for the library (tests/mock_lib.py + mock_ops.py, extended by
tests/mock_onn.py with the pair lookup's two entry points), against the reference's golden values (tests/golden/onn,
tools/golden/make_onn_golden.py): logits within 1e-5, every parameter gradient within 2e-5 x max|g_ref| (no floor of 1 for
the pair tables), 3-step SGD / Adagrad trajectories, the 8-step regularised Adam run on the lazy update.  Plus what needs no
library at all: the plan's pair mode, same-seed initial weights, the constructor's ValueErrors, the trainers' refusals.  The
kernels themselves are checked by tests/test_gpu_onn_kernel.py, the model on the GPU by tests/test_gpu_onn_models.py."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import mock_onn
from helpers import GOLDEN_DIR, build_model, feature_columns, load_golden, max_abs

DEV = "cpu"
LOGIT_TOL, GRAD_TOL, TRAJ_TOL = 1e-5, 2e-5, 2e-5
FORWARD = ["onn_two", "onn_d6", "onn_criteo", "onn_mixed", "onn_one_sparse", "onn_nolinear", "onn_bn"]
STEPS = ["onn_two", "onn_criteo"]


@pytest.fixture()
def onn_mock(mock):
    return mock_onn.extend(mock)


def _loaded(name, l2=0.0):
    g = load_golden("onn/" + name)
    m = build_model(g["spec"], DEV, l2=l2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    return g, m


def grad_scale(key, ref):
    """The gradient bound's scale: max|g_ref| of the parameter; the floor of 1 the other model suites use is NOT applied to
    the pair tables (their gradients are 5e-3 .. 0.2 in these fixtures: a floor would hide them)."""
    top = float(np.max(np.abs(ref))) if ref.size else 0.0
    return top if "second_order_embedding_dict" in key else max(1.0, top)


def test_model_is_exported():
    import deepctr_torch.models as M
    from deepctr_torch.models import ONN
    assert M.ONN is ONN and "ONN" in M.__all__


# ---- the model over the stand-in -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORWARD)
def test_forward_matches_reference(onn_mock, name):
    g, m = _loaded(name)
    # (the fixtures hold the reference's train-mode forward: BatchNorm then normalises with the batch's statistics)
    m.train(bool(g["spec"]["kwargs"].get("dnn_use_bn")))
    cap = {}
    h = m.out.register_forward_pre_hook(lambda mod, inp: cap.__setitem__("logit", inp[0].detach()))
    with torch.no_grad():
        y = m(torch.from_numpy(g["X"]))
    h.remove()
    m.model_plan().check_ids()
    assert max_abs(cap["logit"].numpy(), g["logit"]) <= LOGIT_TOL
    assert max_abs(y.numpy(), g["y_pred"]) <= LOGIT_TOL
    assert onn_mock.calls.count("pair_embed_fwd") == 1 and "embed_fwd" not in onn_mock.calls


@pytest.mark.parametrize("name", FORWARD)
def test_gradients_match_reference(onn_mock, name):
    g, m = _loaded(name)
    m.train()
    loss = torch.nn.functional.binary_cross_entropy(m(torch.from_numpy(g["X"])).squeeze(1), torch.from_numpy(g["y"]),
                                                    reduction="sum")
    m.zero_grad()
    loss.backward()
    assert abs(loss.item() - g["loss"]) <= 1e-4 * max(1.0, abs(g["loss"]))
    assert set(g["grads"]) == set(k for k, _ in m.named_parameters())
    for k, p in m.named_parameters():
        ref = g["grads"][k]
        got = p.grad.numpy() if p.grad is not None else np.zeros_like(ref)
        err = max_abs(got, ref)
        assert err <= GRAD_TOL * grad_scale(k, ref), "%s: max|d|=%.3e max|g_ref|=%.3g" % (k, err, np.max(np.abs(ref)))
        if k.startswith("embedding_dict."):
            assert p.grad is None, "%s: the output never depends on embedding_dict" % k
    assert onn_mock.calls.count("pair_embed_bwd") == (1 if m.model_plan().deep else 0)


def test_unused_tables_get_the_l2_gradient_only(onn_mock):
    """``embedding_dict`` is L2-regularised like in the reference although nothing looks it up: its gradient is 2 lambda w."""
    g, m = _loaded("onn_two", l2=1e-3)
    m.train()
    y = m(torch.from_numpy(g["X"])).squeeze(1)
    loss = torch.nn.functional.binary_cross_entropy(y, torch.from_numpy(g["y"]), reduction="sum")
    m.zero_grad()
    (loss + m.get_regularization_loss()).backward()
    for k, p in m.embedding_dict.named_parameters():
        assert max_abs(p.grad.numpy(), 2e-3 * p.detach().numpy()) <= 1e-9, k


@pytest.mark.parametrize("name", STEPS)
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adagradp"])
def test_in_kernel_optimizer_trajectory(onn_mock, name, opt):
    g, m = _loaded(name)
    m.compile("adagrad" if opt == "adagradp" else opt, "binary_crossentropy", metrics=[])
    if opt == "adagradp":
        for grp in m.optim.param_groups:
            for p in grp["params"]:
                m.optim.state[p]["sum"].fill_(0.05)
    m.train()
    losses = [float(m._train_step(torch.from_numpy(Xb), torch.from_numpy(yb))[0])
              for Xb, yb in zip(g["extra"]["X_steps"], g["extra"]["y_steps"])]
    plan = m.model_plan()
    kind = "sgd" if opt == "sgd" else "adagrad"
    assert plan.pair and plan.update[0] == kind and plan.unit_path
    assert "embed_update:%d" % (0 if opt == "sgd" else 1) in onn_mock.calls
    assert not any(c.startswith("embed_bwd") or c == "embed_fwd" for c in onn_mock.calls)
    np.testing.assert_allclose(losses, g["extra"][opt + "3_loss"], rtol=2e-5)
    sd = m.state_dict()
    n = 0
    for k, v in g["extra"].items():
        if k.startswith(opt + "3/"):
            assert max_abs(sd[k[len(opt) + 2:]].numpy(), v) <= TRAJ_TOL, k
            n += 1
    assert n == len(sd)


def test_lazy_adam_replays_reference_trajectory(onn_mock):
    """The reference's default kind of training (L2 on every table, Adam): ids -> catch-up -> pair forward -> pair backward ->
    update(ACCUM) on the row gradients -> apply (the stand-in's dctr_embed_update_lazy answers DCTR_ENOSUP: two passes)."""
    g, m = _loaded("lazy_onn", l2=1e-3)
    ex = g["extra"]
    m.compile("adam", "binary_crossentropy", metrics=[])
    m.train()
    assert m.model_plan().update == ("lazy", "adam")
    bce, tot = [], []
    for Xb, yb in zip(ex["lazy_X"], ex["lazy_y"]):
        loss, total, _ = m._train_step(torch.from_numpy(Xb), torch.from_numpy(yb))
        bce.append(float(loss))
        tot.append(float(total))
    assert "embed_update:2" in onn_mock.calls and "lazy_apply" in onn_mock.calls
    np.testing.assert_allclose(bce, ex["lazy_adam_bce"], rtol=2e-5)
    np.testing.assert_allclose(tot, ex["lazy_adam_total"], rtol=2e-5)
    sd = m.state_dict()
    for k, v in ex.items():
        if k.startswith("lazy_adam/"):
            ref = np.asarray(v, np.float64)
            err = max_abs(sd[k[len("lazy_adam/"):]].numpy(), ref)
            assert err <= 2e-5 * max(1.0, float(np.max(np.abs(ref)))), k


def test_default_kwargs_take_the_lazy_update(onn_mock):
    from deepctr_torch.models import ONN
    cols = feature_columns(load_golden("onn/onn_two")["spec"]["dnn_columns"])
    m = ONN(cols, cols, dnn_hidden_units=(8,))
    m.compile("adam", "binary_crossentropy")
    plan = m.model_plan()
    assert plan.update == ("lazy", "adam")
    tables = set(id(p) for p in plan.table_params)
    assert tables == set(id(p) for p in m.second_order_embedding_dict.parameters()) | \
        set(id(p) for p in m.linear_model.embedding_dict.parameters())
    assert m.linear_model.plan().update == plan.update


# ---- same-seed initial weights -------------------------------------------------------------------------------------
def _init_configs():
    path = os.path.join(GOLDEN_DIR, "onn", "init.npz")
    if not os.path.exists(path):
        return []
    z = np.load(path, allow_pickle=False)
    out = []
    for i, spec in enumerate(json.loads(str(z["configs"]))):
        pre = "%d/param/" % i
        out.append((spec, {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}))
    return out


def test_init_fixture_exists():
    assert len(_init_configs()) == 2


@pytest.mark.parametrize("c", _init_configs(), ids=lambda c: "%ds" % len([x for x in c[0]["dnn_columns"]
                                                                             if x["kind"] == "sparse"]))
def test_same_seed_initial_weights_are_the_references(c):
    from deepctr_torch.models import ONN
    spec, params = c
    cols = feature_columns(spec["dnn_columns"])
    kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in spec["kwargs"].items()}
    sd = ONN(cols, cols, device="cpu", **kw).state_dict()
    assert list(sd) == list(params)
    for k, v in params.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert np.array_equal(sd[k].numpy(), v), k


# ---- constructor ---------------------------------------------------------------------------------------------------
def test_constructor_errors():
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    from deepctr_torch.models import ONN
    with pytest.raises(ValueError, match="embedding_name"):      # (the reference: KeyError at the first forward)
        ONN([], [SparseFeat("a", 5, 4, embedding_name="t"), SparseFeat("b", 6, 4), DenseFeat("x", 1)])
    with pytest.raises(ValueError, match="embedding_name"):      # (the reference: two columns silently share pair tables)
        ONN([], [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4, embedding_name="a"), DenseFeat("x", 1)])
    with pytest.raises(ValueError, match="must be same"):
        ONN([], [SparseFeat("a", 5, 4), SparseFeat("b", 6, 8)])


def test_state_dict_keys_and_dnn_width():
    from deepctr_torch.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_torch.models import ONN
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4), SparseFeat("c", 7, 4), DenseFeat("x", 2),
            VarLenSparseFeat(SparseFeat("h", 6, 4), 3, "mean")]
    m = ONN(cols, cols, dnn_hidden_units=(8,))
    keys = [k for k in m.state_dict() if k.startswith("second_order_embedding_dict.")]
    assert keys == ["second_order_embedding_dict.%s.emb%d.weight" % (p, e) for p in ("a+b", "a+c", "b+c") for e in (1, 2)]
    assert m.dnn.linears[0].weight.shape[1] == 3 * 4 + 2         # the VarLen column takes no part in the second order
    assert m.dnn_linear.bias is None
    assert [len(w) for w, _, _ in m.regularization_weight][2] == 6


# ---- the plan's pair mode ------------------------------------------------------------------------------------------
def _pair_model():
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    from deepctr_torch.models import ONN
    cols = [SparseFeat("a", 5, 6), SparseFeat("b", 6, 6), SparseFeat("c", 7, 6), DenseFeat("x", 2), DenseFeat("y", 1)]
    return ONN(cols[1:], cols, dnn_hidden_units=(8,), l2_reg_embedding=0, l2_reg_linear=0)


def test_pair_plan_layout():
    m = _pair_model()
    p = m.model_plan()
    so = m.second_order_embedding_dict
    assert p.pair and not p.wide_per_field
    assert [f.name for f in p.deep] == ["a+b.emb1", "a+b.emb2", "a+c.emb1", "a+c.emb2", "b+c.emb1", "b+c.emb2"]
    assert [f.param for f in p.deep][2] is so["a+c"].emb1.weight and p.deep[5].param is so["b+c"].emb2.weight
    fi = m.feature_index
    assert [f.col for f in p.deep] == [fi[n][0] for n in ("a", "b", "a", "c", "b", "c")]
    assert [f.out_off for f in p.deep] == [0, 6, 12, 18, 24, 30]
    assert p.n_deep_fixed == 6 and p.emb_dim == 6 and p.vec == 2
    assert p.emb_width == 18 and p.dense_off == 18 and p.width == 21 and p.ld_out == 24 and p.ld_rows == 36
    assert p.simple_units and p.unit_path and p.gen is None
    # one unit per pair table; the first-order tables of b and c ride on a unit over the same X column
    assert len(p.units) == 6 and [u[0] for u in p.units] == list(range(6))
    assert sorted(u[1] for u in p.units if u[1] >= 0) == [0, 1]
    for di, wi, col, _ in p.units:
        assert col == p.deep[di].col and (wi < 0 or p.wide[wi].col == col)
    assert len(p.table_params) == 8 and all(id(t) != id(e.weight) for t in p.table_params
                                            for e in m.embedding_dict.values())


def test_pair_plan_pickles_and_old_pickles_get_defaults():
    p = _pair_model().model_plan()
    q = pickle.loads(pickle.dumps(p))
    assert q.pair and q.ld_rows == 36 and q.width == 21 and [f.out_off for f in q.deep] == [0, 6, 12, 18, 24, 30]
    d = p.__getstate__()
    d.pop("pair")
    d.pop("ld_rows")                  # a plan pickled before the mode existed
    from deepctr_torch._hip.plan import EmbeddingPlan
    old = EmbeddingPlan.__new__(EmbeddingPlan)
    old.__setstate__(d)
    assert old.pair is False and old.ld_rows == 0


def test_pair_plan_binds(onn_mock):
    p = _pair_model().model_plan()
    p.bind("cpu")
    c = p.cplan
    assert c.n_deep == c.n_deep_fixed == 6 and c.emb_dim == c.max_dim == 6 and c.vec == 2 and c.dense_off == 18
    assert c.n_dense == 3 and c.n_wide == 2 and not c.out_chunks and not c.ext


def test_pair_mode_argument_checks():
    from deepctr_torch._hip.plan import EmbeddingPlan
    w = [torch.nn.Parameter(torch.zeros(5, d)) for d in (4, 4, 4, 8)]
    fi = {"a": (0, 1), "b": (1, 2)}
    with pytest.raises(ValueError):
        EmbeddingPlan(fi, deep_fields=[("x", w[0], 0), ("y", w[1], 1), ("z", w[2], 0)], pair=True)      # odd
    with pytest.raises(ValueError):
        EmbeddingPlan(fi, deep_fields=[("x", w[0], 0), ("y", w[3], 1)], pair=True)                      # mixed dims
    with pytest.raises(ValueError):
        EmbeddingPlan(fi, pair=True)                                                                    # no fields
    plain = EmbeddingPlan(fi, deep_fields=[("x", w[0], 0), ("y", w[3], 1)])      # explicit fields without the pair mode
    assert not plain.pair and [f.out_off for f in plain.deep] == [0, 4] and plain.width == 12 and plain.ld_rows == 0


def test_few_sparse_features_is_dnn_of_dense_plus_linear(onn_mock):
    g, m = _loaded("onn_one_sparse")
    p = m.model_plan()
    assert not p.deep and p.width == 2 and len(m.second_order_embedding_dict) == 0
    assert m.dnn.linears[0].weight.shape[1] == 2


# ---- multi-GPU trainers --------------------------------------------------------------------------------------------
def test_multi_gpu_trainers_refuse_the_pair_lookup(monkeypatch):
    import torch.distributed as dist
    from deepctr_torch import distributed_fit, parallel
    m = _pair_model()
    m.compile("adagrad", "binary_crossentropy")
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    for cls in (parallel.DataParallelTrainer, parallel.ShardedTrainer):
        with pytest.raises(NotImplementedError, match="pair lookup"):
            cls(m)
    with pytest.raises(NotImplementedError, match="pair lookup"):
        distributed_fit.fit(m, torch.zeros(4, 6), torch.zeros(4), 2, 1, 0, 0, False, None, None, False, None)


def test_pair_embed_refuses_exchange_and_sharder(onn_mock):
    from deepctr_torch._hip import ops
    m = _pair_model()
    p = m.model_plan()
    X = torch.zeros(3, 6)
    for attr in ("exchange", "sharder"):
        setattr(p, attr, object())
        with pytest.raises(NotImplementedError):
            ops.pair_embed(p, X)
        setattr(p, attr, None)
    with pytest.raises(ValueError):
        ops.pair_embed(m.linear_model.plan(), X)
