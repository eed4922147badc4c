"""CPU: MLR through the real Python stack over the stand-in for the library (tests/mock_lib.py + mock_iafm.py for the
per-field gather / update, extended by tests/mock_mlr.py with the mixture's entry points), against the reference's golden
values (tests/golden/mlr, tools/golden/make_mlr_golden.py): y within 1e-5, every parameter gradient within 2e-5 x
max|g_ref| (no floor of 1 for the region and bias sides), the 3-step SGD / Adagrad trajectories, the 8-step runs of the lazy
fixture, the fit() History.  Plus what needs no library at all: the plan's several-sided wide mode, same-seed initial
weights, the constructor's ValueError, the multi-rank refusal.  The kernels themselves are checked by
tests/test_gpu_mlr_kernel.py, the model on the GPU by tests/test_gpu_mlr_models.py."""
import pickle

import numpy as np
import pytest
import torch

import mock_mlr
from helpers import max_abs
from mlr_helpers import (FIT_RUNS, FORWARD, GRAD_TOL, STEPS, TRAJ_TOL, Y_TOL, build, fit_inputs, grad_scale, init_configs,
                         load, loaded, loss_name, loss_sum)

DEV = "cpu"


@pytest.fixture()
def mlr_mock(mock):
    return mock_mlr.extend(mock)


def test_model_is_exported():
    import deepctr_torch.models as M
    from deepctr_torch.models import MLR
    assert M.MLR is MLR and "MLR" in M.__all__


# ---- state_dict / initial weights ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORWARD)
def test_state_dict_keys_and_shapes_are_the_references(name):
    g = load(name)
    sd = build(g["spec"], DEV).state_dict()
    assert list(sd) == list(g["params"])
    for k, v in g["params"].items():
        assert tuple(sd[k].shape) == v.shape, k


def test_init_fixture_exists():
    assert len(init_configs()) == 2


@pytest.mark.parametrize("c", init_configs(), ids=lambda c: "R%d" % c[0]["kwargs"].get("region_num", 4))
def test_same_seed_initial_weights_are_the_references(c):
    spec, params = c
    sd = build(spec, DEV).state_dict()
    assert list(sd) == list(params)
    for k, v in params.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert np.array_equal(sd[k].numpy(), v), k


# ---- the model over the stand-in -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FORWARD)
def test_forward_matches_reference(mlr_mock, name):
    g, m = loaded(name, DEV)
    with torch.no_grad():
        y = m(torch.from_numpy(g["X"]))
    m.model_plan().check_ids()
    assert y.shape == (g["X"].shape[0], 1)
    assert max_abs(y.numpy(), g["y_pred"]) <= Y_TOL
    # one launch of the mixture per forward on the fused route, no gather
    assert mlr_mock.calls.count("mlr_fwd") == 1 and "embed_fwd" not in mlr_mock.calls


def _backward(g, m):
    m.train()
    loss = loss_sum(g["spec"], m(torch.from_numpy(g["X"])).squeeze(1), torch.from_numpy(g["y"]))
    m.zero_grad()
    loss.backward()
    return loss


@pytest.mark.parametrize("name", FORWARD)
def test_gradients_match_reference(mlr_mock, name):
    g, m = loaded(name, DEV)
    loss = _backward(g, m)
    assert abs(loss.item() - g["loss"]) <= 1e-4 * max(1.0, abs(g["loss"]))
    assert set(g["grads"]) == set(k for k, _ in m.named_parameters())
    for k, p in m.named_parameters():
        ref = g["grads"][k]
        got = p.grad.numpy() if p.grad is not None else np.zeros_like(ref)
        err = max_abs(got, ref)
        assert err <= GRAD_TOL * grad_scale(k, ref), "%s: max|d|=%.3e max|g_ref|=%.3g" % (k, err, np.max(np.abs(ref)))
        if k.startswith(("base_linear_model.", "embedding_dict.", "linear_model.")):
            assert p.grad is None or not p.grad.any(), "%s: the output never depends on it" % k
    assert mlr_mock.calls.count("mlr_bwd") == 1


@pytest.mark.parametrize("name", ["mlr_bias", "mlr_mixed", "mlr_dense_only", "mlr_regression"])
def test_composed_route_matches(mlr_mock, monkeypatch, name):
    """DCTR_MLR=0: one per-field gather on the same plan + torch ops -- the same values within the bars."""
    monkeypatch.setenv("DCTR_MLR", "0")
    g, m = loaded(name, DEV)
    _backward(g, m)
    with torch.no_grad():
        y = m(torch.from_numpy(g["X"]))
    assert max_abs(y.numpy(), g["y_pred"]) <= Y_TOL
    for k, p in m.named_parameters():
        ref = g["grads"][k]
        got = p.grad.numpy() if p.grad is not None else np.zeros_like(ref)
        assert max_abs(got, ref) <= GRAD_TOL * grad_scale(k, ref), k
    assert "mlr_fwd" not in mlr_mock.calls and "mlr_bwd" not in mlr_mock.calls
    assert mlr_mock.calls.count("embed_fwd") == (2 if m.model_plan().wide else 0)      # (train forward + eval forward)


def test_refused_plan_runs_composed(mlr_mock):
    """The envelope switch-over: a plan the kernel refuses runs composed and still matches."""
    g, m = loaded("mlr_bias", DEV)
    mlr_mock.dctr_mlr_supported = lambda pref, mref: 0
    _backward(g, m)
    with torch.no_grad():
        y = m(torch.from_numpy(g["X"]))
    assert max_abs(y.numpy(), g["y_pred"]) <= Y_TOL
    for k, p in m.named_parameters():
        ref = g["grads"][k]
        got = p.grad.numpy() if p.grad is not None else np.zeros_like(ref)
        assert max_abs(got, ref) <= GRAD_TOL * grad_scale(k, ref), k
    assert "mlr_fwd" not in mlr_mock.calls and mlr_mock.calls.count("embed_fwd") == 2


@pytest.mark.parametrize("name", STEPS)
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adagradp"])
def test_in_kernel_optimizer_trajectory(mlr_mock, name, opt):
    g, m = loaded(name, DEV)
    start = {k: v.clone() for k, v in m.state_dict().items()}
    m.compile("adagrad" if opt == "adagradp" else opt, loss_name(g["spec"]), metrics=[])
    if opt == "adagradp":
        for grp in m.optim.param_groups:
            for p in grp["params"]:
                m.optim.state[p]["sum"].fill_(0.05)
    m.train()
    losses = [float(m._train_step(torch.from_numpy(Xb), torch.from_numpy(yb))[0])
              for Xb, yb in zip(g["extra"]["X_steps"], g["extra"]["y_steps"])]
    plan = m.model_plan()
    assert plan.update[0] == ("sgd" if opt == "sgd" else "adagrad")
    if plan.unit_path:
        assert "embed_update:%d" % (0 if opt == "sgd" else 1) in mlr_mock.calls
    assert "embed_fwd" not in mlr_mock.calls and mlr_mock.calls.count("mlr_fwd") == 3
    np.testing.assert_allclose(losses, g["extra"][opt + "3_loss"], rtol=2e-5)
    sd = m.state_dict()
    n = 0
    for k, v in g["extra"].items():
        if k.startswith(opt + "3/"):
            key = k[len(opt) + 2:]
            assert max_abs(sd[key].numpy(), v) <= TRAJ_TOL, k
            if key.startswith("base_linear_model."):
                assert torch.equal(sd[key], start[key]), "%s moved" % key
            if key.startswith(("embedding_dict.", "linear_model.")) and start[key].abs().max() > 0:
                assert not torch.equal(sd[key], start[key]), "%s: the dead groups decay under their L2" % key
            n += 1
    assert n == len(sd)


@pytest.mark.parametrize("tag,opt,mode", [("sgd", "sgd", ("sgd",)), ("adagrad", "adagrad", ("adagrad",)),
                                          ("adam", "adam", ("lazy", "adam")), ("adam0", "adam", ("lazy", "adam"))])
def test_lazy_fixture_runs_replay_reference(mlr_mock, tag, opt, mode):
    """The 8-step runs of the lazy fixture.  ``l2_reg_linear`` does nothing in MLR, so SGD and Adagrad stay on the fused sorted
    update whatever its value; Adam takes the lazy update (moments that keep decaying between two touches)."""
    g, m = loaded("lazy_mlr", DEV, l2_reg_linear=0.0 if tag == "adam0" else 1e-3)
    ex = g["extra"]
    m.compile(opt, "binary_crossentropy", metrics=[])
    m.train()
    assert m.model_plan().update[:len(mode)] == mode
    bce, tot = [], []
    for Xb, yb in zip(ex["lazy_X"], ex["lazy_y"]):
        loss, total, _ = m._train_step(torch.from_numpy(Xb), torch.from_numpy(yb))
        bce.append(float(loss))
        tot.append(float(total))
    np.testing.assert_allclose(bce, ex["lazy_%s_bce" % tag], rtol=2e-5)
    np.testing.assert_allclose(tot, ex["lazy_%s_total" % tag], rtol=2e-5)
    sd = m.state_dict()
    pre = "lazy_%s/" % tag
    for k, v in ex.items():
        if k.startswith(pre):
            ref = np.asarray(v, np.float64)
            assert max_abs(sd[k[len(pre):]].numpy(), ref) <= TRAJ_TOL * max(1.0, float(np.max(np.abs(ref)))), k
    m.eval()
    with torch.no_grad():
        assert max_abs(m(torch.from_numpy(ex["lazy_X"][0])).numpy(), ex["lazy_%s_pred" % tag]) <= 5e-5


@pytest.mark.parametrize("tag,opt,l2,shuffle", FIT_RUNS)
def test_fit_history_and_predict_match_reference(mlr_mock, monkeypatch, tag, opt, l2, shuffle):
    monkeypatch.setenv("DCTR_FIT_GRAPH", "0")            # (no device to capture on; the GPU file runs both ways)
    g, m = loaded("fit_mlr", DEV, l2_reg_linear=l2)
    ex = g["extra"]
    m.compile(opt, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    x = fit_inputs(m, ex["fit_X"])
    torch.manual_seed(777)
    hist = m.fit(x, ex["fit_y"], batch_size=64, epochs=3, verbose=0, validation_split=0.25, shuffle=shuffle)
    ref = {k[len("fit_%s_hist/" % tag):]: v for k, v in ex.items() if k.startswith("fit_%s_hist/" % tag)}
    assert set(hist.history) == set(ref)
    for k, v in ref.items():
        if k.endswith("auc"):
            np.testing.assert_allclose(hist.history[k], v, atol=5e-3, err_msg=k)
        else:
            np.testing.assert_allclose(hist.history[k], v, rtol=2e-4, err_msg=k)
    pred = m.predict(x, batch_size=50)
    assert pred.shape == ex["fit_%s_pred" % tag].shape
    assert max_abs(pred, ex["fit_%s_pred" % tag]) <= 5e-5


def test_default_kwargs_take_the_fused_sorted_update(mlr_mock):
    """The dead embedding_dict / linear_model carry L2 1e-5; the plan's tables carry none: adagrad stays in the kernel."""
    g = load("mlr_bias")
    m = build(g["spec"], DEV)
    assert [l2 for _, _, l2 in m.regularization_weight] == [1e-5, 1e-5]
    m.compile("adagrad", "binary_crossentropy")
    assert m.model_plan().update[0] == "adagrad"
    m.compile("sgd", "binary_crossentropy")
    assert m.model_plan().update[0] == "sgd"
    m.compile("adam", "binary_crossentropy")
    assert m.model_plan().update == ("lazy", "adam")


# ---- the plan ------------------------------------------------------------------------------------------------------
def _small(varlen=False, bias=True, region_num=3):
    from deepctr_torch.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    from deepctr_torch.models import MLR
    region = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4), DenseFeat("x", 2)]
    if varlen:
        region.append(VarLenSparseFeat(SparseFeat("h", 7, 4), 3, "mean"))
    base = [SparseFeat("p", 4, 4), DenseFeat("q", 1)]
    bias_cols = [SparseFeat("c", 3, 4), DenseFeat("x", 2), DenseFeat("y", 1)] if bias else None
    return MLR(region, base, bias_cols, region_num=region_num)


def test_plan_fields_heads_and_tables():
    m = _small()
    p = m.model_plan()
    fi = m.feature_index
    assert list(fi) == ["a", "b", "x", "p", "q", "c", "y"]
    assert not p.deep and p.wide_per_field and p.wide_dense_weight is None and not p.dense_cols and not p.wdense_cols
    assert [f.name for f in p.wide] == ["a", "b"] * 3 + ["c"]
    assert p.head_of == [0, 0, 1, 1, 2, 2, 3]
    assert [f.col for f in p.wide] == [fi["a"][0], fi["b"][0]] * 3 + [fi["c"][0]]
    for r in range(3):
        assert p.wide[2 * r].param is m.region_linear_model[r].embedding_dict["a"].weight
    assert p.wide[6].param is m.bias_model[0].embedding_dict["c"].weight
    assert p.side_dense_cols == [[2, 3]] * 3 + [[2, 3, fi["y"][0]]]
    assert p.ld_wide == 8 and p.n_wide_fixed == 7
    assert p.simple_units and p.unit_path and p.gen is None and len(p.units) == 7
    assert [u[1] for u in p.units] == list(range(7)) and all(u[0] == -1 for u in p.units)
    dead = [q for mod in (m.base_linear_model, m.embedding_dict, m.linear_model) for q in mod.parameters()]
    assert len(p.table_params) == 7 and not set(id(t) for t in p.table_params) & set(id(q) for q in dead)
    h = m.mlr_heads()
    assert h.n_regions == 3 and h.has_bias and h.dense_off == [0, 2, 4, 6, 9] and h.n_dense == 9
    assert h.weights[1] is m.region_linear_model[1].weight and h.weights[3] is m.bias_model[0].weight


def test_plan_with_varlen_columns_takes_general_units():
    p = _small(varlen=True).model_plan()
    assert [f.name for f in p.wide] == ["a", "b"] * 3 + ["c"] + ["h"] * 3
    assert p.head_of == [0, 0, 1, 1, 2, 2, 3, 0, 1, 2] and p.n_wide_fixed == 7
    assert not p.simple_units and p.unit_path and p.gen is not None
    assert sorted(s["wfield"] for s in p.gen["slots"] if s["pool"] == 2) == [7, 7, 7, 8, 8, 8, 9, 9, 9]


def test_wide_sides_argument_checks():
    from deepctr_torch._hip.plan import EmbeddingPlan
    m = _small(bias=False, region_num=2)
    lm = m.region_linear_model[0]
    with pytest.raises(ValueError, match="wide_sides"):
        EmbeddingPlan(m.feature_index, wide_columns=m.region_feature_columns, wide_tables=lm.embedding_dict,
                      wide_sides=[(m.region_feature_columns, lm.embedding_dict)])
    assert m.model_plan().head_of == [0, 0, 1, 1] and m.mlr_heads().n_heads == 2
    plain = EmbeddingPlan(m.feature_index, wide_columns=m.region_feature_columns, wide_tables=lm.embedding_dict)
    assert plain.head_of is None and plain.side_dense_cols is None


def test_plan_pickles_and_old_pickles_get_defaults():
    from deepctr_torch._hip.plan import EmbeddingPlan
    p = _small().model_plan()
    q = pickle.loads(pickle.dumps(p))
    assert q.head_of == p.head_of and q.side_dense_cols == p.side_dense_cols
    d = p.__getstate__()
    d.pop("head_of")
    d.pop("side_dense_cols")                  # a plan pickled before the mode existed
    old = EmbeddingPlan.__new__(EmbeddingPlan)
    old.__setstate__(d)
    assert old.head_of is None and old.side_dense_cols is None


# ---- constructor, trainers, pickling -------------------------------------------------------------------------------
def test_constructor_errors_and_defaults():
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    from deepctr_torch.models import MLR
    cols = [SparseFeat("a", 5, 4), DenseFeat("x", 1)]
    for r in (1, 0, -2):
        with pytest.raises(ValueError, match="region_num must > 1"):
            MLR(cols, region_num=r)
    m = MLR(cols, base_feature_columns=[], region_num=2, init_std=0.5, l2_reg_linear=0.3, seed=7)
    assert m.base_feature_columns is cols and m.bias_feature_columns == [] and not hasattr(m, "bias_model")
    assert (m.l2_reg_linear, m.init_std, m.seed, m.region_num) == (0.3, 0.5, 7, 2)
    assert len(m.region_linear_model) == len(m.base_linear_model) == 2
    assert m.region_linear_model[0].embedding_dict["a"].weight.std() > 0.1       # init_std reaches every Linear
    assert m.prediction_layer.task == "binary" and not m.prediction_layer.use_bias


def test_fit_refuses_several_ranks(monkeypatch):
    m = _small()
    m.compile("adagrad", "binary_crossentropy")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        m.fit({}, np.zeros(4), batch_size=2)


def test_pickle_round_trip(mlr_mock):
    g, m = loaded("mlr_bias", DEV)
    m.compile("adagrad", "binary_crossentropy", metrics=[])
    X = torch.from_numpy(g["X"])
    with torch.no_grad():
        y = m(X)
    m2 = pickle.loads(pickle.dumps(m))
    assert list(m2.state_dict()) == list(m.state_dict())
    with torch.no_grad():
        assert torch.equal(m2(X), y)
    m2.train()
    m2._train_step(X, torch.from_numpy(g["y"]))
    assert m2.mlr_heads().plan is m2.model_plan()
    sd = {k: v.clone() for k, v in m2.state_dict().items()}
    m3 = build(g["spec"], DEV)
    m3.load_state_dict(sd)
    with torch.no_grad():
        assert torch.equal(m3(X), m2.eval()(X))
