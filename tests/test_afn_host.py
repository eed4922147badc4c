"""CPU: AFN through the real Python stack over the stand-in for the library (tests/mock_lib.py + mock_ops.py, extended by
tests/mock_afn.py with the logarithmic transformation layer's entry points), against the reference's values
(tests/golden/afn, tools/golden/make_afn_golden.py): logits within 1e-5 of the float32 reference; every parameter gradient
and 3-step trajectory against the reference's FLOAT64 run, within max(2e-5, 4 x the float32 reference's own deviation from
it) -- tests/afn_helpers.py says why.  Plus what needs no library: exports, same-seed initial weights, state_dict keys, the
two ValueErrors, ``_kernel_fits``, the torch route.  The kernels themselves are checked by tests/test_gpu_afn_kernel.py,
the model on the GPU by tests/test_gpu_afn_models.py."""
import json
import os

import numpy as np
import pytest
import torch

import mock_afn
from afn_helpers import (ALL, GRAD_DEV, LOGIT_DEV, LOGIT_TOL, STEPS, check_gradients, check_trajectory, loaded, run_steps)
from helpers import GOLDEN_DIR, build_model, feature_columns, golden_names, load_golden, max_abs

DEV = "cpu"


@pytest.fixture()
def afn_mock(mock):
    return mock_afn.extend(mock)


def test_model_and_layers_are_exported():
    import deepctr_torch.layers as Ly
    import deepctr_torch.models as M
    from deepctr_torch._hip.ops import LogTransformFunction  # noqa: F401
    from deepctr_torch.layers import LogTransformLayer
    from deepctr_torch.models import AFN
    assert M.AFN is AFN and "AFN" in M.__all__
    assert Ly.LogTransformLayer is LogTransformLayer


def test_fixture_set_and_stored_margins():
    assert golden_names("afn/") == sorted(ALL + ["init"])
    for name in ALL:
        path = os.path.join(GOLDEN_DIR, "afn", name + ".npz")
        z = np.load(path, allow_pickle=False)
        assert float(z["logit_dev"]) <= LOGIT_DEV and float(z["grad_dev"]) <= GRAD_DEV, name
        assert os.path.getsize(path) < 1 << 20
        g = load_golden("afn/" + name)
        # where the generator's own keys land: nothing of them among the parameters or the float32 gradients
        assert set(g["grads"]) == set(k for k in g["params"] if "running" not in k and "num_batches" not in k)
        assert all("ref64/grad/" + k in g["extra"] for k in g["grads"]) and "ref64/logit" in g["extra"]
        assert max_abs(g["logit"], g["extra"]["ref64/logit"]) == float(z["logit_dev"])
    ex = load_golden("afn/fit_afn")["extra"]
    for tag in ("sgd", "adagradp", "default"):
        assert "fit_%s_hist/loss" % tag in ex and ("fit_%s_pred" % tag in ex) == (tag != "default")
    for name in STEPS:
        ex = load_golden("afn/" + name)["extra"]
        assert all(k in ex for k in ("ref64/sgd3_loss", "ref64/adagradp3_loss", "adagrad3_loss"))


@pytest.mark.parametrize("name", ALL)
def test_forward_matches_reference(afn_mock, name):
    g, m = loaded(name, DEV)
    m.train()
    cap = {}
    h = m.out.register_forward_pre_hook(lambda mod, inp: cap.__setitem__("logit", inp[0].detach()))
    with torch.no_grad():
        y = m(torch.from_numpy(g["X"]))
    h.remove()
    m.model_plan().check_ids()
    assert max_abs(cap["logit"].numpy(), g["logit"]) <= LOGIT_TOL
    assert max_abs(y.numpy(), g["y_pred"]) <= LOGIT_TOL
    assert afn_mock.calls.count("log_transform_fwd_train") == 1 and "log_transform_bwd" not in afn_mock.calls


def _gradients(g, m):
    m.train()
    loss = torch.nn.functional.binary_cross_entropy(m(torch.from_numpy(g["X"])).squeeze(1), torch.from_numpy(g["y"]),
                                                    reduction="sum")
    m.zero_grad()
    loss.backward()
    assert abs(loss.item() - g["loss"]) <= 1e-4 * max(1.0, abs(g["loss"]))
    return {k: (p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
            for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", ALL)
def test_gradients_match_float64_reference(afn_mock, name):
    g, m = loaded(name, DEV)
    worst = check_gradients(g, _gradients(g, m), name)
    print("%s: worst gradient error / bound = %.3f" % (name, worst))
    assert afn_mock.calls.count("log_transform_fwd_train") == 1 and afn_mock.calls.count("log_transform_bwd") == 1


@pytest.mark.parametrize("name", ["afn_two", "afn_varlen", "afn_sigmoid"])
def test_torch_route_gives_the_same_values(afn_mock, monkeypatch, name):
    monkeypatch.setenv("DCTR_LOG_TRANSFORM", "0")
    g, m = loaded(name, DEV)
    grads = _gradients(g, m)
    assert not any(c.startswith("log_transform") for c in afn_mock.calls)
    check_gradients(g, grads, name)
    with torch.no_grad():
        y = m(torch.from_numpy(g["X"]))
    assert max_abs(y.numpy(), g["y_pred"]) <= LOGIT_TOL


@pytest.mark.parametrize("name", STEPS)
@pytest.mark.parametrize("opt", ["sgd", "adagradp"])
def test_trajectory_and_running_statistics(afn_mock, name, opt):
    """three steps after the reference's first forward: every ``state_dict`` entry -- the running statistics of all four
    BatchNorms and their ``num_batches_tracked`` (4: one forward, three steps) among them"""
    g, m = loaded(name, DEV)
    losses = run_steps(g, m, opt, DEV)
    plan = m.model_plan()
    assert plan.update[0] != "dense", plan.update
    ltl = set(id(p) for p in m.ltl.parameters())
    assert ltl and not ltl & set(id(p) for p in plan.table_params)
    np.testing.assert_allclose(losses, g["extra"]["ref64/%s3_loss" % opt], rtol=2e-5)
    sd = m.state_dict()
    assert int(sd["ltl.bn.0.num_batches_tracked"]) == 4 and int(sd["ltl.bn.1.num_batches_tracked"]) == 4
    check_trajectory(g, opt, sd, name)


@pytest.mark.parametrize("name", STEPS)
def test_adagrad_from_zero_losses(afn_mock, name):
    """from zero accumulators the zero-gradient parameters step by +-lr on the sign of rounding noise; train-mode BatchNorm
    cancels them exactly, so the LOSSES are the reference's, the parameters are not compared"""
    g, m = loaded(name, DEV)
    np.testing.assert_allclose(run_steps(g, m, "adagrad", DEV), g["extra"]["adagrad3_loss"], rtol=2e-5)


def test_eval_forward_is_one_launch(afn_mock):
    g, m = loaded("afn_two", DEV)
    m.eval()
    with torch.no_grad():
        y = m(torch.from_numpy(g["X"]))
    assert afn_mock.calls.count("log_transform_fwd_eval") == 1 and "log_transform_fwd_train" not in afn_mock.calls
    ref = build_model(g["spec"], DEV)
    ref.load_state_dict(m.state_dict())
    ref.eval()
    os.environ["DCTR_LOG_TRANSFORM"] = "0"
    try:
        with torch.no_grad():
            want = ref(torch.from_numpy(g["X"]))
    finally:
        del os.environ["DCTR_LOG_TRANSFORM"]
    assert max_abs(y.numpy(), want.numpy()) <= LOGIT_TOL
    assert int(m.ltl.bn[0].num_batches_tracked) == 0


@pytest.mark.parametrize("name", ALL)
def test_state_dict_keys_are_the_references(name):
    g = load_golden("afn/" + name)
    m = build_model(g["spec"], DEV)
    assert list(m.state_dict()) == list(g["params"])
    assert [k for k in m.state_dict() if k.startswith("ltl.")] == ["ltl.ltl_weights", "ltl.ltl_biases"] + [
        "ltl.bn.%d.%s" % (i, s) for i in range(2)
        for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    assert tuple(m.ltl.ltl_biases.shape) == (1, 1, g["spec"]["kwargs"]["ltl_hidden_size"])


def _init_configs():
    path = os.path.join(GOLDEN_DIR, "afn", "init.npz")
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


@pytest.mark.parametrize("c", _init_configs(), ids=lambda c: "%ds" % len(c[0]["dnn_columns"]))
def test_same_seed_initial_weights_are_the_references(c):
    from deepctr_torch.models import AFN
    spec, params = c
    cols = feature_columns(spec["dnn_columns"])
    sd = AFN(cols, cols, device="cpu", **spec["kwargs"]).state_dict()
    assert list(sd) == list(params)
    for k, v in params.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert np.array_equal(sd[k].numpy(), v), k


def test_value_errors(afn_mock):
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    from deepctr_torch.models import AFN
    a, b = SparseFeat("a", 5, 4), SparseFeat("b", 6, 4)
    m = AFN([a, b], [a, b, DenseFeat("x", 1)], ltl_hidden_size=4, afn_dnn_hidden_units=(4,))      # dense: ignored
    assert tuple(m.ltl.ltl_weights.shape) == (2, 4)
    m.train()
    assert tuple(m(torch.tensor([[1., 2., .5], [0., 3., .1], [2., 1., .7]])).shape) == (3, 1)
    m._plan = None
    m.dnn_feature_columns = []
    with pytest.raises(ValueError, match="Sparse embeddings not provided"):
        m(torch.zeros(3, 3))
    shared = SparseFeat("b", 5, 4, embedding_name="a")
    m = AFN([a, shared], [a, shared], ltl_hidden_size=4, afn_dnn_hidden_units=(4,))
    with pytest.raises(ValueError, match="one embedding table per embedded field: 2 fields share 1 tables"):
        m(torch.zeros(3, 2))


def test_kernel_fits_at_its_edges():
    from deepctr_torch.layers import LogTransformLayer
    fits = LogTransformLayer._kernel_fits
    assert fits(1, 1, 1) and fits(64, 64, 1024) and fits(26, 16, 256)
    assert not fits(65, 16, 256) and not fits(26, 65, 256) and not fits(26, 16, 1025)
    assert not fits(0, 16, 256) and not fits(26, 0, 256) and not fits(26, 16, 0)
    for args in [(1, 1, 1), (64, 64, 1024), (65, 1, 1), (1, 65, 1), (1, 1, 1025)]:
        assert fits(*args) == mock_afn.fits(*args)


def test_layer_routes(afn_mock):
    """outside the envelope, in another dtype and with a gradient asked for in eval mode the layer runs the reference's op
    sequence; a batch of one value per channel is refused in train mode as ``nn.BatchNorm1d`` refuses it"""
    from deepctr_torch.layers import LogTransformLayer
    torch.manual_seed(0)
    big = LogTransformLayer(65, 4, 8)
    assert tuple(big(torch.randn(6, 65, 4)).shape) == (6, 32) and afn_mock.calls == []
    dbl = LogTransformLayer(3, 4, 8).double()
    assert dbl(torch.randn(6, 3, 4, dtype=torch.float64)).dtype == torch.float64 and afn_mock.calls == []
    layer = LogTransformLayer(3, 4, 8)
    x = torch.randn(6, 3, 4)
    fused = layer(x)
    assert afn_mock.calls == ["log_transform_fwd_train"] and int(layer.bn[1].num_batches_tracked) == 1
    twin = LogTransformLayer(3, 4, 8)
    twin.load_state_dict({k: v for k, v in layer.state_dict().items() if "running" not in k and "num_b" not in k},
                         strict=False)
    want = twin._torch_route(x)
    assert max_abs(fused.detach().numpy(), want.detach().numpy()) <= 1e-5
    for i in range(2):
        assert max_abs(layer.bn[i].running_mean.numpy(), twin.bn[i].running_mean.numpy()) <= 1e-6
        assert max_abs(layer.bn[i].running_var.numpy(), twin.bn[i].running_var.numpy()) <= 1e-6
    layer.eval()
    del afn_mock.calls[:]
    layer(x)                                          # parameters require grad, grad mode on: the torch route
    assert afn_mock.calls == []
    with torch.no_grad():
        layer(x)
    assert afn_mock.calls == ["log_transform_fwd_eval"]
    layer.train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        LogTransformLayer(1, 4, 8)(torch.randn(1, 1, 4))
