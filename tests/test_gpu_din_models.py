"""GPU: DIN against the golden vectors the real reference produced (tests/golden/din, tools/golden/make_din_golden.py), every
comparison against the reference alone, every element: pre-sigmoid logits and y_pred within 1e-5; every parameter and table
gradient within 2e-5 x max|g_ref| of that parameter; 3-step sgd / adagrad / preset-accumulator adagrad trajectories and the
default-kwargs adam run within 2e-5; fit() Histories and predict() with and without graph replay; state_dict keys; same-seed
initial weights.  Plus the fused route of AttentionSequencePoolingLayer against its own torch-op route, and a call-counting
proxy around the library: the kernel runs where the layer says it does (element-wise activations in both directions, frozen
Dice in predict) and does not where it must not (Dice whenever a gradient or batch statistics are involved)."""
import numpy as np
import pytest
import torch

import din_helpers as H
from helpers import load_golden, max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIT_RUNS = (("plain", "adagrad", 0.0, False), ("shuffled", "adagrad", 0.0, True), ("default", "adam", 1e-5, True))


class _Counting(object):
    """A proxy around the loaded library that counts the calls of every entry point and keeps the last arguments."""

    def __init__(self, lib):
        self._lib, self.n, self.args = lib, {}, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dctr_"):
            return fn

        def counted(*a, **k):
            self.n[name] = self.n.get(name, 0) + 1
            self.args[name] = a
            return fn(*a, **k)
        return counted


@pytest.fixture()
def counting(monkeypatch):
    from deepctr_torch._hip import lib as L
    proxy = _Counting(L.lib())
    monkeypatch.setattr(L, "lib", lambda: proxy)
    return proxy


def _dice(g):
    return g["spec"]["kwargs"].get("att_activation", "Dice") == "Dice"


@pytest.mark.parametrize("name", H.ALL)
def test_forward_matches_reference(counting, name):
    g, m = H.loaded(name, DEV)
    train = name != "din_dice_eval"
    H.check_forward(g, m, DEV, train)
    if _dice(g) and train:
        assert "dctr_din_attn_fwd" not in counting.n
    else:
        assert counting.n.get("dctr_din_attn_fwd") == 1 and counting.args["dctr_din_attn_fwd"][20] is None


@pytest.mark.parametrize("name", H.ALL)
def test_gradients_match_reference(counting, name):
    g, m = H.loaded(name, DEV)
    H.check_gradients(g, m, DEV, name != "din_dice_eval")
    torch.cuda.synchronize()
    if name in H.KERNEL_TRAIN:
        assert counting.n.get("dctr_din_attn_fwd") == 1 and counting.n.get("dctr_din_attn_bwd") == 1
        assert counting.args["dctr_din_attn_fwd"][20] is not None
        a = counting.args["dctr_din_attn_fwd"]
        assert a[0].value == a[2].value                  # the query and the keys are read in place from the gathered row
    else:
        assert "dctr_din_attn_fwd" not in counting.n and "dctr_din_attn_bwd" not in counting.n


@pytest.mark.parametrize("name", H.STEPS)
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adagradp"])
def test_optimizer_trajectory(counting, name, opt):
    g, m = H.loaded(name, DEV)
    H.check_trajectory(g, m, DEV, opt)
    torch.cuda.synchronize()
    m.model_plan().check_ids()
    assert counting.n.get("dctr_din_attn_bwd") == 3


def test_default_kwargs_adam_trajectory(counting):
    g = load_golden("din/din_default_adam")
    m = H.build_din(g["spec"], DEV, l2=1e-6)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    H.check_trajectory(g, m, DEV, "adam")
    assert "dctr_din_attn_fwd" not in counting.n         # default Dice in train mode: torch ops
    m.eval()
    with torch.no_grad():
        m(torch.from_numpy(g["X"]).to(DEV))
    assert counting.n.get("dctr_din_attn_fwd") == 1       # ... and the kernel in predict


@pytest.mark.parametrize("graphs", ["1", "0"])
@pytest.mark.parametrize("tag,opt,l2,shuffle", FIT_RUNS)
def test_fit_history_and_predict_match_reference(monkeypatch, tag, opt, l2, shuffle, graphs):
    from deepctr_torch.inputs import build_input_features
    from helpers import feature_columns
    monkeypatch.setenv("DCTR_FIT_GRAPH", graphs)
    g, m = H.loaded("fit_din", DEV, l2=l2)
    ex = g["extra"]
    m.compile(opt, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    fi = build_input_features(feature_columns(g["spec"]["dnn_columns"]))
    x = {n: (ex["fit_X"][:, lo] if hi - lo == 1 else ex["fit_X"][:, lo:hi]) for n, (lo, hi) in fi.items()}
    torch.manual_seed(777)
    hist = m.fit(x, ex["fit_y"], batch_size=64, epochs=3, verbose=2, validation_split=0.25, shuffle=shuffle)
    ref = {k[len("fit_%s_hist/" % tag):]: v for k, v in ex.items() if k.startswith("fit_%s_hist/" % tag)}
    assert set(hist.history) == set(ref)
    for k, v in ref.items():
        if k.endswith("auc"):
            np.testing.assert_allclose(hist.history[k], v, atol=5e-3, err_msg=k)
        else:
            np.testing.assert_allclose(hist.history[k], v, rtol=2e-4, err_msg=k)
    pred = m.predict(x, batch_size=50)
    assert pred.dtype == np.float64 and pred.shape == ex["fit_%s_pred" % tag].shape
    assert max_abs(pred, ex["fit_%s_pred" % tag]) <= 5e-5


@pytest.mark.parametrize("name", H.ALL)
def test_state_dict_keys_are_the_fixtures(name):
    g, m = H.loaded(name, DEV)
    sd = m.state_dict()
    assert list(sd) == list(g["params"])
    for k, v in g["params"].items():
        assert tuple(sd[k].shape) == v.shape, k


def test_same_seed_initial_weights_on_the_gpu_are_the_references():
    configs = H.init_configs()
    assert len(configs) == 2
    for spec, params in configs:
        sd = H.build_din(spec, DEV, l2=1e-6).state_dict()
        assert list(sd) == list(params)
        for k, v in params.items():
            assert np.array_equal(sd[k].cpu().numpy(), v), k


@pytest.mark.parametrize("name", ["din_sigmoid", "din_prelu", "din_softmax", "din_t50"])
def test_fused_route_equals_the_torch_op_route(counting, name):
    """The layer on the fixture's own embeddings: the kernel against the same module's formula as PyTorch-ROCm ops, values
    within 1e-5 x max, gradients within 2e-5 x max|g| (din_helpers.grad_scale's rule for the bias under a softmax)."""
    g, m = H.loaded(name, DEV)
    segs, T, _, _, queries, keys, off = m._layout()
    with torch.no_grad():
        gathered, _, _ = m.fused_inputs(torch.from_numpy(g["X"]).to(DEV))
    B = gathered.shape[0]
    q = torch.cat([gathered[:, off[c.name]:off[c.name] + c.embedding_dim] for c in queries], dim=-1)
    k = torch.cat([gathered[:, off[c.name + "[0]"]:off[c.name + "[0]"] + T * c.embedding_dim].reshape(B, T, -1)
                   for c in keys], dim=-1)
    q, k = q.unsqueeze(1).clone().requires_grad_(True), k.clone().requires_grad_(True)
    from deepctr_torch.inputs import build_input_features
    from helpers import feature_columns
    fi = build_input_features(feature_columns(g["spec"]["dnn_columns"]))
    n = torch.from_numpy(g["X"][:, fi["seq_length"][0]]).long().reshape(-1, 1).to(DEV)
    layer = m.attention
    fused = layer(q, k, n)
    assert counting.n.get("dctr_din_attn_fwd") == 1
    plain = layer._forward_torch(q, k, layer._valid(k, n, None))
    scale = float(plain.abs().max())
    assert fused.shape == plain.shape and max_abs(fused.detach().cpu().numpy(), plain.detach().cpu().numpy()) <= 1e-5 * scale
    go = torch.randn_like(plain)
    names = ["q", "k"] + [n_ for n_, _ in layer.named_parameters()]
    a = torch.autograd.grad(fused, [q, k] + list(layer.parameters()), go)
    b = torch.autograd.grad(plain, [q, k] + list(layer.parameters()), go)
    assert counting.n.get("dctr_din_attn_bwd") == 1
    sc = dict((n_, float(y.abs().max())) for n_, y in zip(names, b))
    if layer.weight_normalization:
        sc["local_att.dense.bias"] = sc["local_att.dense.weight"]
    for n_, x, y in zip(names, a, b):
        assert x.shape == y.shape and max_abs(x.cpu().numpy(), y.cpu().numpy()) <= H.GRAD_TOL * sc[n_], n_


def test_dice_routes(counting):
    """Default Dice: torch ops in train mode and whenever a gradient is needed, the kernel in eval mode under no_grad --
    and both give the fixture's eval-mode values."""
    g, m = H.loaded("din_dice_eval", DEV)
    X = torch.from_numpy(g["X"]).to(DEV)
    m.eval()
    with torch.no_grad():
        y_kernel = m(X)
    assert counting.n.get("dctr_din_attn_fwd") == 1 and counting.args["dctr_din_attn_fwd"][15] == 4
    counting.n.clear()
    y_torch = m(X)                                        # gradients enabled: the frozen form has no backward
    assert "dctr_din_attn_fwd" not in counting.n
    assert max_abs(y_kernel.cpu().numpy(), g["y_pred"]) <= H.LOGIT_TOL
    assert max_abs(y_torch.detach().cpu().numpy(), g["y_pred"]) <= H.LOGIT_TOL
    m.train()
    with torch.no_grad():
        m(X)
    assert "dctr_din_attn_fwd" not in counting.n


def test_shape_outside_the_kernel_runs_the_torch_ops(counting):
    from deepctr_torch.inputs import SparseFeat, VarLenSparseFeat
    from deepctr_torch.models import DIN
    torch.manual_seed(1)
    cols = [SparseFeat("item", 9, 4),
            VarLenSparseFeat(SparseFeat("hist_item", 9, 4, embedding_name="item"), 5, length_name="seq_length")]
    m = DIN(cols, ["item"], dnn_hidden_units=(8,), att_hidden_size=(8, 4, 4, 4), att_activation="sigmoid", init_std=0.1,
            device=DEV)
    rng = np.random.RandomState(0)
    X = np.concatenate([rng.randint(0, 9, (7, 1)), rng.randint(1, 9, (7, 5)), rng.randint(0, 6, (7, 1))], axis=1)
    X = torch.from_numpy(X.astype(np.float32)).to(DEV)
    m.train()
    y = m(X)
    y.sum().backward()
    torch.cuda.synchronize()
    assert "dctr_din_attn_fwd" not in counting.n and "dctr_din_attn_bwd" not in counting.n
    assert tuple(y.shape) == (7, 1) and bool(torch.isfinite(y).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.attention.parameters())
