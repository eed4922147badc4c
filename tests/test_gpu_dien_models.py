"""GPU: DIEN against the golden vectors the real reference produced (tests/golden/dien, tools/golden/make_dien_golden.py),
every comparison against the reference alone, every element: pre-sigmoid logits and y_pred within 1e-5, the auxiliary loss,
every parameter and table gradient within 2e-5 x max|g_ref| of that parameter; 3-step sgd / adagrad / preset-accumulator
adagrad trajectories and the default-kwargs adam run; fit() Histories and predict() with and without graph replay -- and
that the replay really is one: the step is captured, which a single host synchronisation inside it would prevent; state_dict
keys; same-seed initial weights.  Plus the fused route against ``DCTR_GRU_SEQ=0`` on the same model, and a call-counting proxy
around the library: the recurrence kernel runs twice per direction and step for every gru_type, reading the keys in place."""
import warnings

import numpy as np
import pytest
import torch

import dien_helpers as H
from helpers import load_golden, max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIT_RUNS = (("plain", "adagrad", 0.0, False), ("shuffled", "adagrad", 0.0, True), ("default", "adam", 1e-5, True))


class _Counting(object):
    """A proxy around the loaded library that counts the calls of every entry point and keeps every call's arguments."""

    def __init__(self, lib):
        self._lib, self.n, self.args = lib, {}, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dctr_"):
            return fn

        def counted(*a, **k):
            self.n[name] = self.n.get(name, 0) + 1
            self.args.setdefault(name, []).append(a)
            return fn(*a, **k)
        return counted


@pytest.fixture()
def counting(monkeypatch):
    from deepctr_torch._hip import lib as L
    proxy = _Counting(L.lib())
    monkeypatch.setattr(L, "lib", lambda: proxy)
    return proxy


def _modes(counting, entry):
    return [a[10] for a in counting.args.get(entry, [])]


def _expected_modes(g):
    gt = H.gru_type(g)
    return [0, H.MODES[gt]]


@pytest.mark.parametrize("name", H.ALL)
def test_forward_matches_reference(counting, name):
    g, m = H.loaded(name, DEV)
    H.check_forward(g, m, DEV)
    assert _modes(counting, "dctr_gru_seq_fwd") == _expected_modes(g) and "dctr_gru_seq_bwd" not in counting.n
    assert all(a[16] is None for a in counting.args["dctr_gru_seq_fwd"])          # no gradient: no gates buffer
    # GRU: the attention kernel pools the second recurrence's states; the others score with torch ops
    assert counting.n.get("dctr_din_attn_fwd", 0) == (1 if H.gru_type(g) == "GRU" else 0)


@pytest.mark.parametrize("name", H.ALL)
def test_gradients_match_reference(counting, name):
    g, m = H.loaded(name, DEV)
    H.check_gradients(g, m, DEV)
    torch.cuda.synchronize()
    assert _modes(counting, "dctr_gru_seq_fwd") == _expected_modes(g)
    assert _modes(counting, "dctr_gru_seq_bwd") == _expected_modes(g)[::-1]       # two launches per direction
    ext = counting.args["dctr_gru_seq_fwd"][0]
    T = [c["maxlen"] for c in g["spec"]["dnn_columns"] if c["name"].startswith("hist_")][0]
    Hd = sum(c["dim"] for c in g["spec"]["dnn_columns"] if c["name"] in g["spec"]["history_feature_list"])
    assert ext[1] > T * Hd and ext[4] == len(g["spec"]["history_feature_list"])   # the keys in place in the gathered row
    assert all(a[16] is not None for a in counting.args["dctr_gru_seq_fwd"])


@pytest.mark.parametrize("name", H.STEPS)
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adagradp"])
def test_optimizer_trajectory(counting, name, opt):
    g, m = H.loaded(name, DEV)
    H.check_trajectory(g, m, DEV, opt)
    torch.cuda.synchronize()
    m.model_plan().check_ids()
    assert counting.n.get("dctr_gru_seq_fwd") == 6 and counting.n.get("dctr_gru_seq_bwd") == 6


def test_default_kwargs_adam_trajectory(counting):
    g = load_golden("dien/dien_default_adam")
    m = H.build_dien(g["spec"], DEV, l2=1e-6)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    H.check_trajectory(g, m, DEV, "adam")
    assert counting.n.get("dctr_gru_seq_bwd") == 6


@pytest.mark.parametrize("graphs", ["1", "0"])
@pytest.mark.parametrize("tag,opt,l2,shuffle", FIT_RUNS)
def test_fit_history_and_predict_match_reference(monkeypatch, tag, opt, l2, shuffle, graphs):
    monkeypatch.setenv("DCTR_FIT_GRAPH", graphs)
    g, m = H.loaded("fit_dien", DEV, l2=l2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                    # a capture that fails is reported as a warning
        H.check_fit(g, m, tag, opt, shuffle)
    graph = (m._fit_graph or {}).get("graph")
    if graphs == "1" and opt == "adagrad":
        # the lengths stay on the device and the auxiliary loss is computed there: the whole step was captured, which one
        # host synchronisation inside it would have made impossible, and fit() replayed it
        assert graph is not None
    else:
        assert graph is None                              # (torch's Adam keeps its step count on the host)


def test_captured_step_has_no_host_synchronisation():
    """the train step of the negative-sampling model, captured directly: stream capture refuses every synchronising call"""
    g, m = H.loaded("dien_augru_neg", DEV)
    m.compile("adagrad", "binary_crossentropy", metrics=[])
    m.train()
    X, y = torch.from_numpy(g["X"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    for _ in range(2):
        m._train_step(X, y)
    assert m._graph_safe_step()
    from deepctr_torch._hip.graph import GraphedTrainStep
    step = GraphedTrainStep(m, X, y).capture(X, y)
    loss = step(X, y)[0]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all())


@pytest.mark.parametrize("name", H.ALL)
def test_state_dict_keys_are_the_fixtures(name):
    g, m = H.loaded(name, DEV)
    sd = m.state_dict()
    assert list(sd) == list(g["params"])
    for k, v in g["params"].items():
        assert tuple(sd[k].shape) == v.shape, k


def test_same_seed_initial_weights_on_the_gpu_are_the_references():
    configs = H.init_configs()
    assert len(configs) == 9
    for spec, params in configs:
        sd = H.build_dien(spec, DEV, l2=1e-6).state_dict()
        assert list(sd) == list(params)
        for k, v in params.items():
            assert np.array_equal(sd[k].cpu().numpy(), v), k


@pytest.mark.parametrize("name", ["dien_gru_neg", "dien_aigru", "dien_agru_neg", "dien_augru", "dien_t50"])
def test_fused_route_equals_the_torch_op_route(counting, monkeypatch, name):
    """the same model, same input: the kernels against ``DCTR_GRU_SEQ=0``; logits within 1e-5, gradients within
    2e-5 x max|g| of the torch-op route's"""
    g, m = H.loaded(name, DEV)
    X, y = torch.from_numpy(g["X"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)

    def run():
        m.train()
        m.zero_grad()
        cap = {}
        h = m.out.register_forward_pre_hook(lambda mod, inp: cap.__setitem__("logit", inp[0].detach()))
        yp = m(X).squeeze(1)
        h.remove()
        (torch.nn.functional.binary_cross_entropy(yp, y, reduction="sum") + m.aux_loss).sum().backward()
        return cap["logit"].cpu().numpy(), dict((k, p.grad.cpu().numpy().copy()) for k, p in m.named_parameters())
    fused_logit, fused = run()
    assert counting.n.get("dctr_gru_seq_fwd") == 2 and counting.n.get("dctr_gru_seq_bwd") == 2
    counting.n.clear()
    monkeypatch.setenv("DCTR_GRU_SEQ", "0")
    plain_logit, plain = run()
    assert "dctr_gru_seq_fwd" not in counting.n and "dctr_gru_seq_bwd" not in counting.n
    assert max_abs(fused_logit, plain_logit) <= H.LOGIT_TOL
    for k in plain:
        scale = H.grad_scale(k, plain, g["spec"])
        assert max_abs(fused[k], plain[k]) <= H.GRAD_TOL * scale, k


def test_shape_outside_the_kernel_runs_the_torch_ops(counting):
    from deepctr_torch.inputs import SparseFeat, VarLenSparseFeat
    from deepctr_torch.models import DIEN
    torch.manual_seed(1)
    cols = [SparseFeat("item", 9, 68),
            VarLenSparseFeat(SparseFeat("hist_item", 9, 68, embedding_name="item"), 5, length_name="seq_length")]
    m = DIEN(cols, ["item"], gru_type="AUGRU", dnn_hidden_units=(8,), att_hidden_units=(8, 4), init_std=0.1, device=DEV)
    rng = np.random.RandomState(0)
    X = np.concatenate([rng.randint(0, 9, (7, 1)), rng.randint(1, 9, (7, 5)), rng.randint(0, 6, (7, 1))], axis=1)
    X = torch.from_numpy(X.astype(np.float32)).to(DEV)
    m.train()
    y = m(X)
    y.sum().backward()
    torch.cuda.synchronize()
    assert "dctr_gru_seq_fwd" not in counting.n and "dctr_gru_seq_bwd" not in counting.n
    assert tuple(y.shape) == (7, 1) and bool(torch.isfinite(y).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.interest_extractor.parameters())


@pytest.mark.parametrize("gru_type", ["AIGRU", "AUGRU", "AGRU", "GRU"])
def test_layer_takes_lengths_that_live_on_the_host(counting, gru_type):
    """the reference's own layer test passes ``torch.tensor([3, 4])``: the lengths follow the keys to their device"""
    from deepctr_torch.models.dien import InterestEvolving
    torch.manual_seed(0)
    layer = InterestEvolving(input_size=3, gru_type=gru_type, init_std=0.5).to(DEV)
    q = torch.tensor([[1, 1, 1], [0.1, 0.2, 0.3]], device=DEV)
    k = torch.tensor([[[0.1, 0.2, 0.3], [1, 2, 3], [0.4, 0.2, 1], [0.0, 0.0, 0.0]],
                      [[0.1, 0.2, 0.3], [1, 2, 3], [0.4, 0.2, 1], [0.5, 0.5, 0.5]]], device=DEV)
    with torch.no_grad():
        on_host = layer(q, k, torch.tensor([3, 4]))
        on_device = layer(q, k, torch.tensor([3, 4], device=DEV))
    torch.cuda.synchronize()
    assert counting.n.get("dctr_gru_seq_fwd") == 2
    assert tuple(on_host.shape) == (2, 3) and torch.equal(on_host, on_device) and bool(torch.isfinite(on_host).all())


@pytest.mark.parametrize("name", ["dien_gru_neg", "dien_augru_neg"])
def test_all_zero_lengths_give_zero_hist_and_zero_auxiliary_loss(counting, name):
    """the deliberate difference from the reference (which raises): states, evolved interest and auxiliary loss exactly 0"""
    from deepctr_torch.inputs import build_input_features
    from helpers import feature_columns
    g, m = H.loaded(name, DEV)
    fi = build_input_features(feature_columns(g["spec"]["dnn_columns"]))
    X = g["X"].copy()
    X[:, fi["seq_length"][0]] = 0
    seen = {}
    h = m.interest_evolution.register_forward_hook(
        lambda mod, inp, out: seen.update(hist=out.detach().clone(), states=inp[1].detach().clone()))
    m.train()
    y = m(torch.from_numpy(X).to(DEV))
    h.remove()
    (y.sum() + m.aux_loss.sum()).backward()
    torch.cuda.synchronize()
    assert counting.n.get("dctr_gru_seq_fwd") == 2 and counting.n.get("dctr_gru_seq_bwd") == 2
    assert tuple(seen["hist"].shape) == (X.shape[0], 12) and not seen["hist"].any() and not seen["states"].any()
    assert float(m.aux_loss.detach()) == 0.0 and bool(torch.isfinite(y).all())
    for p in m.interest_extractor.gru.parameters():
        assert not p.grad.any()
