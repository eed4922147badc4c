"""GPU: SharedBottom, ESMM, MMOE and PLE on the real library against the reference's golden values (tests/golden/mtl,
tools/golden/make_mtl_golden.py): per-task logits within 1e-5, every parameter gradient within 2e-5 x max|g_ref| (no floor),
the 3-step trajectories, the Adam runs on the lazy table update, ``fit()`` History and ``predict()`` with and without graph
replay; the fused gate mix against the torch-op route (``DCTR_GATE_MIX=0``); and every configuration of the reference's own
multi-task tests through ``compile('adam', losses, ...)``, ``fit`` and save / load, with the metrics the generator found
the reference to accept on such labels."""
import json

import numpy as np
import pytest
import torch

from helpers import load_golden, max_abs
import mtl_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIT_RUNS = (("plain", "adagrad", 0.0, False), ("shuffled", "adagrad", 0.0, True), ("default", "adam", 1e-5, True))
CONFIGS, METRICS = H.init_configs()


class _Counting(object):
    """the loaded library with its calls counted"""

    def __init__(self, inner):
        self.inner, self.n = inner, {}

    def __getattr__(self, name):
        fn = getattr(self.inner, name)

        def call(*a):
            self.n[name] = self.n.get(name, 0) + 1
            return fn(*a)
        return call


def n_gate_launches(spec):
    kw = spec["kwargs"]
    return {"MMOE": 1, "PLE": kw.get("num_levels", 2)}.get(spec["model"], 0)


@pytest.mark.parametrize("name", H.ALL)
def test_logits_match_reference(monkeypatch, name):
    from deepctr_torch._hip import lib as L
    g, m = H.loaded(name, DEV)
    m.train()           # (the fixtures hold the train-mode forward: BatchNorm on the batch's statistics)
    proxy = _Counting(L.lib())
    monkeypatch.setattr(L, "lib", lambda: proxy)
    with torch.no_grad():
        logits, y = H.forward_logits(m, torch.from_numpy(g["X"]).to(DEV))
    torch.cuda.synchronize()
    m.model_plan().check_ids()
    assert tuple(y.shape) == g["y_pred"].shape
    err = max_abs(logits.cpu().numpy(), g["logit"])
    print("%s: max|logit - ref| = %.3e" % (name, err))
    assert err <= H.LOGIT_TOL
    assert max_abs(y.cpu().numpy(), g["y_pred"]) <= H.LOGIT_TOL
    assert proxy.n.get("dctr_gate_mix_fwd", 0) == n_gate_launches(g["spec"])


@pytest.mark.parametrize("name", H.ALL)
def test_gradients_match_reference(monkeypatch, name):
    from deepctr_torch._hip import lib as L
    g, m = H.loaded(name, DEV)
    proxy = _Counting(L.lib())
    monkeypatch.setattr(L, "lib", lambda: proxy)
    worst = H.check_gradients(g, m, DEV)
    torch.cuda.synchronize()
    print("%s: worst gradient error / bound = %.3f" % (name, worst))
    assert proxy.n.get("dctr_gate_mix_fwd", 0) == proxy.n.get("dctr_gate_mix_bwd", 0) == n_gate_launches(g["spec"])


@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adagradp"])
@pytest.mark.parametrize("name", H.STEPS)
def test_training_trajectory_matches_reference(name, opt):
    g, m = H.loaded(name, DEV)
    H.check_trajectory(g, m, DEV, opt)
    torch.cuda.synchronize()
    m.model_plan().check_ids()
    assert m.model_plan().update[0] != "dense"


@pytest.mark.parametrize("tag,l2", [("adam", None), ("adam0", 0.0)])
def test_lazy_adam_matches_reference(tag, l2):
    m = H.check_lazy(load_golden("mtl/lazy_mtl"), DEV, tag, l2)
    assert m.model_plan().update == ("lazy", "adam")


def _fit(g, tag, opt, l2, shuffle):
    ex = g["extra"]
    m = H.build(g["spec"], DEV, l2=l2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    m.compile(opt, g["spec"]["losses"], metrics=json.loads(str(ex["fit_metrics"])))
    x = H.feature_dict(g["spec"], ex["fit_X"])
    torch.manual_seed(777)
    hist = m.fit(x, ex["fit_y"], batch_size=64, epochs=3, verbose=2, validation_split=0.25, shuffle=shuffle)
    return m, x, hist


@pytest.mark.parametrize("graphs", ["1", "0"])
@pytest.mark.parametrize("tag,opt,l2,shuffle", FIT_RUNS)
def test_fit_history_and_predict_match_reference(monkeypatch, tag, opt, l2, shuffle, graphs):
    monkeypatch.setenv("DCTR_FIT_GRAPH", graphs)
    g = load_golden("mtl/fit_mtl")
    ex = g["extra"]
    m, x, hist = _fit(g, tag, opt, l2, shuffle)
    ref = {k[len("fit_%s_hist/" % tag):]: v for k, v in ex.items() if k.startswith("fit_%s_hist/" % tag)}
    assert set(hist.history) == set(ref) and len(ref) > 2
    for k, v in ref.items():
        if k.endswith("auc") or k.endswith("acc"):       # (step functions of the predictions)
            np.testing.assert_allclose(hist.history[k], v, atol=5e-3, err_msg=k)
        else:
            np.testing.assert_allclose(hist.history[k], v, rtol=2e-4, err_msg=k)
    pred = m.predict(x, batch_size=50)
    assert pred.dtype == np.float64 and pred.shape == ex["fit_%s_pred" % tag].shape == (300, 2)
    assert max_abs(pred, ex["fit_%s_pred" % tag]) <= 5e-5


def test_fit_with_and_without_graph_replay_agree(monkeypatch):
    g = load_golden("mtl/fit_mtl")
    out = []
    for graphs in ("1", "0"):
        monkeypatch.setenv("DCTR_FIT_GRAPH", graphs)
        m, x, hist = _fit(g, "shuffled", "adagrad", 0.0, True)
        out.append((hist.history["loss"], m.predict(x, batch_size=50)))
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-5)
    assert max_abs(out[0][1], out[1][1]) <= 1e-5


@pytest.mark.parametrize("name", ["mmoe", "mmoe_nogate", "mmoe_three", "ple_222", "ple_333_nogate", "ple_noshared"])
def test_fused_route_equals_the_torch_op_route(monkeypatch, name):
    from deepctr_torch._hip import lib as L
    g = load_golden("mtl/" + name)
    res = []
    for switch in ("1", "0"):
        monkeypatch.setenv("DCTR_GATE_MIX", switch)
        m = H.build(g["spec"], DEV)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
        m.train()
        proxy = _Counting(L.lib())
        monkeypatch.setattr(L, "lib", lambda proxy=proxy: proxy)
        y = m(torch.from_numpy(g["X"]).to(DEV))
        loss = H.list_loss(g["spec"], y, torch.from_numpy(g["y"]).to(DEV))
        m.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        assert proxy.n.get("dctr_gate_mix_fwd", 0) == (n_gate_launches(g["spec"]) if switch == "1" else 0)
        res.append((y.detach().cpu().numpy(), {k: (None if p.grad is None else p.grad.cpu().numpy())
                                               for k, p in m.named_parameters()}))
    assert max_abs(res[0][0], res[1][0]) <= 1e-5
    for k, a in res[0][1].items():
        b = res[1][1][k]
        assert (a is None) == (b is None), k
        if a is not None:
            assert max_abs(a, b) <= H.GRAD_TOL * float(np.max(np.abs(b))), k


@pytest.mark.parametrize("c", CONFIGS, ids=H.config_id)
def test_reference_test_matrix_trains_saves_and_loads(c, tmp_path):
    """The reference's check_mtl_model on every configuration of its four multi-task tests: same-seed weights, compile with
    adam and one loss per task (mae for a regression task, as there), fit with a validation split, weights and whole model
    through torch.save / torch.load."""
    spec, params = c
    types = spec["kwargs"]["task_types"]
    m = H.build(spec, DEV, l2=None)
    sd = m.state_dict()
    assert list(sd) == list(params)
    for k, v in params.items():
        assert np.array_equal(sd[k].cpu().numpy(), v), k
    rng = np.random.default_rng(5)
    n = 64
    x = {}
    for col in spec["dnn_columns"]:
        if col["kind"] == "sparse":
            x[col["name"]] = rng.integers(0, col["vocab"], n)
        elif col["kind"] == "dense":
            x[col["name"]] = rng.random(n)
        else:
            x[col["name"]] = rng.integers(1, col["vocab"], (n, col["maxlen"]))
    y = np.stack([rng.integers(0, 2, n) if t == "binary" else rng.random(n) for t in types], axis=1)
    metrics = METRICS[",".join(types)]
    assert metrics
    m.compile("adam", ["binary_crossentropy" if t == "binary" else "mae" for t in types], metrics=metrics)
    hist = m.fit(x, y, batch_size=100, epochs=1, verbose=2, validation_split=0.5)
    assert np.isfinite(hist.history["loss"]).all() and all("val_" + k in hist.history for k in metrics)
    path = str(tmp_path / "weights.h5")
    torch.save(m.state_dict(), path)
    m.load_state_dict(torch.load(path))
    before = m.predict(x, batch_size=64)
    assert before.shape == (n, len(types)) and np.isfinite(before).all()
    path = str(tmp_path / "model.h5")
    torch.save(m, path)
    again = torch.load(path, weights_only=False)
    assert max_abs(again.predict(x, batch_size=64), before) == 0.0


def test_batch_of_one_and_outside_the_envelope():
    from deepctr_torch.inputs import SparseFeat
    from deepctr_torch.models import MMOE
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4)]
    torch.manual_seed(0)
    m = MMOE(cols, num_experts=17, expert_dnn_hidden_units=(8,), gate_dnn_hidden_units=(), tower_dnn_hidden_units=(4,),
             init_std=0.2, device=DEV)          # 17 members per gate: the torch-op route
    X = torch.tensor([[1., 2.], [3., 4.], [0., 5.]], device=DEV)
    m.eval()
    with torch.no_grad():
        y3, y1 = m(X), m(X[:1])
    assert tuple(y3.shape) == (3, 2) and tuple(y1.shape) == (1, 2)
    assert max_abs(y1.cpu().numpy(), y3[:1].cpu().numpy()) <= 1e-6
