"""GPU: CCPM against the golden vectors the real reference produced (tests/golden/ccpm, tools/golden/make_ccpm_golden.py),
every comparison against the reference alone, every element: pre-sigmoid logits and y_pred within 1e-5; every parameter and
table gradient within 2e-5 x max|g_ref| of that parameter; 3-step sgd / adagrad / preset-accumulator adagrad trajectories on
the sparse table update; the four lazy runs; fit() Histories and predict() with and without graph replay; state_dict keys;
same-seed initial weights; the fused route of ConvLayer against its own torch-op route; a shape outside the kernel.

k-max pooling routes the gradient to the selected rows, so a fixture on which two candidates of a column are closer than
rounding would test luck.  Every fixture here was accepted by its generator only with ``min_topk_gap`` >= MIN_GAP over every
pooling call of its run, and MIN_GAP is at least 8 times the kernel's largest deviation from float64
(tests/test_gpu_ccpm_kernel.py prints it, DESIGN.md quotes it): no selection can differ from the reference's."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, build_model, feature_columns, load_golden, max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOGIT_TOL, GRAD_TOL, TRAJ_TOL = 1e-5, 2e-5, 2e-5
ALL = ["ccpm_two", "ccpm_three", "ccpm_criteo", "ccpm_f26", "ccpm_mixed", "ccpm_one_layer", "ccpm_three_layers",
       "ccpm_nolinear", "ccpm_bn", "lazy_ccpm", "fit_ccpm"]
STEPS = ["ccpm_two", "ccpm_criteo"]
FIT_RUNS = (("plain", "adagrad", 0.0, False), ("shuffled", "adagrad", 0.0, True), ("default", "adam", 1e-5, True))


def _loaded(name, l2=0.0):
    g = load_golden("ccpm/" + name)
    m = build_model(g["spec"], DEV, l2=l2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    return g, m


def grad_scale(key, grads, spec):
    """max|g_ref| of the parameter, no floor.  One exception, by reasoning and not by result: with ``dnn_use_bn`` a Linear
    bias sits directly in front of a BatchNorm in train mode, which subtracts the batch mean -- its exact gradient is 0 and
    the reference's own value (4.8e-7 in ccpm_bn) is the rounding noise of a sum that cancels; the terms of that sum are
    those of the same layer's weight gradient, so that gradient's scale is used."""
    if spec["kwargs"].get("dnn_use_bn") and key.startswith("dnn.linears.") and key.endswith(".bias"):
        key = key[:-len("bias")] + "weight"
    return float(np.max(np.abs(grads[key])))


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


@pytest.mark.parametrize("name", ALL)
def test_forward_logits_match_reference(name):
    g, m = _loaded(name)
    # (the fixtures hold the reference's train-mode forward: BatchNorm then normalises with the batch's statistics)
    m.train(bool(g["spec"]["kwargs"].get("dnn_use_bn")))
    cap = {}
    h = m.out.register_forward_pre_hook(lambda mod, inp: cap.__setitem__("logit", inp[0].detach()))
    with torch.no_grad():
        y = m(torch.from_numpy(g["X"]).to(DEV))
    h.remove()
    torch.cuda.synchronize()
    m.model_plan().check_ids()
    err = max_abs(cap["logit"].cpu().numpy(), g["logit"])
    print("%s: logit max|d| = %.3e" % (name, err))
    assert err <= LOGIT_TOL, "logit max|d|=%.3e" % err
    assert max_abs(y.cpu().numpy(), g["y_pred"]) <= LOGIT_TOL


@pytest.mark.parametrize("name", ALL)
def test_gradients_match_reference(name):
    g, m = _loaded(name)
    m.train()
    X, y = torch.from_numpy(g["X"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    loss = torch.nn.functional.binary_cross_entropy(m(X).squeeze(1), y, reduction="sum")
    m.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - g["loss"]) <= 1e-4 * max(1.0, abs(g["loss"]))
    assert set(g["grads"]) == set(k for k, _ in m.named_parameters())
    worst = 0.0
    for k, p in m.named_parameters():
        ref = g["grads"][k]
        got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        scale = grad_scale(k, g["grads"], g["spec"])
        err = max_abs(got, ref)
        if scale > 0:
            worst = max(worst, err / scale)
        assert err <= GRAD_TOL * scale, "%s: max|d|=%.3e scale %.3g" % (k, err, scale)
    print("%s: worst gradient error / scale = %.3e" % (name, worst))


@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adagradp"])
@pytest.mark.parametrize("name", STEPS)
def test_training_trajectory_matches_reference(name, opt):
    g, m = _loaded(name)
    m.compile("adagrad" if opt == "adagradp" else opt, "binary_crossentropy", metrics=[])
    if opt == "adagradp":
        for grp in m.optim.param_groups:
            for p in grp["params"]:
                m.optim.state[p]["sum"].fill_(0.05)
    m.train()
    plan = m.model_plan()
    assert plan.update[0] != "dense", plan.update
    losses = []
    for Xb, yb in zip(g["extra"]["X_steps"], g["extra"]["y_steps"]):
        loss, _, _ = m._train_step(torch.from_numpy(Xb).to(DEV), torch.from_numpy(yb).to(DEV))
        losses.append(loss.item())
    torch.cuda.synchronize()
    plan.check_ids()
    assert plan.update[0] != "dense", plan.update
    np.testing.assert_allclose(losses, g["extra"][opt + "3_loss"], rtol=2e-5)
    sd = m.state_dict()
    pre = opt + "3/"
    n = 0
    for k, v in g["extra"].items():
        if k.startswith(pre):
            err = max_abs(sd[k[len(pre):]].cpu().numpy(), v)
            assert err <= TRAJ_TOL, "%s: %.3e" % (k, err)
            n += 1
    assert n == len(sd)


def _close(tag, got, ref, tol=2e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(1.0, float(np.max(np.abs(ref))) if ref.size else 1.0)
    err = max_abs(got, ref)
    assert err <= tol * scale, "%s: max|d| = %.3e (scale %.3e)" % (tag, err, scale)


@pytest.mark.parametrize("tag", ["sgd", "adagrad", "adam", "adam0"])
def test_lazy_trajectory_matches_reference(tag):
    """The reference's eight steps with L2 on every table (and Adam without): the tables on the exact lazy update, their row
    gradients coming out of the conv backward kernel's gE; the conv parameters on the dense optimizer."""
    g, m = _loaded("lazy_ccpm", l2=0.0 if tag == "adam0" else 1e-3)
    ex = g["extra"]
    m.compile("adam" if tag == "adam0" else tag, "binary_crossentropy", metrics=[])
    m.train()
    plan = m.model_plan()
    assert plan.update == ("lazy", "adam" if tag == "adam0" else tag), plan.update
    bce, tot = [], []
    for Xb, yb in zip(ex["lazy_X"], ex["lazy_y"]):
        loss, total, _ = m._train_step(torch.from_numpy(Xb).to(DEV), torch.from_numpy(yb).to(DEV))
        bce.append(float(loss.item()))
        tot.append(float(total.item()))
    assert plan.update == ("lazy", "adam" if tag == "adam0" else tag), plan.update
    np.testing.assert_allclose(bce, ex["lazy_%s_bce" % tag], rtol=2e-5)
    np.testing.assert_allclose(tot, ex["lazy_%s_total" % tag], rtol=2e-5)
    sd = m.state_dict()
    pre = "lazy_%s/" % tag
    for k, v in ex.items():
        if k.startswith(pre):
            _close(k, sd[k[len(pre):]].cpu().numpy(), v)
    m.eval()
    with torch.no_grad():
        pred = m(torch.from_numpy(ex["lazy_X"][0]).to(DEV))
    _close("pred", pred.cpu().numpy().reshape(-1, 1), ex["lazy_%s_pred" % tag])


@pytest.mark.parametrize("graphs", ["1", "0"])
@pytest.mark.parametrize("tag,opt,l2,shuffle", FIT_RUNS)
def test_fit_history_and_predict_match_reference(monkeypatch, tag, opt, l2, shuffle, graphs):
    monkeypatch.setenv("DCTR_FIT_GRAPH", graphs)
    g, m = _loaded("fit_ccpm", l2=l2)
    ex = g["extra"]
    m.compile(opt, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    x = {c["name"]: ex["fit_X"][:, i] for i, c in enumerate(g["spec"]["dnn_columns"])}
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


@pytest.mark.parametrize("name", ALL)
def test_state_dict_keys_are_the_fixtures(name):
    g, m = _loaded(name)
    sd = m.state_dict()
    assert list(sd) == list(g["params"])
    for k, v in g["params"].items():
        assert tuple(sd[k].shape) == v.shape, k


def test_same_seed_initial_weights_on_the_gpu_are_the_references():
    from deepctr_torch.models import CCPM
    z = np.load(os.path.join(GOLDEN_DIR, "ccpm", "init.npz"), allow_pickle=False)
    configs = json.loads(str(z["configs"]))
    assert len(configs) == 2
    for i, spec in enumerate(configs):
        pre = "%d/param/" % i
        params = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        cols = feature_columns(spec["dnn_columns"])
        sd = CCPM(cols, cols, device=DEV, **spec["kwargs"]).state_dict()
        assert list(sd) == list(params)
        for k, v in params.items():
            assert np.array_equal(sd[k].cpu().numpy(), v), k


@pytest.mark.parametrize("name", ["ccpm_criteo", "ccpm_three_layers", "ccpm_f26"])
def test_fused_route_equals_the_torch_op_route(monkeypatch, name):
    """ConvLayer on the fixture's own embeddings (tie-free by construction of the fixture): the kernel against the layer's
    Sequential as PyTorch-ROCm ops, values within 1e-5, gradients within 2e-5 x max|g|."""
    from deepctr_torch._hip import lib as L
    g, m = _loaded(name)
    plan = m.model_plan()
    with torch.no_grad():
        gathered, _, _ = m.fused_inputs(torch.from_numpy(g["X"]).to(DEV))
    emb = gathered[:, :plan.emb_width].reshape(-1, 1, len(plan.deep), plan.emb_dim).clone().requires_grad_(True)
    layer = m.conv_layer
    proxy = _Counting(L.lib())
    monkeypatch.setattr(L, "lib", lambda: proxy)
    fused = layer(emb)
    assert proxy.n.get("dctr_ccpm_fwd") == 1
    plain = layer.conv_layer(emb)
    assert fused.shape == plain.shape
    assert max_abs(fused.detach().cpu().numpy(), plain.detach().cpu().numpy()) <= 1e-5
    go = torch.randn_like(plain)
    a = torch.autograd.grad(fused, [emb] + list(layer.parameters()), go)
    b = torch.autograd.grad(plain, [emb] + list(layer.parameters()), go)
    assert proxy.n.get("dctr_ccpm_bwd") == 1
    for x, y in zip(a, b):
        assert x.shape == y.shape
        assert max_abs(x.cpu().numpy(), y.cpu().numpy()) <= GRAD_TOL * float(y.abs().max())


def test_shape_outside_the_kernel_runs_the_fallback(monkeypatch):
    from deepctr_torch._hip import lib as L
    from deepctr_torch.inputs import SparseFeat
    from deepctr_torch.models import CCPM
    torch.manual_seed(1)
    cols = [SparseFeat("s%d" % i, 5 + i % 3, 4) for i in range(70)]
    m = CCPM(cols, cols, dnn_hidden_units=(8,), init_std=0.1, device=DEV)
    assert not m.conv_layer._kernel_fits(70, 4, *m.conv_layer._spec())
    X = torch.from_numpy(np.random.RandomState(0).randint(0, 5, (9, 70)).astype(np.float32)).to(DEV)
    proxy = _Counting(L.lib())
    monkeypatch.setattr(L, "lib", lambda: proxy)
    m.train()
    y = m(X)
    y.sum().backward()
    torch.cuda.synchronize()
    assert "dctr_ccpm_fwd" not in proxy.n and "dctr_ccpm_bwd" not in proxy.n
    assert tuple(y.shape) == (9, 1) and bool(torch.isfinite(y).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.conv_layer.parameters())
    # the same stack, straight from the modules
    with torch.no_grad():
        gathered, logit, _ = m.fused_inputs(X)
        pooled = m.conv_layer.conv_layer(gathered[:, :280].reshape(9, 1, 70, 4))
        ref = torch.sigmoid(logit + m.dnn_linear(m.dnn(pooled.reshape(9, -1))) + m.out.bias)
    assert max_abs(y.detach().cpu().numpy(), ref.cpu().numpy()) <= 1e-5


@pytest.mark.parametrize("opt,l2", [("adagrad", 0.0), ("adam", 1e-5)])
def test_launch_accounting(monkeypatch, opt, l2):
    """A train step is one conv forward (with a selection buffer) and one conv backward; predict passes no buffer."""
    from deepctr_torch._hip import lib as L
    g, m = _loaded("ccpm_criteo", l2=l2)
    m.compile(opt, "binary_crossentropy", metrics=[])
    m.train()
    X, y = torch.from_numpy(g["X"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    m._train_step(X, y)
    proxy = _Counting(L.lib())
    monkeypatch.setattr(L, "lib", lambda: proxy)
    m._train_step(X, y)
    torch.cuda.synchronize()
    assert proxy.n.get("dctr_ccpm_fwd") == 1 and proxy.n.get("dctr_ccpm_bwd") == 1, proxy.n
    assert proxy.args["dctr_ccpm_fwd"][12] is not None
    m.eval()
    proxy.n.clear()
    with torch.no_grad():
        m(X)
    assert proxy.n.get("dctr_ccpm_fwd") == 1 and "dctr_ccpm_bwd" not in proxy.n
    assert proxy.args["dctr_ccpm_fwd"][12] is None
