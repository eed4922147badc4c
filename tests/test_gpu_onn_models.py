"""GPU: ONN against the golden vectors the real reference produced (tests/golden/onn, tools/golden/make_onn_golden.py),
every comparison against the reference alone, every element: pre-sigmoid logits and y_pred within 1e-5; every parameter
gradient within 2e-5 x max|g_ref| of that parameter -- WITHOUT the other suites' floor of 1 for the pair tables, whose
gradients are 5e-3 .. 0.2 in these fixtures (the fp32 reference is within 7e-7 x max|g| of its own fp64 run on these
shapes, so the bound leaves it a 30x margin); 3-step sgd / adagrad / preset-accumulator adagrad trajectories on the sparse
table update; the reference's default kind of training (L2 on the tables, Adam) on the exact lazy update; fit() Histories;
graph replay; checkpoints; same-seed initial weights; and the launch accounting of a train step."""
import io
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, build_model, feature_columns, load_golden, max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOGIT_TOL, GRAD_TOL, TRAJ_TOL = 1e-5, 2e-5, 2e-5
FORWARD = ["onn_two", "onn_d6", "onn_criteo", "onn_mixed", "onn_one_sparse", "onn_nolinear", "onn_bn", "lazy_onn", "fit_onn"]
STEPS = ["onn_two", "onn_criteo"]
FIT_RUNS = (("plain", "adagrad", 0.0, False), ("shuffled", "adagrad", 0.0, True), ("default", "adam", 1e-5, True))


def _loaded(name, l2=0.0):
    g = load_golden("onn/" + name)
    m = build_model(g["spec"], DEV, l2=l2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    return g, m


def grad_scale(key, ref):
    top = float(np.max(np.abs(ref))) if ref.size else 0.0
    return top if "second_order_embedding_dict" in key else max(1.0, top)


@pytest.mark.parametrize("name", FORWARD)
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


@pytest.mark.parametrize("name", FORWARD)
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
        scale = grad_scale(k, ref)
        err = max_abs(got, ref)
        if scale > 0:
            worst = max(worst, err / scale)
        assert err <= GRAD_TOL * scale, "%s: max|d|=%.3e scale %.3g" % (k, err, scale)
        if k.startswith("embedding_dict."):
            assert p.grad is None, "%s: the output never depends on embedding_dict" % k
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
    assert plan.pair and plan.update[0] != "dense", plan.update
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
    """The reference's eight steps with L2 on every table (and Adam without): the pair tables and the first-order tables on
    the exact lazy update, their row gradients coming out of the pair backward kernel."""
    g, m = _loaded("lazy_onn", l2=0.0 if tag == "adam0" else 1e-3)
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
    # (the fixture's optimizer state is that of embedding_dict's first table: a dense parameter of this model)
    p0 = m.embedding_dict[g["spec"]["dnn_columns"][0]["embedding_name"]].weight
    st = m.optim.state[p0]
    for key in ("sum", "exp_avg", "exp_avg_sq"):
        ref = ex.get("lazy_%s_state_%s" % (tag, key))
        if ref is not None:
            _close("state." + key, st[key].cpu().numpy(), ref)


@pytest.mark.parametrize("graphs", ["1", "0"])
@pytest.mark.parametrize("tag,opt,l2,shuffle", FIT_RUNS)
def test_fit_history_and_predict_match_reference(monkeypatch, tag, opt, l2, shuffle, graphs):
    monkeypatch.setenv("DCTR_FIT_GRAPH", graphs)
    g, m = _loaded("fit_onn", l2=l2)
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


def test_fit_replays_graphs(monkeypatch):
    """fit() replays a hipGraph of the autograd train step of this model: same parameters and History as without."""
    g = load_golden("onn/onn_criteo")
    names = []
    for c in g["spec"]["linear_columns"] + g["spec"]["dnn_columns"]:
        if c["name"] not in names:
            names.append(c["name"])
    n = (g["X"].shape[0] // 16) * 16
    X = np.concatenate([g["X"][:n]] * 3, axis=0)
    y = np.concatenate([g["y"][:n]] * 3, axis=0)
    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("DCTR_FIT_GRAPH", flag)
        m = build_model(g["spec"], DEV)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
        m.compile("adagrad", "binary_crossentropy", metrics=[])
        fi = m.feature_index
        x = {nm: X[:, fi[nm][0]] for nm in names}
        hist = m.fit(x, y, batch_size=16, epochs=2, verbose=0, shuffle=False)
        used = m._fit_graph is not None and m._fit_graph.get("graph") is not None
        runs.append(({k: v.clone() for k, v in m.state_dict().items()}, dict(hist.history), used))
    (a, ha, ua), (b, hb, ub) = runs
    assert ua and not ub
    for k in a:
        err = max_abs(a[k].cpu().numpy(), b[k].cpu().numpy())
        assert err <= 1e-6 * max(1.0, float(b[k].abs().max())), "%s: %.3e" % (k, err)
    np.testing.assert_allclose(ha["loss"], hb["loss"], rtol=1e-6)


@pytest.mark.parametrize("name", ["onn_mixed", "onn_criteo"])
def test_checkpoint_round_trip(name):
    g, m = _loaded(name)
    sd = m.state_dict()
    assert list(sd) == list(g["params"])
    for k, v in g["params"].items():
        assert tuple(sd[k].shape) == v.shape, k
    X = torch.from_numpy(g["X"]).to(DEV)
    m.eval()
    with torch.no_grad():
        before = m(X).cpu()
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    torch.manual_seed(5)
    m2 = build_model(g["spec"], DEV)
    m2.load_state_dict(torch.load(buf))
    m2.eval()
    with torch.no_grad():
        after = m2(X).cpu()
    assert torch.equal(before, after)


def test_same_seed_initial_weights_on_the_gpu_are_the_references():
    from deepctr_torch.models import ONN
    z = np.load(os.path.join(GOLDEN_DIR, "onn", "init.npz"), allow_pickle=False)
    configs = json.loads(str(z["configs"]))
    assert len(configs) == 2
    for i, spec in enumerate(configs):
        pre = "%d/param/" % i
        params = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        cols = feature_columns(spec["dnn_columns"])
        kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in spec["kwargs"].items()}
        sd = ONN(cols, cols, device=DEV, **kw).state_dict()
        assert list(sd) == list(params)
        for k, v in params.items():
            assert np.array_equal(sd[k].cpu().numpy(), v), k


class _Counting(object):
    """A proxy around the loaded library that counts the calls of every entry point."""

    def __init__(self, lib):
        self._lib, self.n = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dctr_"):
            return fn

        def counted(*a, **k):
            self.n[name] = self.n.get(name, 0) + 1
            return fn(*a, **k)
        return counted


@pytest.mark.parametrize("name", ["onn_criteo", "onn_mixed"])
@pytest.mark.parametrize("opt,l2", [("adagrad", 0.0), ("adam", 1e-5)])
def test_launch_accounting(monkeypatch, name, opt, l2):
    """Without a profiler: a train step is exactly one pair forward and one pair backward, and no dctr_embed_fwd at all (none
    over the pair tables, none for the first-order logit); no secondary plan is built on the way."""
    from deepctr_torch._hip import lib as L
    g, m = _loaded(name, l2=l2)
    m.compile(opt, "binary_crossentropy", metrics=[])
    m.train()
    X, y = torch.from_numpy(g["X"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    m._train_step(X, y)                      # (plans, slabs and optimizer state exist from here on)
    proxy = _Counting(L.lib())
    monkeypatch.setattr(L, "lib", lambda: proxy)
    m._train_step(X, y)
    torch.cuda.synchronize()
    assert proxy.n.get("dctr_pair_embed_fwd") == 1 and proxy.n.get("dctr_pair_embed_bwd") == 1, proxy.n
    assert "dctr_embed_fwd" not in proxy.n and "dctr_embed_bwd" not in proxy.n, proxy.n
    for d in (m.embedding_dict, m.linear_model.embedding_dict, m.second_order_embedding_dict):
        assert not d.__dict__.get("_dctr_plans"), "a secondary plan was built on the training path"
    m.eval()
    proxy.n.clear()
    with torch.no_grad():
        m(X)
    assert proxy.n.get("dctr_pair_embed_fwd") == 1 and "dctr_embed_fwd" not in proxy.n and \
        "dctr_pair_embed_bwd" not in proxy.n
