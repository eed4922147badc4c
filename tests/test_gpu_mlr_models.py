"""GPU: MLR on the device against the reference's golden values (tests/golden/mlr, tools/golden/make_mlr_golden.py): y
within 1e-5, every parameter gradient within 2e-5 x max|g_ref| (no floor of 1 for the region and bias sides), the 3-step
trajectories, the 8-step runs of the lazy fixture, the fit() History with and without hipGraph replays -- and the reference's
own test matrix (tests/models/MLR_test.py: nine (region, base, bias) column configurations plus test_MLR), run as there:
compile adam, fit with a validation split, predict, save / load ``state_dict`` and the model.  The columns and the data are
built here (the reference's generator draws vocabularies and lengths at random; fixed ones of the same kind stand in)."""
import io

import numpy as np
import pytest
import torch

from helpers import max_abs
from mlr_helpers import (FIT_RUNS, FORWARD, GRAD_TOL, STEPS, TRAJ_TOL, Y_TOL, build, fit_inputs, grad_scale, load, loaded,
                         loss_name, loss_sum)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize("name", FORWARD)
def test_forward_and_gradients_match_reference(name):
    g, m = loaded(name, DEV)
    m.train()
    y = m(_dev(g["X"]))
    loss = loss_sum(g["spec"], y.squeeze(1), _dev(g["y"]))
    m.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    m.model_plan().check_ids()
    err = max_abs(y.detach().cpu().numpy(), g["y_pred"])
    print("%s: y max|d| = %.3e" % (name, err))
    assert err <= Y_TOL
    assert abs(loss.item() - g["loss"]) <= 1e-4 * max(1.0, abs(g["loss"]))
    assert set(g["grads"]) == set(k for k, _ in m.named_parameters())
    worst = 0.0
    for k, p in m.named_parameters():
        ref = g["grads"][k]
        got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        scale = grad_scale(k, ref)
        e = max_abs(got, ref)
        if scale > 0:
            worst = max(worst, e / scale)
        assert e <= GRAD_TOL * scale, "%s: max|d|=%.3e scale %.3g" % (k, e, scale)
        if k.startswith(("base_linear_model.", "embedding_dict.", "linear_model.")):
            assert p.grad is None or not p.grad.any(), "%s: the output never depends on it" % k
    print("%s: worst gradient error / scale = %.3e" % (name, worst))


@pytest.mark.parametrize("name", ["mlr_bias", "mlr_mixed", "mlr_dense_only", "mlr_regression"])
def test_composed_route_equals_fused(monkeypatch, name):
    """DCTR_MLR=0 (one per-field gather + torch ops) against the fused kernels: y and every gradient within the bars."""
    out = []
    for route in ("1", "0"):
        monkeypatch.setenv("DCTR_MLR", route)
        g, m = loaded(name, DEV)
        m.train()
        y = m(_dev(g["X"]))
        m.zero_grad()
        loss_sum(g["spec"], y.squeeze(1), _dev(g["y"])).backward()
        torch.cuda.synchronize()
        assert max_abs(y.detach().cpu().numpy(), g["y_pred"]) <= Y_TOL
        out.append((y.detach().cpu().numpy(), {k: (p.grad.cpu().numpy() if p.grad is not None else None)
                                               for k, p in m.named_parameters()}))
    (ya, ga), (yb, gb) = out
    assert max_abs(ya, yb) <= Y_TOL
    for k, ref in g["grads"].items():
        a = ga[k] if ga[k] is not None else np.zeros_like(ref)
        b = gb[k] if gb[k] is not None else np.zeros_like(ref)
        assert max_abs(a, b) <= GRAD_TOL * grad_scale(k, ref), k


@pytest.mark.parametrize("name", STEPS)
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adagradp"])
def test_in_kernel_optimizer_trajectory(name, opt):
    g, m = loaded(name, DEV)
    start = {k: v.clone() for k, v in m.state_dict().items()}
    m.compile("adagrad" if opt == "adagradp" else opt, loss_name(g["spec"]), metrics=[])
    if opt == "adagradp":
        for grp in m.optim.param_groups:
            for p in grp["params"]:
                m.optim.state[p]["sum"].fill_(0.05)
    m.train()
    losses = [float(m._train_step(_dev(Xb), _dev(yb))[0]) for Xb, yb in zip(g["extra"]["X_steps"], g["extra"]["y_steps"])]
    torch.cuda.synchronize()
    m.model_plan().check_ids()
    assert m.model_plan().update[0] == ("sgd" if opt == "sgd" else "adagrad")
    np.testing.assert_allclose(losses, g["extra"][opt + "3_loss"], rtol=2e-5)
    sd = m.state_dict()
    worst = 0.0
    for k, v in g["extra"].items():
        if k.startswith(opt + "3/"):
            key = k[len(opt) + 2:]
            e = max_abs(sd[key].cpu().numpy(), v)
            worst = max(worst, e)
            assert e <= TRAJ_TOL, "%s: %.3e" % (k, e)
            if key.startswith("base_linear_model."):
                assert torch.equal(sd[key], start[key]), "%s moved" % key
    print("%s/%s: worst parameter error = %.3e" % (name, opt, worst))


@pytest.mark.parametrize("tag,opt,mode", [("sgd", "sgd", ("sgd",)), ("adagrad", "adagrad", ("adagrad",)),
                                          ("adam", "adam", ("lazy", "adam")), ("adam0", "adam", ("lazy", "adam"))])
def test_lazy_fixture_runs_replay_reference(tag, opt, mode):
    g, m = loaded("lazy_mlr", DEV, l2_reg_linear=0.0 if tag == "adam0" else 1e-3)
    ex = g["extra"]
    m.compile(opt, "binary_crossentropy", metrics=[])
    m.train()
    assert m.model_plan().update[:len(mode)] == mode
    bce, tot = [], []
    for Xb, yb in zip(ex["lazy_X"], ex["lazy_y"]):
        loss, total, _ = m._train_step(_dev(Xb), _dev(yb))
        bce.append(float(loss))
        tot.append(float(total))
    np.testing.assert_allclose(bce, ex["lazy_%s_bce" % tag], rtol=2e-5)
    np.testing.assert_allclose(tot, ex["lazy_%s_total" % tag], rtol=2e-5)
    sd = m.state_dict()
    pre = "lazy_%s/" % tag
    for k, v in ex.items():
        if k.startswith(pre):
            ref = np.asarray(v, np.float64)
            e = max_abs(sd[k[len(pre):]].cpu().numpy(), ref)
            assert e <= TRAJ_TOL * max(1.0, float(np.max(np.abs(ref)))), "%s: %.3e" % (k, e)
    m.eval()
    with torch.no_grad():
        assert max_abs(m(_dev(ex["lazy_X"][0])).cpu().numpy(), ex["lazy_%s_pred" % tag]) <= 5e-5


@pytest.mark.parametrize("graphs", ["1", "0"])
@pytest.mark.parametrize("tag,opt,l2,shuffle", FIT_RUNS)
def test_fit_history_and_predict_match_reference(monkeypatch, tag, opt, l2, shuffle, graphs):
    monkeypatch.setenv("DCTR_FIT_GRAPH", graphs)
    g, m = loaded("fit_mlr", DEV, l2_reg_linear=l2)
    ex = g["extra"]
    base0 = [p.detach().clone() for p in m.base_linear_model.parameters()]
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
    for p, q in zip(m.base_linear_model.parameters(), base0):
        assert torch.equal(p.detach(), q), "base_linear_model moved under fit()"


def test_fit_replays_graphs():
    """fit() replays a hipGraph of the autograd train step of this model: same parameters and History as without."""
    import os
    g = load("mlr_criteo")
    rng = np.random.RandomState(3)
    X = np.concatenate([g["X"]] + list(g["extra"]["X_steps"]))[:144]
    y = rng.randint(0, 2, len(X)).astype(np.float32)
    runs = []
    for graphs in ("1", "0"):
        os.environ["DCTR_FIT_GRAPH"] = graphs
        try:
            _, m = loaded("mlr_criteo", DEV)
            m.compile("adagrad", "binary_crossentropy", metrics=[])
            hist = m.fit(fit_inputs(m, X), y, batch_size=16, epochs=2, verbose=0, shuffle=False)
        finally:
            os.environ.pop("DCTR_FIT_GRAPH", None)
        used = m._fit_graph is not None and m._fit_graph.get("graph") is not None
        runs.append(({k: v.clone() for k, v in m.state_dict().items()}, dict(hist.history), used))
    (a, ha, ua), (b, hb, ub) = runs
    assert ua and not ub
    for k in a:
        e = max_abs(a[k].cpu().numpy(), b[k].cpu().numpy())
        assert e <= TRAJ_TOL * max(1.0, float(b[k].abs().max())), "%s: %.3e" % (k, e)
    np.testing.assert_allclose(ha["loss"], hb["loss"], rtol=2e-5)


def test_predict_on_a_never_compiled_model():
    g, m = loaded("mlr_mixed", DEV)
    pred = m.predict(fit_inputs(m, g["X"]), batch_size=7)
    assert pred.shape == g["y_pred"].shape and max_abs(pred, g["y_pred"]) <= Y_TOL


# ---- the reference's own test matrix (tests/models/MLR_test.py) ----------------------------------------------------------
SAMPLE_SIZE = 64


def _test_data(rng, n_sparse, n_dense, prefix):
    from deepctr_torch.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    cols = [SparseFeat("%ssparse_feature_%d" % (prefix, i), 3 + 2 * i, 4) for i in range(n_sparse)] + \
        [DenseFeat("%sdense_feature_%d" % (prefix, i), 1) for i in range(n_dense)] + \
        [VarLenSparseFeat(SparseFeat(prefix + "sequence_" + mode, vocab, 4), maxlen, mode)
         for mode, vocab, maxlen in (("sum", 5, 4), ("mean", 7, 6), ("max", 4, 3))]
    x = {}
    for c in cols:
        if isinstance(c, DenseFeat):
            x[c.name] = rng.random_sample(SAMPLE_SIZE)
        elif isinstance(c, SparseFeat):
            x[c.name] = rng.randint(0, c.vocabulary_size, SAMPLE_SIZE)
        else:
            lens = rng.randint(1, c.maxlen + 1, SAMPLE_SIZE)
            ids = rng.randint(1, c.vocabulary_size, (SAMPLE_SIZE, c.maxlen)) if c.vocabulary_size > 1 else \
                np.zeros((SAMPLE_SIZE, c.maxlen), np.int64)
            ids[np.arange(c.maxlen)[None, :] >= lens[:, None]] = 0
            x[c.name] = ids
    return x, cols


def _check_model(m, x, y):
    """tests/utils.py check_model: compile, train with a validation split, save / load weights and model"""
    from deepctr_torch.models import MLR
    m.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy", "acc"])
    hist = m.fit(x, y, batch_size=16, epochs=2, verbose=0, validation_split=0.5)
    assert len(hist.history["loss"]) == 2 and np.all(np.isfinite(hist.history["loss"]))
    assert np.all(np.isfinite(hist.history["val_binary_crossentropy"]))
    pred = m.predict(x, batch_size=32)
    assert pred.shape == (SAMPLE_SIZE, 1) and np.all(np.isfinite(pred)) and pred.min() >= 0 and pred.max() <= 1
    buf = io.BytesIO()
    torch.save(m.state_dict(), buf)
    buf.seek(0)
    m.load_state_dict(torch.load(buf))
    assert max_abs(m.predict(x, batch_size=32), pred) == 0
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    m2 = torch.load(buf, weights_only=False)
    assert isinstance(m2, MLR) and max_abs(m2.predict(x, batch_size=32), pred) == 0


@pytest.mark.parametrize("region_sparse,region_dense,base_sparse,base_dense,bias_sparse,bias_dense",
                         [(0, 2, 0, 2, 0, 1), (0, 2, 0, 1, 0, 2), (0, 2, 0, 0, 1, 0),
                          (0, 1, 1, 2, 1, 1), (0, 1, 1, 1, 1, 2), (0, 1, 1, 0, 2, 0),
                          (1, 0, 2, 2, 2, 1), (2, 0, 2, 1, 2, 2), (2, 0, 2, 0, 0, 0)])
def test_reference_matrix(region_sparse, region_dense, base_sparse, base_dense, bias_sparse, bias_dense):
    from deepctr_torch.models import MLR
    rng = np.random.RandomState(11)
    x, y = {}, rng.randint(0, 2, SAMPLE_SIZE).astype(np.float32)
    cols = {}
    for prefix, ns, nd in (("region", region_sparse, region_dense), ("base", base_sparse, base_dense),
                           ("bias", bias_sparse, bias_dense)):
        xi, cols[prefix] = _test_data(rng, ns, nd, prefix)
        x.update(xi)
    m = MLR(cols["region"], cols["base"], bias_feature_columns=cols["bias"], device=DEV)
    _check_model(m, x, y)


def test_reference_test_mlr():
    from deepctr_torch.models import MLR
    rng = np.random.RandomState(12)
    x, cols = _test_data(rng, 3, 3, "region")
    y = rng.randint(0, 2, SAMPLE_SIZE).astype(np.float32)
    _check_model(MLR(cols, device=DEV), x, y)
