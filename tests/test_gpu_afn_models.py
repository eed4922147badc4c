"""GPU: AFN against the reference's values (tests/golden/afn, tools/golden/make_afn_golden.py).

Logits and ``y_pred``: within the project's 1e-5 of the float32 reference, train mode, every fixture.  Gradients and 3-step
trajectories: against the reference's FLOAT64 run, per parameter within max(2e-5, 4 x the float32 reference's own deviation
from it) -- tests/afn_helpers.py has the rule and its reasons, ``scale_key`` the parameters whose exact gradient is zero.
``fit()``: whole History and ``predict`` for SGD and for Adagrad with preset accumulators, with and without graph replay,
at the tolerances tests/test_gpu_ccpm_models.py uses for ``fit_ccpm``.

The reference's DEFAULT run (adam, L2 1e-5, shuffled) is compared on the train-side History keys only.  ``val_*`` are
deliberately not compared: Adam turns the sign of the rounding noise that is the whole gradient of every
``afn_dnn.linears.<i>.bias`` and of ``ltl.bn.1.bias`` into steps of +-lr.  Train-mode BatchNorm cancels those parameters
exactly, so the training losses are reproducible; eval-mode BatchNorm does not, so the validation metrics of the reference
are those of its own noise and no other implementation can reproduce them."""
import numpy as np
import pytest
import torch

from afn_helpers import ALL, LOGIT_TOL, STEPS, check_gradients, check_trajectory, loaded, run_steps
from helpers import max_abs
from test_gpu_ccpm_models import _Counting

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIT_RUNS = (("sgd", "sgd", 0.0, False), ("adagradp", "adagrad", 0.0, True), ("default", "adam", 1e-5, True))


@pytest.mark.parametrize("name", ALL)
def test_forward_logits_match_reference(name):
    g, m = loaded(name, DEV)
    m.train()
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


def _gradients(g, m):
    m.train()
    X, y = torch.from_numpy(g["X"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    loss = torch.nn.functional.binary_cross_entropy(m(X).squeeze(1), y, reduction="sum")
    m.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - g["loss"]) <= 1e-4 * max(1.0, abs(g["loss"]))
    return {k: (p.grad.cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
            for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", ALL)
def test_gradients_match_float64_reference(name):
    g, m = loaded(name, DEV)
    worst = check_gradients(g, _gradients(g, m), name)
    print("%s: worst gradient error / bound = %.3f" % (name, worst))


@pytest.mark.parametrize("opt", ["sgd", "adagradp"])
@pytest.mark.parametrize("name", STEPS)
def test_training_trajectory_matches_float64_reference(name, opt):
    g, m = loaded(name, DEV)
    losses = run_steps(g, m, opt, DEV)
    torch.cuda.synchronize()
    plan = m.model_plan()
    plan.check_ids()
    assert plan.update[0] != "dense", plan.update
    np.testing.assert_allclose(losses, g["extra"]["ref64/%s3_loss" % opt], rtol=2e-5)
    worst = check_trajectory(g, opt, m.state_dict(), name)
    print("%s %s: worst trajectory error / bound = %.3f" % (name, opt, worst))


@pytest.mark.parametrize("name", STEPS)
def test_adagrad_from_zero_losses(name):
    """the three losses only: the zero-gradient parameters move by +-lr on the sign of rounding noise (module docstring)"""
    g, m = loaded(name, DEV)
    np.testing.assert_allclose(run_steps(g, m, "adagrad", DEV), g["extra"]["adagrad3_loss"], rtol=2e-5)
    assert m.model_plan().update[0] != "dense"


@pytest.mark.parametrize("graphs", ["1", "0"])
@pytest.mark.parametrize("tag,opt,l2,shuffle", FIT_RUNS)
def test_fit_history_and_predict_match_reference(monkeypatch, tag, opt, l2, shuffle, graphs):
    """Like the reference, ``fit()`` goes on training in EVAL mode after the first validation pass, so the second epoch
    normalises with the running statistics: a train step captured in the first epoch must not be replayed in the second
    (``BaseModel._graph_mode``) -- replaying it gave ``loss`` 0.704164 against the reference's 0.701944 here."""
    monkeypatch.setenv("DCTR_FIT_GRAPH", graphs)
    g, m = loaded("fit_afn", DEV, l2=l2)
    ex = g["extra"]
    m.compile(opt, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    if tag == "adagradp":
        for grp in m.optim.param_groups:
            for p in grp["params"]:
                m.optim.state[p]["sum"].fill_(0.05)
    x = {c["name"]: ex["fit_X"][:, i] for i, c in enumerate(g["spec"]["dnn_columns"])}
    torch.manual_seed(777)
    hist = m.fit(x, ex["fit_y"], batch_size=64, epochs=2, verbose=0, validation_split=0.25, shuffle=shuffle)
    assert m.model_plan().update[0] != "dense", m.model_plan().update
    ref = {k[len("fit_%s_hist/" % tag):]: v for k, v in ex.items() if k.startswith("fit_%s_hist/" % tag)}
    assert set(hist.history) == set(ref)
    for k, v in ref.items():
        if tag == "default" and k.startswith("val_"):
            continue                                   # (module docstring)
        if k.endswith("auc"):
            np.testing.assert_allclose(hist.history[k], v, atol=5e-3, err_msg=k)
        else:
            np.testing.assert_allclose(hist.history[k], v, rtol=2e-4, err_msg=k)
    if tag != "default":
        pred = m.predict(x, batch_size=50)
        assert pred.dtype == np.float64 and pred.shape == ex["fit_%s_pred" % tag].shape
        assert max_abs(pred, ex["fit_%s_pred" % tag]) <= 5e-5


# ---- routes --------------------------------------------------------------------------------------------------------
def test_fused_route_against_torch_route_on_the_gpu(monkeypatch):
    """the same model and batch both ways on the GPU; each gradient within the kernel test's rule, with the torch route's
    own distance from float64 taken from the fixture (the float32 reference is that op sequence)"""
    g, m = loaded("afn_criteo", DEV)
    fused = _gradients(g, m)
    monkeypatch.setenv("DCTR_LOG_TRANSFORM", "0")
    g2, m2 = loaded("afn_criteo", DEV)
    plain = _gradients(g2, m2)
    check_gradients(g, fused, "fused")
    check_gradients(g, plain, "torch route")


def test_the_new_entry_points_are_the_ones_called(monkeypatch):
    from deepctr_torch._hip import lib as L
    g, m = loaded("afn_two", DEV)
    X, y = torch.from_numpy(g["X"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    m.compile("adagrad", "binary_crossentropy", metrics=[])
    m.train()
    m._train_step(X, y)
    proxy = _Counting(L.lib())
    monkeypatch.setattr(L, "lib", lambda: proxy)
    m._train_step(X, y)
    torch.cuda.synchronize()
    assert proxy.n.get("dctr_log_transform_fwd_train") == 1 and proxy.n.get("dctr_log_transform_bwd") == 1
    assert "dctr_log_transform_fwd_eval" not in proxy.n
    proxy.n.clear()
    pred = m.predict({c["name"]: g["X"][:, i] for i, c in enumerate(g["spec"]["dnn_columns"])}, batch_size=64)
    assert pred.shape == (g["X"].shape[0], 1)
    assert proxy.n.get("dctr_log_transform_fwd_eval") == 1 and "dctr_log_transform_fwd_train" not in proxy.n


def test_a_65_field_model_runs_on_the_torch_route(monkeypatch):
    from deepctr_torch._hip import lib as L
    from deepctr_torch.inputs import SparseFeat
    from deepctr_torch.models import AFN
    cols = [SparseFeat("C%d" % i, 5 + i % 3, 4) for i in range(65)]
    m = AFN(cols, cols, ltl_hidden_size=8, afn_dnn_hidden_units=(8,), device=DEV)
    proxy = _Counting(L.lib())
    monkeypatch.setattr(L, "lib", lambda: proxy)
    m.train()
    X = torch.from_numpy(np.random.RandomState(0).randint(0, 5, (16, 65)).astype(np.float32)).to(DEV)
    y = m(X)
    y.sum().backward()
    torch.cuda.synchronize()
    assert tuple(y.shape) == (16, 1) and bool(torch.isfinite(y).all())
    assert not any(k.startswith("dctr_log_transform") for k in proxy.n)
    assert m.ltl.ltl_weights.grad is not None
