"""GPU: the autograd-route train step under ``compile("adam")`` / ``"rmsprop"`` -- the dense parameters on
dctr_dense_opt_multi_reg (stacked weight groups on dctr_dense_opt_reg) with a device-side step count
(BaseModel._step_dense_multi / _step_stacked_groups) -- through the models: fit() replays hipGraphs, the kernel route
equals the ``torch.optim`` route (DCTR_MULTI_ADAM=0), a checkpoint carries the count over, and everything
``match_optimizer`` refuses keeps torch's semantics.

Bars.  Graph against eager: 1e-6 * max(1, |v|) and History rtol 1e-6 (tests/test_gpu_models.py's bars for the same
comparison: the same kernels on both sides).  Kernel route against torch route: 1e-4 * scale (adam), 3e-4 * scale
(rmsprop), scale = max(1, max|ref|) -- the bars tests/test_gpu_lazy.py uses between two routes of one optimizer: both
divide by sqrt(v) + eps with v ~ g^2, so an ulp in g moves a first step by a visible fraction of lr, RMSprop (no bias
correction, 10 lr steps from a zero accumulator) three times as far."""
import io

import numpy as np
import pytest
import torch

from helpers import build_model, feature_columns, load_golden, max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# fibinet_all is the smallest FiBiNET fixture (one shared bilinear matrix: no stacked group); fibinet_each the smallest
# whose bilinear weights form stacked groups (_step_stacked_groups)
NAMES = ["dcn_vector", "xdeepfm_criteo", "afm_criteo", "fibinet_all", "fibinet_each"]
BAR = {"adam": 1e-4, "rmsprop": 3e-4}
MOMENTS = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg",)}


def _model(name, default_l2, params=True):
    """the fixture's model with l2 = 0 everywhere, or with the model class's own default L2 kwargs"""
    g = load_golden(name)
    spec = g["spec"]
    if default_l2:
        import deepctr_torch.models as M
        m = getattr(M, spec["model"])(feature_columns(spec["linear_columns"]), feature_columns(spec["dnn_columns"]),
                                      device=DEV, **spec["kwargs"])
    else:
        m = build_model(spec, DEV)
    if params:
        m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    return g, m


def _fit_data(g, m):
    names = []
    for c in g["spec"]["linear_columns"] + g["spec"]["dnn_columns"]:
        if c["name"] not in names:
            names.append(c["name"])
    n = (g["X"].shape[0] // 16) * 16
    X = np.concatenate([g["X"][:n]] * 3, axis=0)
    y = np.concatenate([g["y"][:n]] * 3, axis=0)
    fi = m.feature_index
    return {nm: X[:, fi[nm][0]] for nm in names}, y


def _batches(g, n):
    X, y = torch.from_numpy(g["X"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    nb = X.shape[0] // 16
    return [(X[(i % nb) * 16:(i % nb) * 16 + 16], y[(i % nb) * 16:(i % nb) * 16 + 16]) for i in range(n)]


def _dense(m):
    tables = set(id(p) for p in m.model_plan().table_params)
    return [(k, p) for k, p in m.named_parameters() if id(p) not in tables]


def _close(tag, a, b, bar):
    for k in b:
        scale = max(1.0, float(b[k].abs().max()))
        err = max_abs(a[k].cpu().numpy(), b[k].cpu().numpy())
        assert err <= bar * scale, "%s %s: %.3e (scale %.3g)" % (tag, k, err, scale)


def _moments(m, opt):
    out = {}
    for k, p in m.named_parameters():
        st = m.optim.state.get(p, {})
        for key in MOMENTS[opt]:
            if key in st:
                out[k + "/" + key] = st[key].detach().clone()
    return out


def _count_optim_steps(m, monkeypatch):
    hits = []
    real = m.optim.step
    monkeypatch.setattr(m.optim, "step", lambda *a, **k: (hits.append(1), real(*a, **k))[1])
    return hits


@pytest.mark.parametrize("default_l2", [False, True])
@pytest.mark.parametrize("opt", ["adam", "rmsprop"])
@pytest.mark.parametrize("name", NAMES)
def test_fit_replays_graphs_under_adam_and_rmsprop(name, opt, default_l2, monkeypatch):
    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("DCTR_FIT_GRAPH", flag)
        g, m = _model(name, default_l2)
        m.compile(opt, "binary_crossentropy", metrics=[])
        x, y = _fit_data(g, m)
        hits = _count_optim_steps(m, monkeypatch)
        hist = m.fit(x, y, batch_size=16, epochs=2, verbose=0, shuffle=False)
        used = m._fit_graph is not None and m._fit_graph.get("graph") is not None
        assert not hits, "optim.step() ran: the kernel did not step every parameter"
        if name == "fibinet_each":
            assert m._stacked_cache[2], "the stacked groups' state was not re-seated: they went to the multi-tensor list"
        runs.append(({k: v.clone() for k, v in m.state_dict().items()}, dict(hist.history), used))
        m.optim.state_dict()
        steps = set(float(m.optim.state[p]["step"]) for _, p in _dense(m))
        assert steps == {2.0 * (len(y) // 16)}, steps          # the count survived the replays (18 steps)
    (a, ha, ua), (b, hb, ub) = runs
    assert ua and not ub
    _close("graph vs eager", a, b, 1e-6)
    np.testing.assert_allclose(ha["loss"], hb["loss"], rtol=1e-6)


def _eight_steps(name, opt, default_l2, monkeypatch, flag, n=8):
    monkeypatch.setenv("DCTR_MULTI_ADAM", flag)
    g, m = _model(name, default_l2)
    m.compile(opt, "binary_crossentropy", metrics=[])
    m.train()
    hits = _count_optim_steps(m, monkeypatch)
    for xb, yb in _batches(g, n):
        m._train_step(xb, yb)
    torch.cuda.synchronize()
    return g, m, hits


@pytest.mark.parametrize("default_l2", [False, True])
@pytest.mark.parametrize("opt", ["adam", "rmsprop"])
@pytest.mark.parametrize("name", NAMES)
def test_kernel_route_equals_torch_route(name, opt, default_l2, monkeypatch):
    """``afm_criteo`` is the sharp case: its attention path yields gradients that cancel to ~1e-8, whose sign is rounding
    noise (tests/test_gpu_models.py says the same of its Adagrad trajectory), and both optimizers turn a sign into a step
    of lr (10 lr for RMSprop from a small accumulator): ONE ulp in fm.attention_W after the first RMSprop step is 1.4e-2
    on fm.attention_b after the second.  The bars are met because the kernel gives torch's bits (opt_step_pinned,
    csrc/lazy_opt.hpp); with a 1-ulp square root in the step it missed them by 2.0e-2 (rmsprop) and 1.4e-4 (adam)."""
    g, mk, hk = _eight_steps(name, opt, default_l2, monkeypatch, "1")
    _, mt, ht = _eight_steps(name, opt, default_l2, monkeypatch, "0")
    assert not hk and len(ht) == 8
    _close("state_dict", mk.state_dict(), mt.state_dict(), BAR[opt])
    _close("optimizer state", _moments(mk, opt), _moments(mt, opt), BAR[opt])
    for m in (mk, mt):
        m.optim.state_dict()
        for k, p in _dense(m):
            assert float(m.optim.state[p]["step"]) == 8, k


@pytest.mark.parametrize("default_l2", [False, True])
@pytest.mark.parametrize("name", ["dcn_vector", "fibinet_each"])
def test_checkpoint_carries_the_step_count(name, default_l2, monkeypatch):
    g, m, hits = _eight_steps(name, "adam", default_l2, monkeypatch, "1", n=5)
    assert not hits
    buf = io.BytesIO()
    torch.save({"model": m.state_dict(), "optim": m.optim.state_dict()}, buf)
    out = []
    for flag in ("1", "0"):
        monkeypatch.setenv("DCTR_MULTI_ADAM", flag)
        buf.seek(0)
        ck = torch.load(buf)
        _, m2 = _model(name, default_l2, params=False)
        m2.load_state_dict(ck["model"])
        optim = torch.optim.Adam(m2.parameters())
        optim.load_state_dict(ck["optim"])
        m2.compile(optim, "binary_crossentropy", metrics=[])
        m2.train()
        hits2 = _count_optim_steps(m2, monkeypatch)
        for xb, yb in _batches(g, 8)[5:]:
            m2._train_step(xb, yb)
        torch.cuda.synchronize()
        assert len(hits2) == (0 if flag == "1" else 3)
        m2.optim.state_dict()
        for k, p in _dense(m2):
            assert float(m2.optim.state[p]["step"]) == 8, k
        out.append(m2)
    _close("resumed state_dict", out[0].state_dict(), out[1].state_dict(), BAR["adam"])
    _close("resumed optimizer state", _moments(out[0], "adam"), _moments(out[1], "adam"), BAR["adam"])


@pytest.mark.parametrize("make", [lambda ps: torch.optim.Adam(ps, amsgrad=True),
                                  lambda ps: torch.optim.Adam(ps, weight_decay=1e-4),
                                  lambda ps: torch.optim.RMSprop(ps, momentum=0.9)],
                         ids=["adam-amsgrad", "adam-weight_decay", "rmsprop-momentum"])
def test_optimizers_the_matcher_refuses_stay_on_torch(make, monkeypatch):
    g, m = _model("dcn_vector", True)
    m.compile(make(m.parameters()), "binary_crossentropy", metrics=[])
    m.train()
    hits = _count_optim_steps(m, monkeypatch)
    for xb, yb in _batches(g, 3):
        m._train_step(xb, yb)
    torch.cuda.synchronize()
    assert len(hits) == 3 and m.__dict__.get("_dense_clock") is None
    assert not m._graph_safe_step()
    assert all(torch.isfinite(p).all() for p in m.parameters())


@pytest.mark.parametrize("opt", ["adam", "rmsprop"])
def test_learning_rate_changed_between_epochs_is_honoured(opt, monkeypatch):
    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("DCTR_MULTI_ADAM", flag)
        g, m = _model("dcn_vector", True)
        m.compile(opt, "binary_crossentropy", metrics=[])
        x, y = _fit_data(g, m)
        m.fit(x, y, batch_size=16, epochs=1, verbose=0, shuffle=False)
        first = m._fit_graph.get("graph") if m._fit_graph is not None else None
        assert (first is not None) == (flag == "1")
        for grp in m.optim.param_groups:
            grp["lr"] = 10.0 * grp["lr"]
        m.fit(x, y, batch_size=16, epochs=1, verbose=0, shuffle=False)
        if flag == "1":
            second = m._fit_graph.get("graph") if m._fit_graph is not None else None
            assert second is not None and second is not first          # dropped, captured again with the new value
        runs.append(m)
    _close("lr x 10 in epoch 2", runs[0].state_dict(), runs[1].state_dict(), BAR[opt])
    for m in runs:
        m.optim.state_dict()
        assert set(float(m.optim.state[p]["step"]) for _, p in _dense(m)) == {2.0 * (len(y) // 16)}


@pytest.mark.parametrize("default_l2", [False, True])
def test_a_gradient_that_is_none_for_one_step_leaves_that_count_behind(default_l2, monkeypatch):
    runs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("DCTR_MULTI_ADAM", flag)
        g, m = _model("dcn_vector", default_l2)
        m.compile("adam", "binary_crossentropy", metrics=[])
        m.train()
        frozen = dict(m.named_parameters())["crossnet.bias"]
        for i, (xb, yb) in enumerate(_batches(g, 3)):
            frozen.requires_grad_(i != 1)
            m._train_step(xb, yb)
        torch.cuda.synchronize()
        m.optim.state_dict()
        for k, p in _dense(m):
            assert float(m.optim.state[p]["step"]) == (2 if p is frozen else 3), k
        runs.append(m)
    _close("frozen for one step", runs[0].state_dict(), runs[1].state_dict(), BAR["adam"])
