"""Shared by the multi-task tests (tests/test_mtl_host.py on the stand-in, tests/test_gpu_mtl_models.py on the GPU): the fixture
list of tools/golden/make_mtl_golden.py, model construction from a spec, and the checks both files make."""
import json
import os

import numpy as np
import torch

from helpers import GOLDEN_DIR, feature_columns, load_golden, max_abs

LOGIT_TOL, GRAD_TOL, TRAJ_TOL = 1e-5, 2e-5, 2e-5
BASE = ["sb_towers", "sb_notower", "esmm", "mmoe", "mmoe_nogate", "mmoe_notower", "mmoe_three", "mmoe_two_experts", "ple_112",
        "ple_222", "ple_333_nogate", "ple_noshared", "mmoe_bn", "ple_mixed"]
ALL = BASE + ["lazy_mtl", "fit_mtl"]
STEPS = ["sb_towers", "esmm", "mmoe", "ple_112"]
RELU_MARGIN = 2e-6


def build(spec, device, l2=0.0, **more):
    """the drop-in model a spec names; ``l2``: the embedding regulariser (None: the constructor's default)"""
    import deepctr_torch.models as M
    kw = dict(spec["kwargs"], **more)
    if l2 is not None:
        kw.update(l2_reg_embedding=l2, l2_reg_linear=l2)
    return getattr(M, spec["model"])(feature_columns(spec["dnn_columns"]), device=device, **kw)


def loaded(name, device, l2=0.0):
    g = load_golden("mtl/" + name)
    m = build(g["spec"], device, l2=l2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    return g, m


def head_hooks(model, cap):
    """what the generator captured: the input of every head.  ESMM has one head, called for the CTR logit and then for the
    CVR logit: the generator took the outputs of its two projections, which the tower kernels compute here without
    calling the modules -- the head's two inputs are the same two tensors."""
    if isinstance(model.out, torch.nn.ModuleList):
        return [h.register_forward_pre_hook(lambda m, inp, i=i: cap.__setitem__(i, inp[0].detach().clone()))
                for i, h in enumerate(model.out)]
    return [model.out.register_forward_pre_hook(lambda m, inp: cap.__setitem__(len(cap), inp[0].detach().clone()))]


LOSSES = {"binary_crossentropy": torch.nn.functional.binary_cross_entropy, "mse": torch.nn.functional.mse_loss}


def list_loss(spec, y_pred, y):
    return sum(LOSSES[name](y_pred[:, i], y[:, i], reduction="sum") for i, name in enumerate(spec["losses"]))


def forward_logits(model, X):
    """-> (per-task logits [B, T], y_pred [B, T]) of one forward in the model's current mode"""
    cap = {}
    hooks = head_hooks(model, cap)
    y = model(X)
    for h in hooks:
        h.remove()
    return torch.cat([cap[i].reshape(-1, 1) for i in range(model.num_tasks)], 1), y


def grad_scale(key, grads, spec):
    """The gradient bound's scale: max|g_ref| of the parameter, no floor.  One exception, by reasoning and not by result
    (tests/test_ccpm_host.py): with ``dnn_use_bn`` a Linear bias sits directly in front of a BatchNorm in train mode, which
    subtracts the batch mean -- its exact gradient is 0 and the reference's own value is the rounding noise of a sum that
    cancels; the same layer's weight gradient gives the scale of the terms of that sum."""
    if spec["kwargs"].get("dnn_use_bn") and ".linears." in key and key.endswith(".bias"):
        key = key[:-len("bias")] + "weight"
    return float(np.max(np.abs(grads[key])))


def check_gradients(g, m, dev, out=None):
    """loss and every parameter gradient of fixture ``g`` on model ``m``; -> the largest error relative to its bound"""
    m.train()          # (not compiled: the tables' gradients then are plain dense tensors in .grad)
    y_pred = m(torch.from_numpy(g["X"]).to(dev))
    loss = list_loss(g["spec"], y_pred, torch.from_numpy(g["y"]).to(dev))
    m.zero_grad()
    loss.backward()
    assert abs(loss.item() - g["loss"]) <= 1e-4 * max(1.0, abs(g["loss"]))
    absent = set(json.loads(str(g["extra"]["grad_absent"])))
    assert set(g["grads"]) == set(k for k, _ in m.named_parameters())
    worst = 0.0
    for k, p in m.named_parameters():
        ref = g["grads"][k]
        if k in absent:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        err, scale = max_abs(p.grad.cpu().numpy(), ref), grad_scale(k, g["grads"], g["spec"])
        assert err <= GRAD_TOL * scale, "%s: max|d|=%.3e max|g_ref|=%.3g" % (k, err, scale)
        worst = max(worst, err / (GRAD_TOL * scale) if scale else 0.0)
    return worst


def check_trajectory(g, m, dev, opt):
    m.compile("adagrad" if opt == "adagradp" else opt, g["spec"]["losses"], metrics=[])
    if opt == "adagradp":
        for grp in m.optim.param_groups:
            for p in grp["params"]:
                m.optim.state[p]["sum"].fill_(0.05)
    m.train()
    losses = [float(m._train_step(torch.from_numpy(Xb).to(dev), torch.from_numpy(yb).to(dev))[0])
              for Xb, yb in zip(g["extra"]["X_steps"], g["extra"]["y_steps"])]
    np.testing.assert_allclose(losses, g["extra"][opt + "3_loss"], rtol=2e-5)
    sd = m.state_dict()
    n = 0
    for k, v in g["extra"].items():
        if k.startswith(opt + "3/"):
            assert max_abs(sd[k[len(opt) + 2:]].cpu().numpy(), v) <= TRAJ_TOL, k
            n += 1
    assert n == len(sd)


def check_lazy(g, dev, tag, l2):
    m = build(g["spec"], dev, l2=l2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    ex = g["extra"]
    m.compile("adam", g["spec"]["losses"], metrics=[])
    m.train()
    bce, tot = [], []
    for Xb, yb in zip(ex["lazy_X"], ex["lazy_y"]):
        loss, total, _ = m._train_step(torch.from_numpy(Xb).to(dev), torch.from_numpy(yb).to(dev))
        bce.append(float(loss))
        tot.append(float(total))
    np.testing.assert_allclose(bce, ex["lazy_%s_bce" % tag], rtol=2e-5)
    np.testing.assert_allclose(tot, ex["lazy_%s_total" % tag], rtol=2e-5)
    sd = m.state_dict()
    pre = "lazy_%s/" % tag
    for k, v in ex.items():
        if k.startswith(pre):
            ref = np.asarray(v, np.float64)
            assert max_abs(sd[k[len(pre):]].cpu().numpy(), ref) <= 2e-5 * max(1.0, float(np.max(np.abs(ref)))), k
    m.eval()
    with torch.no_grad():
        pred = m(torch.from_numpy(ex["lazy_X"][0]).to(dev))
    assert max_abs(pred.cpu().numpy(), ex["lazy_%s_pred" % tag]) <= 2e-5
    return m


def init_configs():
    """[(spec, {key: initial weight})] of tests/golden/mtl/init.npz and init_ple.npz, and the accepted metrics"""
    out, metrics = [], {}
    for name in ("init", "init_ple"):
        path = os.path.join(GOLDEN_DIR, "mtl", name + ".npz")
        if not os.path.exists(path):
            continue
        z = np.load(path, allow_pickle=False)
        metrics = json.loads(str(z["metrics"]))
        for i, spec in enumerate(json.loads(str(z["configs"]))):
            pre = "%d/param/" % i
            out.append((spec, {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}))
    return out, metrics


def config_id(c):
    kw = c[0]["kwargs"]
    return "%s-%s" % (c[0]["model"], "-".join("%s" % "x".join(str(e)[:3] for e in v) if isinstance(v, list) else str(v)
                                              for k, v in sorted(kw.items())))


def feature_dict(spec, X):
    from np_oracle import build_input_features
    return {n: (X[:, lo] if hi - lo == 1 else X[:, lo:hi])
            for n, (lo, hi) in build_input_features(spec["dnn_columns"]).items()}
