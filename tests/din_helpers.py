"""What tests/test_din_host.py and tests/test_gpu_din_models.py share: the fixture names, the model builder (DIN's
constructor takes ``history_feature_list`` and no linear columns, so ``helpers.build_model`` does not fit) and the checks
against a fixture (tests/golden/din, tools/golden/make_din_golden.py)."""
import json
import os

import numpy as np
import torch

from helpers import GOLDEN_DIR, feature_columns, load_golden, max_abs

LOGIT_TOL, GRAD_TOL, TRAJ_TOL = 1e-5, 2e-5, 2e-5
TRAIN = ["din_ref", "din_sigmoid", "din_relu", "din_prelu", "din_linear", "din_softmax", "din_one", "din_extra_varlen",
         "din_t50", "din_default_adam", "fit_din"]
ALL = TRAIN + ["din_dice_eval"]
STEPS = ["din_sigmoid", "din_relu"]
# fixtures whose attention net trains through the kernel (an element-wise activation); the others hold default Dice
KERNEL_TRAIN = [n for n in TRAIN if n not in ("din_ref", "din_default_adam")]


def build_din(spec, device, l2=0.0):
    from deepctr_torch.models import DIN
    return DIN(feature_columns(spec["dnn_columns"]), spec["history_feature_list"], l2_reg_embedding=l2, device=device,
               **spec["kwargs"])


def loaded(name, device, l2=0.0):
    g = load_golden("din/" + name)
    m = build_din(g["spec"], device, l2=l2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    return g, m


def init_configs():
    path = os.path.join(GOLDEN_DIR, "din", "init.npz")
    if not os.path.exists(path):
        return []
    z = np.load(path, allow_pickle=False)
    out = []
    for i, spec in enumerate(json.loads(str(z["configs"]))):
        pre = "%d/param/" % i
        out.append((spec, {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}))
    return out


def check_forward(g, m, device, train):
    m.train(train)
    cap = {}
    h = m.out.register_forward_pre_hook(lambda mod, inp: cap.__setitem__("logit", inp[0].detach()))
    with torch.no_grad():
        y = m(torch.from_numpy(g["X"]).to(device))
    h.remove()
    m.model_plan().check_ids()
    e1, e2 = max_abs(cap["logit"].cpu().numpy(), g["logit"]), max_abs(y.cpu().numpy(), g["y_pred"])
    print("logit %.3e y_pred %.3e" % (e1, e2))
    assert e1 <= LOGIT_TOL and e2 <= LOGIT_TOL


def grad_scale(key, grads, spec):
    """The gradient bound's scale: max|g_ref| of the parameter, no floor.  One exception, by reasoning and not by result:
    under ``att_weight_normalization`` the scores pass through a softmax, which is invariant to a shift of all of them, so
    the exact gradient of ``dense.bias`` is 0 and the reference's own value (9.3e-10 in din_softmax) is the rounding noise
    of a sum that cancels.  The terms of that sum are the d loss / d score that also form ``dense.weight``'s gradient
    (times activations in (0, 1)), so that gradient's scale is used."""
    if spec["kwargs"].get("att_weight_normalization") and key == "attention.local_att.dense.bias":
        key = "attention.local_att.dense.weight"
    return float(np.max(np.abs(grads[key])))


def check_gradients(g, m, device, train=True):
    m.train(train)
    y = m(torch.from_numpy(g["X"]).to(device)).squeeze(1)
    loss = torch.nn.functional.binary_cross_entropy(y, torch.from_numpy(g["y"]).to(device), reduction="sum")
    m.zero_grad()
    loss.backward()
    assert abs(loss.item() - g["loss"]) <= 1e-4 * max(1.0, abs(g["loss"]))
    assert set(g["grads"]) == set(k for k, _ in m.named_parameters())
    for k, p in m.named_parameters():
        ref = g["grads"][k]
        got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        err, scale = max_abs(got, ref), grad_scale(k, g["grads"], g["spec"])
        print("%-50s max|d|=%.3e max|g_ref|=%.3g" % (k, err, scale))
        assert err <= GRAD_TOL * scale, "%s: max|d|=%.3e max|g_ref|=%.3g" % (k, err, scale)


def check_trajectory(g, m, device, opt):
    """3 steps of the model's own train step against ``<opt>3/<key>`` and ``<opt>3_loss``"""
    m.compile("adagrad" if opt == "adagradp" else opt, "binary_crossentropy", metrics=[])
    if opt == "adagradp":
        for grp in m.optim.param_groups:
            for p in grp["params"]:
                m.optim.state[p]["sum"].fill_(0.05)
    m.train()
    ex = g["extra"]
    losses = [float(m._train_step(torch.from_numpy(Xb).to(device), torch.from_numpy(yb).to(device))[0])
              for Xb, yb in zip(ex["X_steps"], ex["y_steps"])]
    np.testing.assert_allclose(losses, ex[opt + "3_loss"], rtol=2e-5)
    sd = m.state_dict()
    n = 0
    for k, v in ex.items():
        if k.startswith(opt + "3/"):
            if k.endswith("num_batches_tracked"):
                assert int(sd[k[len(opt) + 2:]]) == int(v), k
            else:
                err = max_abs(sd[k[len(opt) + 2:]].cpu().numpy(), v)
                assert err <= TRAJ_TOL, "%s: %.3e" % (k, err)
            n += 1
    assert n == len(sd)
