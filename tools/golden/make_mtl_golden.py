"""Generate tests/golden/mtl/*.npz by EXECUTING THE REFERENCE's multi-task models (torch-CPU fp32): SharedBottom, ESMM,
MMOE, PLE.

Like the generators beside it: a sub-directory of its own, and what drives the reference is imported from
oracle/make_golden.py (the TensorFlow stub, the column builders, ``ref_columns``, ``randomise``, ``synth_inputs`` for ``X``).
``run_case`` there is single-task -- it passes ``lin, dnn``, hooks one ``model.out`` and takes one label column -- so this
tool has its own.

    python tools/golden/make_mtl_golden.py            # rewrites every fixture (deterministic)

A fixture holds what a fixture of oracle/make_golden.py holds, with these differences:
  ``y`` ``[B, num_tasks]``      binary tasks draw {0, 1}, regression tasks uniform [0, 1)
  ``logit`` ``[B, num_tasks]``  the input of every head (a pre-hook on each ``PredictionLayer``); ESMM has ONE head that is
                                called twice, so there it is the output of ``ctr_dnn_final_layer`` and
                                ``cvr_dnn_final_layer``
  ``loss``                      the summed list-loss: ``spec["losses"]`` holds one loss name per task (binary_crossentropy
                                for a binary task, mse for a regression task)
  ``grad_absent``               json list of the parameters the reference left WITHOUT a gradient (the shared gate of PLE's
                                last level feeds nothing); their ``grad/<key>`` is zeros
``steps`` cases: the 3-step ``sgd`` / ``adagrad`` / ``adagradp`` trajectories exactly as ``run_case`` does them
(``<opt>3_loss``, ``<opt>3/<key>``, ``X_steps``, ``y_steps`` ``[3, B, num_tasks]``).  ``lazy_mtl``: 8 steps of ``adam`` with the
default regularisation (``lazy_adam*``) and without any (``lazy_adam0*``).  ``fit_mtl``: ``fit()`` History and ``predict()``
of the three runs of oracle/make_golden.py; ``fit_metrics`` is the json list of the metrics the reference evaluated on
these ``[N, num_tasks]`` labels without raising -- found by running each candidate, not assumed.

ReLU kinks: a pre-activation within fp32 rounding of 0 may fall on either side in two implementations, and the unit's
gradient then exists in one and not in the other.  As in make_din_golden.py every ReLU input of every DNN is watched over
every forward of a case, and the fixture is accepted only if none is closer to 0 than RELU_MARGIN; otherwise the case's seed
advances.  ``seed`` and ``min_relu_margin`` are stored.

``init.npz`` (SharedBottom, ESMM, MMOE) and ``init_ple.npz``: the freshly constructed ``state_dict`` of every configuration of the reference's own multi-task tests
(tests/models/multitask/*_test.py) over fixed columns of their kind: ``configs`` (json list of specs), ``<i>/param/<key>``,
and ``metrics`` -- per task-type combination the metrics the reference's ``fit`` accepted.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402
from make_iafm_golden import offline_requests  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "mtl")
RELU_MARGIN = 2e-6
MAX_TRIES = 400
LAZY_STEPS = 8
METRIC_CANDIDATES = ("binary_crossentropy", "auc", "mse", "acc")
LOSS_OF = {"binary": "binary_crossentropy", "regression": "mse"}

CASES = []


def case(name, model, dnn, batch=32, seed=0, steps=False, mode=None, **kwargs):
    types = kwargs.get("task_types", ("binary", "binary"))
    CASES.append({"name": name, "batch": batch, "seed": seed, "steps": steps, "mode": mode,
                  "spec": {"model": model, "linear_columns": [], "dnn_columns": dnn, "kwargs": kwargs,
                           "losses": [LOSS_OF[t] for t in types]}})


SMALL = [G.sparse("user", 11, 4), G.sparse("item", 9, 4), G.sparse("cate", 6, 4), G.dense("price"), G.dense("ctx", 2)]
ODD = [G.sparse("user", 11, 5), G.sparse("item", 9, 3), G.dense("price")]          # input width 9: no multiple of 4
FIXED = G.criteo_columns(6, 2, 20, 4)

case("sb_towers", "SharedBottom", SMALL, steps=True, bottom_dnn_hidden_units=(32, 16), tower_dnn_hidden_units=(8,))
case("sb_notower", "SharedBottom", ODD, batch=24, bottom_dnn_hidden_units=(16,), tower_dnn_hidden_units=())
case("esmm", "ESMM", SMALL, steps=True, tower_dnn_hidden_units=(32, 16))
case("mmoe", "MMOE", SMALL, batch=64, steps=True, expert_dnn_hidden_units=(32, 16), gate_dnn_hidden_units=(16,),
     tower_dnn_hidden_units=(8,))
case("mmoe_nogate", "MMOE", ODD, batch=24, expert_dnn_hidden_units=(16, 7), gate_dnn_hidden_units=(),
     tower_dnn_hidden_units=(8,))
case("mmoe_notower", "MMOE", SMALL, expert_dnn_hidden_units=(16,), gate_dnn_hidden_units=(8,), tower_dnn_hidden_units=())
case("mmoe_three", "MMOE", SMALL, expert_dnn_hidden_units=(16, 8), gate_dnn_hidden_units=(8,),
     tower_dnn_hidden_units=(8,), task_types=("binary", "regression", "binary"), task_names=("ctr", "stay", "ctcvr"))
case("mmoe_two_experts", "MMOE", SMALL, num_experts=2, expert_dnn_hidden_units=(16,), gate_dnn_hidden_units=(8,),
     tower_dnn_hidden_units=(8,))
case("ple_112", "PLE", SMALL, steps=True, shared_expert_num=1, specific_expert_num=1, num_levels=2,
     expert_dnn_hidden_units=(32, 16), gate_dnn_hidden_units=(16,), tower_dnn_hidden_units=(8,))
case("ple_222", "PLE", SMALL, shared_expert_num=2, specific_expert_num=2, num_levels=2,
     expert_dnn_hidden_units=(16, 8), gate_dnn_hidden_units=(8,), tower_dnn_hidden_units=(8,))
case("ple_333_nogate", "PLE", ODD, batch=24, shared_expert_num=3, specific_expert_num=3, num_levels=3,
     expert_dnn_hidden_units=(16, 6), gate_dnn_hidden_units=(), tower_dnn_hidden_units=(8,))
case("ple_noshared", "PLE", SMALL, shared_expert_num=0, specific_expert_num=1, num_levels=2,
     expert_dnn_hidden_units=(16, 8), gate_dnn_hidden_units=(8,), tower_dnn_hidden_units=(),
     task_types=("binary", "regression"))
case("mmoe_bn", "MMOE", SMALL, expert_dnn_hidden_units=(16, 8), gate_dnn_hidden_units=(8,), tower_dnn_hidden_units=(8,),
     dnn_use_bn=True)
case("ple_mixed", "PLE", G.mixed_columns(4), shared_expert_num=1, specific_expert_num=2, num_levels=2,
     expert_dnn_hidden_units=(16, 8), gate_dnn_hidden_units=(8,), tower_dnn_hidden_units=(8,))
case("lazy_mtl", "MMOE", FIXED, mode="lazy", expert_dnn_hidden_units=(16, 8), gate_dnn_hidden_units=(8,),
     tower_dnn_hidden_units=(8,))
case("fit_mtl", "MMOE", FIXED, batch=64, mode="fit", expert_dnn_hidden_units=(16, 8), gate_dnn_hidden_units=(8,),
     tower_dnn_hidden_units=(8,))

# the reference's own tests (tests/models/multitask/*_test.py) over 3 sparse, 3 dense and its three sequence columns
_TEST = [G.sparse("sparse_feature_%d" % i, v, 4) for i, v in enumerate((5, 7, 9))] + \
    [G.dense("dense_feature_%d" % i) for i in range(3)] + \
    [G.varlen("sequence_sum", 6, 4, 4, "sum"), G.varlen("sequence_mean", 8, 4, 3, "mean"),
     G.varlen("sequence_max", 5, 4, 5, "max")]
_BB, _BR = ("binary", "binary"), ("binary", "regression")
INIT_CONFIGS = [("SharedBottom", dict(bottom_dnn_hidden_units=(32, 16), tower_dnn_hidden_units=t, task_types=ty))
                for t, ty in (((64,), _BB), ((), _BB), ((64,), _BR))]
INIT_CONFIGS += [("ESMM", dict(tower_dnn_hidden_units=(32, 16), task_types=_BB))]
INIT_CONFIGS += [("MMOE", dict(num_experts=3, expert_dnn_hidden_units=(32, 16), gate_dnn_hidden_units=g,
                               tower_dnn_hidden_units=t, task_types=ty))
                 for g, t, ty in (((64,), (64,), _BB), ((), (64,), _BB), ((64,), (), _BB), ((), (), _BB), ((64,), (64,), _BR))]
INIT_CONFIGS += [("PLE", dict(shared_expert_num=sh, specific_expert_num=sp, num_levels=lv, expert_dnn_hidden_units=(32, 16),
                              gate_dnn_hidden_units=g, tower_dnn_hidden_units=t, task_types=ty))
                 for sh, sp, lv, g, t, ty in ((1, 1, 2, (64,), (64,), _BB), (3, 3, 3, (), (64,), _BB), (3, 3, 3, (64,), (), _BB),
                                              (3, 3, 3, (), (), _BB), (3, 3, 3, (64,), (64,), _BR))]


def build_reference_model(spec, l2=None):
    """``l2``: strength of the embedding regulariser (None: the reference's default)"""
    import deepctr_torch.inputs as ref_inputs
    import deepctr_torch.models as ref_models
    kw = dict(spec["kwargs"])
    if l2 is not None:
        kw.update(l2_reg_embedding=l2, l2_reg_linear=l2)
    return getattr(ref_models, spec["model"])(G.ref_columns(ref_inputs, spec["dnn_columns"]), device="cpu", **kw)


def synth(spec, batch, rng):
    X, _ = G.synth_inputs(spec, batch, rng)
    types = spec["kwargs"].get("task_types", ("binary", "binary"))
    y = np.stack([rng.integers(0, 2, batch).astype(np.float32) if t == "binary" else rng.random(batch, dtype=np.float32)
                  for t in types], axis=1)
    return X, y


class Watch(object):
    """the smallest |ReLU input| any DNN of the watched models has seen"""

    def __init__(self):
        self.margin = float("inf")

    def attach(self, model):
        for mod in model.modules():
            if type(mod).__name__ == "DNN":
                for m in (mod.bn if mod.use_bn else mod.linears):
                    m.register_forward_hook(self.see)
        return model

    def see(self, mod, inp, res):
        self.margin = min(self.margin, float(res.detach().abs().min()))


def head_hooks(model, cap):
    """pre-PredictionLayer logits of every task into ``cap[i]``; -> the hook handles"""
    if isinstance(model.out, __import__("torch").nn.ModuleList):
        return [h.register_forward_pre_hook(lambda m, inp, i=i: cap.__setitem__(i, inp[0].detach().clone()))
                for i, h in enumerate(model.out)]
    return [fc.register_forward_hook(lambda m, inp, res, i=i: cap.__setitem__(i, res.detach().clone()))
            for i, fc in enumerate((model.ctr_dnn_final_layer, model.cvr_dnn_final_layer))]


def list_loss(model, y_pred, y):
    return sum(model.loss_func[i](y_pred[:, i], y[:, i], reduction="sum") for i in range(model.num_tasks))


def train_step(model, Xb, yb):
    """the reference's own step (basemodel.py:242-262, the num_tasks branch) -> (loss, total)"""
    import torch
    yp = model(torch.from_numpy(Xb)).squeeze()
    model.optim.zero_grad()
    ls = list_loss(model, yp, torch.from_numpy(yb))
    total = ls + model.get_regularization_loss() + model.aux_loss
    total.backward()
    model.optim.step()
    return ls.item(), total.item()


def base(c, watch, l2=0.0):
    """forward, list-loss and gradients in train mode; -> (out, model, rng)"""
    import torch
    spec = c["spec"]
    rng = np.random.default_rng(1000 + c["seed"] + sum(map(ord, c["name"])))
    torch.manual_seed(c["seed"])
    model = watch.attach(build_reference_model(spec, l2=l2))
    G.randomise(model, rng)
    X, y = synth(spec, c["batch"], rng)
    out = {"spec": np.array(json.dumps(spec)), "X": X, "y": y}
    for k, v in model.state_dict().items():
        out["param/" + k] = v.detach().numpy().copy()
    cap = {}
    hooks = head_hooks(model, cap)
    model.compile("sgd", spec["losses"], metrics=[])
    model.train()
    y_pred = model(torch.from_numpy(X))
    for h in hooks:
        h.remove()
    loss = list_loss(model, y_pred, torch.from_numpy(y))
    model.zero_grad()
    loss.backward()
    out["logit"] = torch.cat([cap[i].reshape(-1, 1) for i in range(model.num_tasks)], 1).numpy()
    out["y_pred"] = y_pred.detach().numpy().copy()
    out["loss"] = np.array(loss.item(), np.float64)
    absent = []
    for k, p in model.named_parameters():
        if p.grad is None:
            absent.append(k)
        out["grad/" + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    out["grad_absent"] = np.array(json.dumps(absent))
    return out, model, rng


def run_steps(c, out, model, rng):
    import torch
    spec = c["spec"]
    Xs, ys = zip(*[synth(spec, c["batch"], rng) for _ in range(3)])
    out["X_steps"], out["y_steps"] = np.stack(Xs), np.stack(ys)
    start = {k: v.clone() for k, v in model.state_dict().items()}
    for opt_name in ("sgd", "adagrad", "adagradp"):
        model.load_state_dict(start)
        model.compile("adagrad" if opt_name == "adagradp" else opt_name, spec["losses"], metrics=[])
        if opt_name == "adagradp":
            for grp in model.optim.param_groups:
                for p in grp["params"]:
                    model.optim.state[p]["sum"].fill_(G.ADAGRAD_SUM0)
        out[opt_name + "3_loss"] = np.array([train_step(model, Xb, yb)[0] for Xb, yb in zip(Xs, ys)], np.float64)
        for k, v in model.state_dict().items():
            out[opt_name + "3/" + k] = v.detach().numpy().copy()


def run_lazy(c, out, model, rng, watch):
    import torch
    spec = c["spec"]
    Xs, ys = zip(*[synth(spec, c["batch"], rng) for _ in range(LAZY_STEPS)])
    out["lazy_X"], out["lazy_y"] = np.stack(Xs), np.stack(ys)
    start = {k: v.clone() for k, v in model.state_dict().items()}
    for tag, l2 in (("adam", None), ("adam0", 0.0)):
        torch.manual_seed(c["seed"])
        m = watch.attach(build_reference_model(spec, l2=l2))
        m.load_state_dict(start)
        m.compile("adam", spec["losses"], metrics=[])
        m.train()
        both = [train_step(m, Xb, yb) for Xb, yb in zip(Xs, ys)]
        out["lazy_%s_bce" % tag] = np.array([b[0] for b in both], np.float64)
        out["lazy_%s_total" % tag] = np.array([b[1] for b in both], np.float64)
        for k, v in m.state_dict().items():
            out["lazy_%s/%s" % (tag, k)] = v.detach().numpy().copy()
        m.eval()
        with torch.no_grad():
            out["lazy_%s_pred" % tag] = m(torch.from_numpy(Xs[0])).numpy().copy()


def accepted_metrics(spec, X, y, batch):
    """the candidates the reference's own fit() / evaluate() get through on these labels, found by running them"""
    import contextlib
    import io
    import torch
    ok = []
    for name in METRIC_CANDIDATES:
        torch.manual_seed(0)
        m = build_reference_model(spec, l2=0.0)
        m.compile("adam", spec["losses"], metrics=[name])
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                m.fit(feature_dict(spec, X), y, batch_size=batch, epochs=1, verbose=2, validation_split=0.5)
        except Exception as e:      # the reference raises: the metric is not usable on such labels
            print("  metric %-20s refused by the reference: %s: %s" % (name, type(e).__name__, str(e)[:90]))
            continue
        ok.append(name)
    return ok


def feature_dict(spec, X):
    from np_oracle import build_input_features
    return {n: (X[:, lo] if hi - lo == 1 else X[:, lo:hi])
            for n, (lo, hi) in build_input_features(spec["dnn_columns"]).items()}


def run_fit(c, out, model, rng, watch):
    import contextlib
    import io
    import torch
    spec = c["spec"]
    Xf, yf = synth(spec, G.FIT_ROWS, rng)
    out["fit_X"], out["fit_y"] = Xf, yf
    metrics = accepted_metrics(spec, Xf, yf, c["batch"])
    out["fit_metrics"] = np.array(json.dumps(metrics))
    xin = feature_dict(spec, Xf)
    start = {k: v.clone() for k, v in model.state_dict().items()}
    for tag, opt_name, l2, shuffle in G.FIT_RUNS:
        torch.manual_seed(c["seed"])
        m = watch.attach(build_reference_model(spec, l2=l2))
        m.load_state_dict(start)
        m.compile(opt_name, spec["losses"], metrics=metrics)
        torch.manual_seed(G.FIT_SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            hist = m.fit(xin, yf, batch_size=c["batch"], epochs=G.FIT_EPOCHS, verbose=2, validation_split=G.FIT_SPLIT,
                         shuffle=shuffle)
        for k, v in hist.history.items():
            out["fit_%s_hist/%s" % (tag, k)] = np.asarray(v, np.float64)
        out["fit_%s_pred" % tag] = m.predict(xin, batch_size=50)


def run_case(c):
    for s in range(c["seed"], c["seed"] + MAX_TRIES):
        cs = dict(c, seed=s)
        watch = Watch()
        out, model, rng = base(cs, watch)
        if c["steps"]:
            run_steps(cs, out, model, rng)
        if c["mode"] == "lazy":
            run_lazy(cs, out, model, rng, watch)
        if c["mode"] == "fit":
            run_fit(cs, out, model, rng, watch)
        if watch.margin >= RELU_MARGIN:
            out["seed"] = np.array(s, np.int64)
            out["min_relu_margin"] = np.array(watch.margin, np.float64)
            return out
    raise RuntimeError("%s: no seed in %d tries keeps every ReLU input %g away from 0" % (c["name"], MAX_TRIES, RELU_MARGIN))


def init_fixture(ple):
    """Freshly constructed reference models at their default seed and default regularisation, and the metrics the
    reference's fit() accepts per combination of task types.  ``ple``: PLE's configurations (a file of their own: together
    the two would pass the size a committed file may have)."""
    out, configs, metrics = {}, [], {}
    for i, (model, kw) in enumerate(c for c in INIT_CONFIGS if (c[0] == "PLE") == ple):
        spec = {"model": model, "linear_columns": [], "dnn_columns": _TEST, "kwargs": kw,
                "losses": [LOSS_OF[t] for t in kw["task_types"]]}
        configs.append(spec)
        for k, v in build_reference_model(spec).state_dict().items():
            out["%d/param/%s" % (i, k)] = v.detach().numpy().copy()
        key = ",".join(kw["task_types"])
        if key not in metrics:
            X, y = synth(spec, 64, np.random.default_rng(7))
            metrics[key] = accepted_metrics(spec, X, y, 100)
    out["configs"] = np.array(json.dumps(configs))
    out["metrics"] = np.array(json.dumps(metrics))
    return out


def main(names=None):
    offline_requests()
    G.import_reference()
    os.makedirs(OUT_DIR, exist_ok=True)
    for c in CASES:
        if names and c["name"] not in names:
            continue
        data = run_case(c)
        path = os.path.join(OUT_DIR, c["name"] + ".npz")
        np.savez_compressed(path, **data)
        print("%-18s B=%-3d seed=%d margin=%.1e logit[min,max]=[%+.3f,%+.3f] loss=%.4f  -> %s (%.0f KB)" % (
            c["name"], c["batch"], int(data["seed"]), float(data["min_relu_margin"]), data["logit"].min(),
            data["logit"].max(), float(data["loss"]), os.path.relpath(path), os.path.getsize(path) / 1024))
    for name, ple in (("init", False), ("init_ple", True)):
        if not names or name in names:
            path = os.path.join(OUT_DIR, name + ".npz")
            np.savez_compressed(path, **init_fixture(ple))
            print("%s -> %s (%.0f KB)" % (name, os.path.relpath(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main(sys.argv[1:] or None)
