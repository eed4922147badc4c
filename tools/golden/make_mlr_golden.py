"""Generate tests/golden/mlr/*.npz by EXECUTING THE REFERENCE's MLR (torch-CPU fp32).

Like tools/golden/make_onn_golden.py: a sub-directory of its own, and everything that drives the reference imported from
oracle/make_golden.py (the TensorFlow stub, the column builders, ``synth_inputs``, ``randomise``).  ``run_case`` there hooks
``model.out`` (which MLR never calls) and builds models as ``cls(lin, dnn, ...)``, so the runner is here; it records the same
kinds of entries: ``spec``, ``X``, ``y``, ``param/*``, ``logit`` (the R (+ 1) head logits ``z``), ``y_pred``, ``loss``,
``grad/*`` (zeros where the reference leaves None), the 3-step ``sgd`` / ``adagrad`` / ``adagradp`` trajectories, the 8-step
runs of the lazy fixtures and a ``fit()`` History.

    python tools/golden/make_mlr_golden.py            # rewrites every fixture (deterministic)

A spec is ``{"model": "MLR", "region_columns", "base_columns" (None: the region columns), "bias_columns" (None: none),
"kwargs"}``.  Weights: ``randomise`` first, then the region tables and region dense weights N(0, 0.8) and the bias side
N(0, 0.3) -- with the default ``init_std`` the gate is uniform to seven digits and a wrong softmax would pass.  A fixture is
accepted only if ``y_pred`` spans at least 0.25 over the batch (a case that misses gets another seed, never another bound).

``init.npz`` holds freshly constructed ``state_dict``s at the default seed: the reference's own ``test_MLR`` shape (3 sparse
+ 3 dense + the three sequence columns, default kwargs) and one with bias columns and ``region_num=2``.
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

OUT_DIR = os.path.join(ROOT, "tests", "golden", "mlr")
MIN_SPAN = 0.25
REGION_STD, BIAS_STD = 0.8, 0.3

CASES = []


def case(name, region, base=None, bias=None, batch=33, seed=0, steps=False, lazy=False, fit=False, **kwargs):
    CASES.append({"name": name, "batch": batch, "seed": seed, "steps": steps, "lazy": lazy, "fit": fit,
                  "spec": {"model": "MLR", "region_columns": region, "base_columns": base, "bias_columns": bias,
                           "kwargs": kwargs}})


def prefixed(cols, prefix):
    out = []
    for c in cols:
        c = dict(c, name=prefix + c["name"])
        if c.get("embedding_name"):
            c["embedding_name"] = prefix + c["embedding_name"]
        if c.get("length_name"):
            c["length_name"] = prefix + c["length_name"]
        out.append(c)
    return out


case("mlr_bias", G.criteo_columns(3, 2, 7, 4), bias=prefixed(G.criteo_columns(2, 1, 6, 4), "b"), batch=33, region_num=4)
case("mlr_criteo", G.criteo_columns(9, 4, 22, 4), batch=40, steps=True, region_num=4)
case("mlr_two", G.criteo_columns(2, 0, 9, 4), batch=24, region_num=2)
# (two inputs in [0, 1): most draws of the weights move y_pred by less than MIN_SPAN over a batch; seed 14 is the first that
# does not)
case("mlr_dense_only", G.criteo_columns(0, 2, 9, 4), batch=17, seed=14, region_num=3)
case("mlr_r8", G.criteo_columns(1, 0, 12, 4), batch=20, region_num=8)
case("mlr_mixed", G.mixed_columns(), bias=prefixed(G.mixed_columns()[1:7], "b"), batch=33, steps=True, region_num=3)
case("mlr_regression", G.criteo_columns(4, 2, 10, 4), bias=prefixed(G.criteo_columns(1, 1, 5, 4), "b"), batch=29,
     steps=True, region_num=3, task="regression")
case("mlr_base", G.criteo_columns(3, 1, 8, 4), base=prefixed(G.criteo_columns(2, 2, 6, 4), "a"),
     bias=prefixed(G.criteo_columns(1, 0, 5, 4), "b"), batch=25, steps=True, region_num=2)
_l = G.criteo_columns(8, 3, 20, 4)
case("lazy_mlr", _l, bias=prefixed(G.criteo_columns(2, 1, 9, 4), "b"), batch=24, lazy=True, region_num=4)
case("fit_mlr", _l, bias=prefixed(G.criteo_columns(2, 1, 9, 4), "b"), batch=64, fit=True, region_num=4)


def seq_columns(prefix=""):
    """the reference's test data (tests/utils.py get_test_data): one sequence column per pooling mode"""
    return [G.varlen(prefix + "sequence_sum", 5, 4, 4, "sum"), G.varlen(prefix + "sequence_mean", 7, 4, 6, "mean"),
            G.varlen(prefix + "sequence_max", 4, 4, 3, "max")]


def test_columns(n_sparse, n_dense, prefix=""):
    return [G.sparse("%ssparse_feature_%d" % (prefix, i), 3 + 2 * i, 4) for i in range(n_sparse)] + \
        [G.dense("%sdense_feature_%d" % (prefix, i)) for i in range(n_dense)] + seq_columns(prefix)


INIT_CONFIGS = [
    {"model": "MLR", "region_columns": test_columns(3, 3, "region"), "base_columns": None, "bias_columns": None,
     "kwargs": {}},
    {"model": "MLR", "region_columns": G.criteo_columns(2, 2, 7, 4), "base_columns": None,
     "bias_columns": prefixed(G.criteo_columns(2, 1, 6, 4), "b"), "kwargs": {"region_num": 2, "init_std": 0.01}},
]


def all_columns(spec):
    """region + base + bias, the order ``MLR`` rebuilds ``feature_index`` over (de-duplicated by name)"""
    return spec["region_columns"] + (spec["base_columns"] or spec["region_columns"]) + (spec["bias_columns"] or [])


def build_reference_mlr(spec, l2=None):
    import deepctr_torch.inputs as ref_inputs
    import deepctr_torch.models as ref_models
    conv = lambda cols: None if cols is None else G.ref_columns(ref_inputs, cols)      # noqa: E731
    kw = dict(spec["kwargs"])
    if l2 is not None:
        kw["l2_reg_linear"] = l2
    return ref_models.MLR(conv(spec["region_columns"]), conv(spec["base_columns"]), conv(spec["bias_columns"]),
                          device="cpu", **kw)


def inputs_for(spec, batch, rng):
    return G.synth_inputs({"linear_columns": all_columns(spec), "dnn_columns": []}, batch, rng)


def randomise_mlr(model, rng):
    import torch
    G.randomise(model, rng)
    with torch.no_grad():
        for k, p in model.named_parameters():
            std = REGION_STD if k.startswith("region_linear_model.") else BIAS_STD if k.startswith("bias_model.") else None
            if std is not None:
                p.copy_(torch.from_numpy(rng.normal(0, std, tuple(p.shape)).astype(np.float32)))


def head_logits(model, xt):
    import torch
    with torch.no_grad():
        z = [lm(xt) for lm in model.region_linear_model]
        if hasattr(model, "bias_model"):
            z.append(model.bias_model[0](xt))
        return torch.cat(z, dim=-1).numpy()


def ref_step(m, Xb, yb):
    """the reference's own train step (basemodel.py:242-262) -> (loss, total)"""
    import torch
    yp = m(torch.from_numpy(Xb)).squeeze()
    m.optim.zero_grad()
    ls = m.loss_func(yp, torch.from_numpy(yb), reduction="sum")
    total = ls + m.get_regularization_loss() + m.aux_loss
    total.backward()
    m.optim.step()
    return ls.item(), total.item()


def run_case(case_):
    import torch
    import torch.nn.functional as F
    spec, batch = case_["spec"], case_["batch"]
    rng = np.random.default_rng(1000 + case_["seed"] + sum(map(ord, case_["name"])))
    torch.manual_seed(case_["seed"])
    binary = spec["kwargs"].get("task", "binary") == "binary"
    loss_name = "binary_crossentropy" if binary else "mse"
    model = build_reference_mlr(spec)
    randomise_mlr(model, rng)
    X, y = inputs_for(spec, batch, rng)
    out = {"spec": np.array(json.dumps(spec)), "X": X, "y": y}
    for k, v in model.state_dict().items():
        out["param/" + k] = v.detach().numpy().copy()
    model.train()
    xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    y_pred = model(xt).squeeze()
    loss = (F.binary_cross_entropy if binary else F.mse_loss)(y_pred, yt, reduction="sum")
    model.zero_grad()
    loss.backward()
    out["logit"] = head_logits(model, xt)
    out["y_pred"] = y_pred.detach().numpy().reshape(-1, 1)
    out["loss"] = np.array(loss.item(), np.float64)
    span = float(out["y_pred"].max() - out["y_pred"].min())
    if span < MIN_SPAN:
        raise SystemExit("%s: y_pred spans %.3f < %.2f over the batch -- give the case another seed" % (
            case_["name"], span, MIN_SPAN))
    for k, p in model.named_parameters():
        out["grad/" + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()

    if case_["steps"]:
        Xs, ys = zip(*[inputs_for(spec, batch, rng) for _ in range(3)])
        out["X_steps"], out["y_steps"] = np.stack(Xs), np.stack(ys)
        start = {k: v.clone() for k, v in model.state_dict().items()}
        for opt_name in ("sgd", "adagrad", "adagradp"):
            model.load_state_dict(start)
            model.compile("adagrad" if opt_name == "adagradp" else opt_name, loss_name, metrics=[])
            if opt_name == "adagradp":
                for grp in model.optim.param_groups:
                    for p in grp["params"]:
                        model.optim.state[p]["sum"].fill_(G.ADAGRAD_SUM0)
            losses = [ref_step(model, Xb, yb)[0] for Xb, yb in zip(Xs, ys)]
            out[opt_name + "3_loss"] = np.array(losses, np.float64)
            for k, v in model.state_dict().items():
                out[opt_name + "3/" + k] = v.detach().numpy().copy()
    if case_.get("lazy"):
        Xs, ys = zip(*[inputs_for(spec, batch, rng) for _ in range(G.LAZY_STEPS)])
        out["lazy_X"], out["lazy_y"] = np.stack(Xs), np.stack(ys)
        start = {k: v.clone() for k, v in model.state_dict().items()}
        # (l2_reg_linear is what the other models' runs regularise the tables with; MLR stores it and never applies it)
        for tag, opt_name, l2 in (("sgd", "sgd", G.LAZY_L2), ("adagrad", "adagrad", G.LAZY_L2), ("adam", "adam", G.LAZY_L2),
                                  ("adam0", "adam", 0.0)):
            torch.manual_seed(case_["seed"])
            m = build_reference_mlr(spec, l2=l2)
            m.load_state_dict(start)
            m.compile(opt_name, loss_name, metrics=[])
            m.train()
            both = [ref_step(m, Xb, yb) for Xb, yb in zip(Xs, ys)]
            out["lazy_%s_bce" % tag] = np.array([b[0] for b in both], np.float64)
            out["lazy_%s_total" % tag] = np.array([b[1] for b in both], np.float64)
            for k, v in m.state_dict().items():
                out["lazy_%s/%s" % (tag, k)] = v.detach().numpy().copy()
            m.eval()
            with torch.no_grad():
                out["lazy_%s_pred" % tag] = m(torch.from_numpy(Xs[0])).numpy().reshape(-1, 1)
    if case_.get("fit"):
        Xf, yf = inputs_for(spec, G.FIT_ROWS, rng)
        out["fit_X"], out["fit_y"] = Xf, yf
        xin = {n: Xf[:, lo:hi] for n, (lo, hi) in model.feature_index.items()}
        start = {k: v.clone() for k, v in model.state_dict().items()}
        for tag, opt_name, l2, shuffle in G.FIT_RUNS:
            torch.manual_seed(case_["seed"])
            m = build_reference_mlr(spec, l2=l2)
            m.load_state_dict(start)
            m.compile(opt_name, loss_name, metrics=["binary_crossentropy", "auc"])
            torch.manual_seed(G.FIT_SEED)
            hist = m.fit(xin, yf, batch_size=batch, epochs=G.FIT_EPOCHS, verbose=0, validation_split=G.FIT_SPLIT,
                         shuffle=shuffle)
            for k, v in hist.history.items():
                out["fit_%s_hist/%s" % (tag, k)] = np.asarray(v, np.float64)
            out["fit_%s_pred" % tag] = m.predict(xin, batch_size=50)
    return out


def init_fixture():
    """Freshly constructed reference models at their default seed."""
    out = {}
    for i, spec in enumerate(INIT_CONFIGS):
        for k, v in build_reference_mlr(spec).state_dict().items():
            out["%d/param/%s" % (i, k)] = v.detach().numpy().copy()
    out["configs"] = np.array(json.dumps(INIT_CONFIGS))
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
        yp = data["y_pred"]
        print("%-16s B=%-3d y_pred[min,max]=[%.3f,%.3f] span=%.3f loss=%.4f  -> %s (%.0f KB)" % (
            c["name"], c["batch"], yp.min(), yp.max(), yp.max() - yp.min(), float(data["loss"]), os.path.relpath(path),
            os.path.getsize(path) / 1024))
    if not names or "init" in names:
        path = os.path.join(OUT_DIR, "init.npz")
        np.savez_compressed(path, **init_fixture())
        print("init -> %s (%.0f KB)" % (os.path.relpath(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main(sys.argv[1:] or None)
