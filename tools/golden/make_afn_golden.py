"""Generate tests/golden/afn/*.npz by EXECUTING THE REFERENCE's AFN (torch-CPU fp32 and fp64).

Like tools/golden/make_ccpm_golden.py: a sub-directory of its own, everything that drives the reference imported from
oracle/make_golden.py unchanged.  ``G.run_case`` runs with ``steps`` where wanted and never with ``fit`` or ``lazy``: those
runs use Adagrad from zero accumulators and Adam on every parameter, and AFN has parameters whose exact gradient is zero
(every ``afn_dnn.linears.<i>.bias`` and ``ltl.bn.1.bias`` sit in front of a train-mode BatchNorm), so their first steps are
+-lr by the sign of rounding noise and no other implementation can replay them.

    python tools/golden/make_afn_golden.py            # rewrites every fixture (deterministic)

A fixture holds what ``run_case`` stores, plus what this file computes itself:

``ref64/...``  the same reference model, parameters and batch in float64 end to end (``torch.set_default_dtype`` around the
  run: the reference's ``Linear`` allocates its zero logit in the default dtype): ``ref64/logit``, ``ref64/grad/<key>``, and
  for ``steps`` fixtures ``ref64/<opt>3_loss`` and ``ref64/<opt>3/<key>`` for ``sgd`` and ``adagradp`` (as ``run_case``
  runs them: from the state after the first forward, whose running statistics have moved once).
``seed``, ``logit_dev``, ``grad_dev``  ACCEPTANCE, the seed advancing as in make_ccpm_golden's ``run_with_margin``: AFN's
  gradients are ill-conditioned (1/x of the log, exp, batch statistics over small batches), two correct float32
  implementations differ by what the reference itself differs from float64.  A fixture is accepted when
  max|logit32 - logit64| <= 2.5e-6 (the tests' flat 1e-5 keeps a 4x margin) and, for every parameter whose gradient is not
  exactly zero, max|g32 - g64| / max|g64| <= 5e-5.
``fit_<tag>_hist/<k>``, ``fit_<tag>_pred``  (the ``fit`` fixture) the reference's ``fit()``, 2 epochs, make_golden's rows and
  validation split: ``sgd`` unshuffled; ``adagradp`` = Adagrad with every accumulator preset to ``G.ADAGRAD_SUM0`` before
  ``fit``, shuffled (History and ``predict``); ``default`` = adam with L2 1e-5, shuffled (History only).

``init.npz``: the freshly constructed ``state_dict`` of the reference's own AFN test configuration
(tests/models/AFN_test.py: 3 sparse features, hidden (32, 16)) and of one 26-field model.
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

OUT_DIR = os.path.join(ROOT, "tests", "golden", "afn")
LOGIT_DEV, GRAD_DEV = 2.5e-6, 5e-5
MAX_TRIES = 300
FIT_EPOCHS = 2
FIT_RUNS = (("sgd", "sgd", 0.0, False, False), ("adagradp", "adagrad", 0.0, True, True),
            ("default", "adam", 1e-5, True, False))       # tag, optimizer, l2, shuffle, preset accumulators

CASES = []


def case(name, lin, dnn, batch=64, seed=0, steps=False, fit=False, **kwargs):
    CASES.append({"name": name, "batch": batch, "seed": seed, "steps": steps, "lazy": False, "fit": False, "afn_fit": fit,
                  "spec": {"model": "AFN", "linear_columns": lin, "dnn_columns": dnn, "kwargs": kwargs}})


_t = G.criteo_columns(2, 0, 7, 4)
case("afn_two", _t, _t, batch=33, steps=True, ltl_hidden_size=8, afn_dnn_hidden_units=(8,))
_h = G.criteo_columns(3, 0, 9, 4)
case("afn_three", _h, _h, batch=20, ltl_hidden_size=8, afn_dnn_hidden_units=(8,))
_c = G.criteo_columns(9, 4, 22, 8)
case("afn_criteo", _c, _c, batch=40, steps=True, ltl_hidden_size=32, afn_dnn_hidden_units=(32, 16))
_f = G.criteo_columns(26, 0, 48, 16)
# (the Criteo layer shape; the tower on top of its 4096 outputs is kept narrow: linears.0.weight is stored three times --
# value, gradient, float64 gradient -- and a committed file stays under 1 MiB)
case("afn_f26", _f, _f, batch=16, ltl_hidden_size=256, afn_dnn_hidden_units=(8, 4))
_s = G.criteo_columns(5, 0, 12, 6)
case("afn_nolinear", [], _s, batch=20, ltl_hidden_size=16, afn_dnn_hidden_units=(8,))
_a = G.criteo_columns(4, 0, 10, 8)
case("afn_sigmoid", _a, _a, batch=24, ltl_hidden_size=16, afn_dnn_hidden_units=(16, 8), dnn_activation="sigmoid")
_v = [G.sparse("user", 11, 4), G.sparse("item", 9, 4), G.varlen("tags_mean", 7, 4, 5, "mean")]
case("afn_varlen", _v, _v, batch=33, ltl_hidden_size=8, afn_dnn_hidden_units=(8,))
_q = G.criteo_columns(4, 0, 20, 8)
case("fit_afn", _q, _q, batch=64, fit=True, ltl_hidden_size=16, afn_dnn_hidden_units=(16, 8))

# (a 26-field model at default sizes has a 4 MB first tower weight; the committed file stays under 1 MiB, so the second
# configuration keeps the defaults' structure -- two hidden layers, relu -- at a quarter of the embedding and layer sizes)
INIT_CONFIGS = [(3, 4, dict(afn_dnn_hidden_units=(32, 16))),
                (26, 4, dict(ltl_hidden_size=64, afn_dnn_hidden_units=(64, 32)))]


def zero_gradient(key):
    """parameters whose exact train-mode gradient is 0: a per-unit constant in front of a train-mode BatchNorm"""
    return (key.startswith("afn_dnn.linears.") and key.endswith(".bias")) or key == "ltl.bn.1.bias"


def _step(model, Xb, yb, torch):
    yp = model(torch.from_numpy(Xb).to(torch.get_default_dtype())).squeeze()
    model.optim.zero_grad()
    ls = model.loss_func(yp, torch.from_numpy(yb).to(torch.get_default_dtype()), reduction="sum")
    total = ls + model.get_regularization_loss() + model.aux_loss
    total.backward()
    model.optim.step()
    return ls.item()


def float64_run(ref, c, data):
    """The reference in float64 on the fixture's parameters and batches -> the ``ref64/`` entries."""
    import torch
    import torch.nn.functional as F
    out = {}
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(c["seed"])
        model = G.build_reference_model(ref, c["spec"]).double()
        model.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in data.items() if k.startswith("param/")})
        captured = {}
        hook = model.out.register_forward_pre_hook(lambda m, inp: captured.__setitem__("logit", inp[0].detach().clone()))
        model.train()
        y_pred = model(torch.from_numpy(data["X"]).double()).squeeze()
        hook.remove()
        loss = F.binary_cross_entropy(y_pred, torch.from_numpy(data["y"]).double(), reduction="sum")
        model.zero_grad()
        loss.backward()
        out["ref64/logit"] = captured["logit"].numpy().reshape(-1, 1)
        for k, p in model.named_parameters():
            out["ref64/grad/" + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
        if c["steps"]:
            start = {k: v.clone() for k, v in model.state_dict().items()}
            for opt_name in ("sgd", "adagradp"):
                model.load_state_dict(start)
                model.compile("adagrad" if opt_name == "adagradp" else opt_name, "binary_crossentropy", metrics=[])
                if opt_name == "adagradp":
                    for grp in model.optim.param_groups:
                        for p in grp["params"]:
                            model.optim.state[p]["sum"].fill_(G.ADAGRAD_SUM0)
                losses = [_step(model, Xb, yb, torch) for Xb, yb in zip(data["X_steps"], data["y_steps"])]
                out["ref64/%s3_loss" % opt_name] = np.array(losses, np.float64)
                for k, v in model.state_dict().items():
                    out["ref64/%s3/%s" % (opt_name, k)] = v.detach().numpy().copy()
    finally:
        torch.set_default_dtype(torch.float32)
    return out


def deviations(data):
    logit_dev = float(np.max(np.abs(data["logit"].astype(np.float64) - data["ref64/logit"])))
    grad_dev = {}
    for k, g64 in data.items():
        if k.startswith("ref64/grad/") and not zero_gradient(k[len("ref64/grad/"):]):
            scale = float(np.max(np.abs(g64)))
            d = float(np.max(np.abs(data["grad/" + k[len("ref64/grad/"):]].astype(np.float64) - g64)))
            grad_dev[k[len("ref64/grad/"):]] = d / scale if scale > 0 else (0.0 if d == 0 else float("inf"))
    return logit_dev, grad_dev


def fit_runs(ref, c, data, rng):
    """the reference's ``fit()`` from the fixture's parameters (the keys follow run_case's ``fit_<tag>_hist/`` pattern)"""
    import torch
    spec = c["spec"]
    Xf, yf = G.synth_inputs(spec, G.FIT_ROWS, rng)
    out = {"fit_X": Xf, "fit_y": yf}
    xin = {col["name"]: Xf[:, i] for i, col in enumerate(spec["dnn_columns"])}     # one column per feature (no VarLen)
    start = {k[6:]: torch.from_numpy(v) for k, v in data.items() if k.startswith("param/")}
    for tag, opt_name, l2, shuffle, preset in FIT_RUNS:
        torch.manual_seed(c["seed"])
        m = G.build_reference_model(ref, spec, l2=l2)
        m.load_state_dict(start)
        m.compile(opt_name, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
        if preset:
            for grp in m.optim.param_groups:
                for p in grp["params"]:
                    m.optim.state[p]["sum"].fill_(G.ADAGRAD_SUM0)
        torch.manual_seed(G.FIT_SEED)
        hist = m.fit(xin, yf, batch_size=c["batch"], epochs=FIT_EPOCHS, verbose=0, validation_split=G.FIT_SPLIT,
                     shuffle=shuffle)
        for k, v in hist.history.items():
            out["fit_%s_hist/%s" % (tag, k)] = np.asarray(v, np.float64)
        if tag != "default":
            out["fit_%s_pred" % tag] = m.predict(xin, batch_size=50)
    return out


def run_accepted(ref, c):
    """``run_case`` + the float64 run at the first seed from the case's own at which the reference's float32 values are
    within LOGIT_DEV / GRAD_DEV of its float64 ones."""
    for s in range(c["seed"], c["seed"] + MAX_TRIES):
        cs = dict(c, seed=s)
        data = G.run_case(ref, cs)
        data.update(float64_run(ref, cs, data))
        logit_dev, grad_dev = deviations(data)
        if logit_dev <= LOGIT_DEV and max(grad_dev.values()) <= GRAD_DEV:
            data["seed"] = np.array(s, np.int64)
            data["logit_dev"] = np.array(logit_dev, np.float64)
            data["grad_dev"] = np.array(max(grad_dev.values()), np.float64)
            if c["afn_fit"]:
                rng = np.random.default_rng(2000 + s + sum(map(ord, c["name"])))
                data.update(fit_runs(ref, cs, data, rng))
            return data
    raise RuntimeError("%s: no seed in %d tries is within the acceptance margins" % (c["name"], MAX_TRIES))


def init_fixture():
    """Freshly constructed reference models at their default seed and default regularisation."""
    import deepctr_torch.inputs as ref_inputs
    import deepctr_torch.models as ref_models
    out, configs = {}, []
    for i, (n, dim, kw) in enumerate(INIT_CONFIGS):
        cols = G.criteo_columns(n, 0, 7, dim)
        spec = {"model": "AFN", "linear_columns": cols, "dnn_columns": cols, "kwargs": kw}
        configs.append(spec)
        fc = G.ref_columns(ref_inputs, cols)
        m = ref_models.AFN(fc, fc, device="cpu", **kw)
        for k, v in m.state_dict().items():
            out["%d/param/%s" % (i, k)] = v.detach().numpy().copy()
    out["configs"] = np.array(json.dumps(configs))
    return out


def main(names=None):
    offline_requests()
    ref = G.import_reference()
    os.makedirs(OUT_DIR, exist_ok=True)
    for c in CASES:
        if names and c["name"] not in names:
            continue
        data = run_accepted(ref, c)
        path = os.path.join(OUT_DIR, c["name"] + ".npz")
        np.savez_compressed(path, **data)
        print("%-14s B=%-3d seed=%-3d logit_dev=%.2e grad_dev=%.2e logit[min,max]=[%+.3f,%+.3f] loss=%.4f  -> %s (%.0f KB)" % (
            c["name"], c["batch"], int(data["seed"]), float(data["logit_dev"]), float(data["grad_dev"]), data["logit"].min(),
            data["logit"].max(), float(data["loss"]), os.path.relpath(path), os.path.getsize(path) / 1024))
    if not names or "init" in names:
        path = os.path.join(OUT_DIR, "init.npz")
        np.savez_compressed(path, **init_fixture())
        print("init -> %s (%.0f KB)" % (os.path.relpath(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main(sys.argv[1:] or None)
