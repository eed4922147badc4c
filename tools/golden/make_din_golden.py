"""Generate tests/golden/din/*.npz by EXECUTING THE REFERENCE's DIN (torch-CPU fp32).

Like tools/golden/make_ccpm_golden.py: a sub-directory of its own, and what drives the reference is imported from
oracle/make_golden.py (the TensorFlow stub, the column builders, ``randomise``, ``run_case`` unchanged).  ``run_case``
looks its model builder and its input generator up in that module, and neither knows DIN -- the constructor takes
``history_feature_list`` and no linear columns; every history column shares ONE length column -- so this tool puts its own
two in their place while it runs.  A fixture holds exactly what a fixture there holds; the spec also has
``history_feature_list``.

    python tools/golden/make_din_golden.py            # rewrites every fixture (deterministic)

Inputs: batches of 16 to 40 rows; the rows 0..3 of every batch have the lengths 0, 1, T - 1 and T, the others are drawn
from 0..T.  Ids beyond a row's length are the padding id 0.

Beyond ``run_case``: ``din_dice_eval`` (BatchNorm running statistics set to non-trivial values, then forward, loss and
gradients in EVAL mode), ``din_default_adam`` (default keyword arguments, 3 steps of ``adam``: ``adam3/<key>``,
``adam3_loss``) and ``fit_din`` (``fit()`` History and ``predict()``, with ``verbose=2`` as oracle/make_golden.py runs it -- the reference records
the training metrics only when it prints them: ``fit_<run>_hist/<metric>``, ``fit_<run>_pred``).
``init.npz``: the freshly constructed ``state_dict`` of the reference's own DIN test configuration and of one default
configuration: ``configs`` (json list of specs) and ``<i>/param/<key>``.
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

OUT_DIR = os.path.join(ROOT, "tests", "golden", "din")
LEN = "seq_length"

CASES = []


def case(name, dnn, hist, batch=24, seed=0, steps=False, mode=None, **kwargs):
    CASES.append({"name": name, "batch": batch, "seed": seed, "steps": steps, "lazy": False, "fit": False, "mode": mode,
                  "spec": {"model": "DIN", "linear_columns": [], "dnn_columns": dnn, "history_feature_list": hist,
                           "kwargs": kwargs}})


def behaviour_columns(feats, T, others=(), dense=0, first=()):
    """``feats``: (name, vocab, dim) of the candidate features; each gets a history column ``hist_<name>`` of T positions
    over the same table.  ``first``: VarLen columns declared in front of everything else."""
    cols = list(first) + [G.sparse(n, v, d) for n, v, d in others] + [G.sparse(n, v, d) for n, v, d in feats]
    cols += [G.dense("d%d" % i) for i in range(dense)]
    cols += [G.varlen("hist_" + n, v, d, T, "mean", length_name=LEN, embedding_name=n) for n, v, d in feats]
    return cols


# the reference's own test (tests/models/DIN_test.py): user / gender of 4, item of 8, category of 4, one dense, T = 4
_ref = behaviour_columns([("item_id", 9, 8), ("cate_id", 6, 4)], 4, others=[("user", 7, 4), ("gender", 2, 4)], dense=1)
_hist = ["item_id", "cate_id"]
SMALL = dict(dnn_hidden_units=(32, 16))
case("din_ref", _ref, _hist, batch=24, att_hidden_size=(64, 16), **SMALL)                       # default Dice, train mode
case("din_sigmoid", _ref, _hist, batch=33, steps=True, att_activation="sigmoid", **SMALL)
case("din_relu", _ref, _hist, batch=24, steps=True, att_activation="relu", att_hidden_size=(80, 40), **SMALL)
case("din_prelu", _ref, _hist, batch=24, att_activation="prelu", att_hidden_size=(16, 8, 4), **SMALL)
case("din_linear", _ref, _hist, batch=16, att_activation="linear", att_hidden_size=(8,), **SMALL)
case("din_softmax", _ref, _hist, batch=40, att_activation="sigmoid", att_weight_normalization=True, **SMALL)
case("din_one", behaviour_columns([("item", 11, 6)], 5), ["item"], batch=20, att_activation="sigmoid",
     att_hidden_size=(16, 8), **SMALL)
# a pooled VarLen column with a length column of its own, declared FIRST: the reference reads the attention's lengths
# from the first length_name among ALL VarLen columns, i.e. from this one
_tags = [G.varlen("tags", 8, 4, 3, "mean", length_name="tags_length")]
case("din_extra_varlen", behaviour_columns([("item", 9, 8), ("cate", 6, 4)], 4, others=[("user", 7, 4)], dense=1,
                                           first=_tags),
     ["item", "cate"], batch=24, att_activation="sigmoid", att_hidden_size=(16, 8), **SMALL)
case("din_t50", behaviour_columns([("item", 40, 16), ("cate", 12, 16)], 50, others=[("user", 9, 8)]), ["item", "cate"],
     batch=16, att_activation="sigmoid", att_hidden_size=(64, 16), **SMALL)
case("din_dice_eval", _ref, _hist, batch=24, mode="eval", att_hidden_size=(16, 8), **SMALL)
case("din_default_adam", _ref, _hist, batch=32, mode="adam")
case("fit_din", _ref, _hist, batch=64, mode="fit", att_activation="sigmoid", att_hidden_size=(16, 8), **SMALL)

INIT_CONFIGS = [dict(dnn_dropout=0.5), dict()]


def build_reference_model(ref, spec, l2=0.0):
    import deepctr_torch.inputs as ref_inputs
    import deepctr_torch.models as ref_models
    return ref_models.DIN(G.ref_columns(ref_inputs, spec["dnn_columns"]), spec["history_feature_list"],
                          l2_reg_embedding=l2, device="cpu", **spec["kwargs"])


def synth_inputs(spec, batch, rng):
    """X [B, n_cols] float32 in build_input_features order + labels; one length per row and LENGTH COLUMN"""
    from np_oracle import build_input_features
    fi = build_input_features(spec["dnn_columns"])
    X = np.zeros((batch, max(hi for _, hi in fi.values())), np.float32)
    lens = {}
    for c in spec["dnn_columns"]:
        lo, hi = fi[c["name"]]
        if c["kind"] == "sparse":
            X[:, lo] = rng.integers(0, c["vocab"], batch)
            X[:batch // 8, lo] = X[0, lo]                      # duplicate ids inside the batch
        elif c["kind"] == "dense":
            X[:, lo:hi] = rng.random((batch, hi - lo), dtype=np.float32)
        else:
            T = hi - lo
            if c["length_name"] not in lens:
                n = rng.integers(0, T + 1, batch)
                n[:4] = [0, 1, T - 1, T]
                lens[c["length_name"]] = n
                X[:, fi[c["length_name"]][0]] = n
            ids = rng.integers(1, c["vocab"], (batch, T))
            ids[np.arange(T)[None, :] >= lens[c["length_name"]][:, None]] = 0     # 0 = padding id
            X[:, lo:hi] = ids
    return X, rng.integers(0, 2, batch).astype(np.float32)


def _base(ref, c, train):
    """what run_case stores for one forward / backward, in train or eval mode; -> (out, model, rng)"""
    import torch
    import torch.nn.functional as F
    spec = c["spec"]
    rng = np.random.default_rng(1000 + c["seed"] + sum(map(ord, c["name"])))
    torch.manual_seed(c["seed"])
    model = build_reference_model(ref, spec)
    G.randomise(model, rng)
    if not train:
        with torch.no_grad():
            for k, v in model.state_dict().items():
                if k.endswith("running_mean"):
                    v.copy_(torch.from_numpy(rng.normal(0, 0.3, tuple(v.shape)).astype(np.float32)))
                elif k.endswith("running_var"):
                    v.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, tuple(v.shape)).astype(np.float32)))
    X, y = synth_inputs(spec, c["batch"], rng)
    out = {"spec": np.array(json.dumps(spec)), "X": X, "y": y}
    for k, v in model.state_dict().items():
        out["param/" + k] = v.detach().numpy().copy()
    cap = {}
    hook = model.out.register_forward_pre_hook(lambda m, inp: cap.__setitem__("logit", inp[0].detach().clone()))
    model.train(train)
    y_pred = model(torch.from_numpy(X)).squeeze()
    hook.remove()
    loss = F.binary_cross_entropy(y_pred, torch.from_numpy(y), reduction="sum")
    model.zero_grad()
    loss.backward()
    out["logit"] = cap["logit"].numpy().reshape(-1, 1)
    out["y_pred"] = y_pred.detach().numpy().reshape(-1, 1)
    out["loss"] = np.array(loss.item(), np.float64)
    for k, p in model.named_parameters():
        out["grad/" + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    return out, model, rng


def run_adam(ref, c):
    """default keyword arguments: forward and gradients in train mode from the model's own initial weights scaled up by
    ``randomise``, then 3 steps of the reference's own train step under ``adam``"""
    import torch
    out, model, rng = _base(ref, c, True)
    model.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in out.items() if k.startswith("param/")})
    Xs, ys = zip(*[synth_inputs(c["spec"], c["batch"], rng) for _ in range(3)])
    out["X_steps"], out["y_steps"] = np.stack(Xs), np.stack(ys)
    model.compile("adam", "binary_crossentropy", metrics=[])
    model.train()
    losses = []
    for Xb, yb in zip(Xs, ys):
        yp = model(torch.from_numpy(Xb)).squeeze()
        model.optim.zero_grad()
        ls = model.loss_func(yp, torch.from_numpy(yb), reduction="sum")
        (ls + model.get_regularization_loss() + model.aux_loss).backward()
        model.optim.step()
        losses.append(ls.item())
    out["adam3_loss"] = np.array(losses, np.float64)
    for k, v in model.state_dict().items():
        out["adam3/" + k] = v.detach().numpy().copy()
    return out


def feature_dict(spec, X):
    from np_oracle import build_input_features
    return {n: (X[:, lo] if hi - lo == 1 else X[:, lo:hi]) for n, (lo, hi) in build_input_features(spec["dnn_columns"]).items()}


RELU_MARGIN = 2e-6
FIT_BASE_BATCH = 40         # rows of fit_din's own forward / gradient part: every batch here has 16 to 40 rows
MAX_TRIES = 50


def run_fit(ref, c):
    """``fit()`` is the one run here that goes through hundreds of tower evaluations, and the tower's ReLU has a kink: a
    pre-activation within fp32 rounding of 0 may fall on either side in two implementations, and the whole unit's gradient
    then exists in one and not in the other (seen with seed 0: one unit of one sample in the last batch of the shuffled
    run's first epoch; everything else agreed to 1e-7).  Like the top-k margin of make_ccpm_golden.py: every output of the
    tower's hidden ``nn.Linear`` layers is watched over every call of the three runs, and the fixture is accepted only if
    none is closer to 0 than RELU_MARGIN (20 times the rounding of a 33-term fp32 dot product of O(1) values); otherwise the
    case's seed advances.  ``seed`` and ``min_relu_margin`` are stored."""
    for s in range(c["seed"], c["seed"] + MAX_TRIES):
        out, margin = _run_fit(ref, dict(c, seed=s))
        if margin >= RELU_MARGIN:
            out["seed"] = np.array(s, np.int64)
            out["min_relu_margin"] = np.array(margin, np.float64)
            return out
    raise RuntimeError("fit_din: no seed in %d tries keeps every ReLU input %g away from 0" % (MAX_TRIES, RELU_MARGIN))


def _run_fit(ref, c):
    import torch
    out, model, rng = _base(ref, dict(c, batch=FIT_BASE_BATCH), True)      # (c["batch"] is fit()'s batch_size)
    spec = c["spec"]
    Xf, yf = synth_inputs(spec, G.FIT_ROWS, rng)
    out["fit_X"], out["fit_y"] = Xf, yf
    xin = feature_dict(spec, Xf)
    start = {k[6:]: torch.from_numpy(v) for k, v in out.items() if k.startswith("param/")}
    margin = [float("inf")]

    def watch(mod, inp, res):
        margin[0] = min(margin[0], float(res.detach().abs().min()))
    for tag, opt_name, l2, shuffle in G.FIT_RUNS:
        torch.manual_seed(c["seed"])
        m = build_reference_model(ref, spec, l2=l2)
        m.load_state_dict(start)
        for fc in m.dnn.linears:
            fc.register_forward_hook(watch)
        m.compile(opt_name, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
        torch.manual_seed(G.FIT_SEED)
        hist = m.fit(xin, yf, batch_size=c["batch"], epochs=G.FIT_EPOCHS, verbose=2, validation_split=G.FIT_SPLIT,
                     shuffle=shuffle)
        for k, v in hist.history.items():
            out["fit_%s_hist/%s" % (tag, k)] = np.asarray(v, np.float64)
        out["fit_%s_pred" % tag] = m.predict(xin, batch_size=50)
    return out, margin[0]


def init_fixture():
    """Freshly constructed reference models at their default seed and default regularisation."""
    out, configs = {}, []
    for i, kw in enumerate(INIT_CONFIGS):
        spec = {"model": "DIN", "linear_columns": [], "dnn_columns": _ref, "history_feature_list": _hist, "kwargs": kw}
        configs.append(spec)
        for k, v in build_reference_model(None, spec, l2=1e-6).state_dict().items():
            out["%d/param/%s" % (i, k)] = v.detach().numpy().copy()
    out["configs"] = np.array(json.dumps(configs))
    return out


def main(names=None):
    offline_requests()
    ref = G.import_reference()
    G.build_reference_model, G.synth_inputs = build_reference_model, synth_inputs
    os.makedirs(OUT_DIR, exist_ok=True)
    for c in CASES:
        if names and c["name"] not in names:
            continue
        if c["mode"] == "eval":
            data = _base(ref, c, False)[0]
        elif c["mode"] == "adam":
            data = run_adam(ref, c)
        elif c["mode"] == "fit":
            data = run_fit(ref, c)
        else:
            data = G.run_case(ref, c)
        path = os.path.join(OUT_DIR, c["name"] + ".npz")
        np.savez_compressed(path, **data)
        print("%-20s B=%-3d logit[min,max]=[%+.3f,%+.3f] loss=%.4f  -> %s (%.0f KB)" % (
            c["name"], c["batch"], data["logit"].min(), data["logit"].max(), float(data["loss"]),
            os.path.relpath(path), os.path.getsize(path) / 1024))
    if not names or "init" in names:
        path = os.path.join(OUT_DIR, "init.npz")
        np.savez_compressed(path, **init_fixture())
        print("init -> %s (%.0f KB)" % (os.path.relpath(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main(sys.argv[1:] or None)
