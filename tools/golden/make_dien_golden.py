"""Generate tests/golden/dien/*.npz by EXECUTING THE REFERENCE's DIEN (torch-CPU fp32).

Like tools/golden/make_din_golden.py: a sub-directory of its own, and what drives the reference is imported from
oracle/make_golden.py unchanged (the TensorFlow stub, the column builders, ``randomise``, the fit constants); the input
generator is make_din_golden.py's (one length per row and length column, the rows 0..3 of every batch with the lengths
0, 1, T - 1 and T, padding id 0, duplicate ids inside the batch).  The negative history columns draw ids of their own.

    python tools/golden/make_dien_golden.py            # rewrites every fixture (deterministic)

A fixture holds what a fixture of oracle/make_golden.py holds, with two differences: ``aux_loss`` is stored, and the
gradients are those of ``BCE(sum) + aux_loss`` (the reference's own training objective without the regularisation term),
so that the auxiliary net has gradients under negative sampling.  ``steps``: 3 steps of sgd / adagrad / adagradp as
there.  ``dien_default_adam``: default keyword arguments, 3 steps of ``adam``.  ``fit_dien``: ``fit()`` History and
``predict()``.  ``init.npz``: freshly constructed ``state_dict``s of the eight (gru_type, use_negsampling) variants at the
reference test's configuration and of one default construction: ``configs`` (json list of specs), ``<i>/param/<key>``.

Kinks: DIEN's tower and, by default, its attention net are ReLU nets.  A pre-activation within fp32 rounding of 0 may fall
on either side in two implementations, and the unit's gradient then exists in one and not in the other.  Every output of
the hidden ``nn.Linear`` layers of the tower and of a relu attention net is watched over every call a fixture makes, and
the fixture is accepted only when none is closer to 0 than RELU_MARGIN; otherwise the case's seed advances.  ``seed`` and
``min_relu_margin`` are stored.
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
from make_din_golden import LEN, feature_dict, synth_inputs  # noqa: E402
from make_iafm_golden import offline_requests  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "dien")
RELU_MARGIN = 2e-6
MAX_TRIES = 200
FIT_BASE_BATCH = 40

CASES = []


def case(name, dnn, hist, batch=24, seed=0, steps=False, mode=None, **kwargs):
    CASES.append({"name": name, "batch": batch, "seed": seed, "steps": steps, "mode": mode,
                  "spec": {"model": "DIEN", "linear_columns": [], "dnn_columns": dnn, "history_feature_list": hist,
                           "kwargs": kwargs}})


def behaviour_columns(feats, T, others=(), dense=0, first=(), neg=False):
    """``feats``: (name, vocab, dim) of the candidate features; each gets ``hist_<name>`` (and ``neg_hist_<name>``) of T
    positions over the same table.  ``first``: VarLen columns declared in front of everything else."""
    cols = list(first) + [G.sparse(n, v, d) for n, v, d in others] + [G.sparse(n, v, d) for n, v, d in feats]
    cols += [G.dense("d%d" % i) for i in range(dense)]
    for prefix in ["hist_"] + (["neg_hist_"] if neg else []):
        cols += [G.varlen(prefix + n, v, d, T, "mean", length_name=LEN, embedding_name=n) for n, v, d in feats]
    return cols


# the reference's own test (tests/models/DIEN_test.py): user / gender of 4, item of 8, category of 4, one dense, T = 4
_feats, _others, _hist = [("item_id", 9, 8), ("cate_id", 6, 4)], [("user", 7, 4), ("gender", 2, 4)], ["item_id", "cate_id"]
_ref = behaviour_columns(_feats, 4, others=_others, dense=1)
_ref_neg = behaviour_columns(_feats, 4, others=_others, dense=1, neg=True)
SMALL = dict(dnn_hidden_units=(32, 16))
NEG = dict(use_negsampling=True, alpha=0.5)
# (the two with 3-step trajectories score without the softmax.  A softmax ignores a shift of all of a sample's scores, so
# the exact gradient of dense.bias -- and of the bias of every attention unit that is active at every position -- is 0; an
# Adagrad step from a zero accumulator is lr * sign(g), and the sign of rounding noise is not a property of the model)
case("dien_gru", _ref, _hist, batch=24, steps=True, gru_type="GRU", att_weight_normalization=False, **SMALL)
case("dien_aigru", _ref, _hist, batch=33, gru_type="AIGRU", **SMALL)
case("dien_agru", _ref, _hist, batch=16, gru_type="AGRU", **SMALL)
case("dien_augru", _ref, _hist, batch=40, steps=True, gru_type="AUGRU", att_weight_normalization=False, **SMALL)
case("dien_gru_neg", _ref_neg, _hist, batch=24, gru_type="GRU", **dict(SMALL, **NEG))
case("dien_aigru_neg", _ref_neg, _hist, batch=20, gru_type="AIGRU", **dict(SMALL, **NEG))
case("dien_agru_neg", _ref_neg, _hist, batch=28, gru_type="AGRU", **dict(SMALL, **NEG))
case("dien_augru_neg", _ref_neg, _hist, batch=24, gru_type="AUGRU", **dict(SMALL, **NEG))
case("dien_one", behaviour_columns([("item", 11, 6)], 5, neg=True), ["item"], batch=20, gru_type="AGRU",
     att_hidden_units=(16, 8), **dict(SMALL, **NEG))
case("dien_t50", behaviour_columns([("item", 40, 16), ("cate", 12, 16)], 50, others=[("user", 9, 8)]), ["item", "cate"],
     batch=16, gru_type="AUGRU", att_hidden_units=(16, 8), **SMALL)
# a pooled VarLen column with a length column of its own, declared FIRST: the reference reads the lengths from the
# first length_name among ALL VarLen columns, i.e. from this one, and ignores the column itself
_tags = [G.varlen("tags", 8, 4, 3, "mean", length_name="tags_length")]
case("dien_extra_varlen", behaviour_columns([("item", 9, 8), ("cate", 6, 4)], 4, others=[("user", 7, 4)], dense=1,
                                            first=_tags),
     ["item", "cate"], batch=24, gru_type="GRU", att_hidden_units=(16, 8), **SMALL)
case("dien_nosoftmax_sigmoid", _ref, _hist, batch=24, gru_type="AUGRU", att_weight_normalization=False,
     att_activation="sigmoid", **SMALL)
case("dien_default_adam", _ref, _hist, batch=32, mode="adam")
# (sigmoid scores without the softmax: fit() makes hundreds of evaluations, and a relu attention net would put a million
# more values under the kink rule; under a softmax the first attention layer's bias gradient is a sum that all but
# cancels, 3.6e-6 against terms of 7e-5, so the reference's own float32 value is mostly rounding)
case("fit_dien", _ref_neg, _hist, batch=64, mode="fit", gru_type="AUGRU", att_activation="sigmoid",
     att_weight_normalization=False, att_hidden_units=(16, 8), **dict(SMALL, **NEG))

INIT_CONFIGS = [dict(gru_type=g, use_negsampling=n, dnn_hidden_units=[4, 4, 4], dnn_dropout=0.5)
                for g in ("GRU", "AIGRU", "AGRU", "AUGRU") for n in (False, True)] + [dict()]


def build_reference_model(ref, spec, l2=0.0):
    import deepctr_torch.inputs as ref_inputs
    import deepctr_torch.models as ref_models
    return ref_models.DIEN(G.ref_columns(ref_inputs, spec["dnn_columns"]), spec["history_feature_list"],
                           l2_reg_embedding=l2, device="cpu", **spec["kwargs"])


class Watch(object):
    """the smallest |input| any watched ReLU has seen"""

    def __init__(self):
        self.margin = float("inf")

    def attach(self, model):
        import torch
        nets = [model.dnn]
        att = model.interest_evolution.attention.local_att.dnn
        if all(isinstance(a, torch.nn.ReLU) for a in att.activation_layers):
            nets.append(att)
        for net in nets:
            if all(isinstance(a, torch.nn.ReLU) for a in net.activation_layers):
                for fc in net.linears:
                    fc.register_forward_hook(self)

    def __call__(self, mod, inp, res):
        if res.numel():
            self.margin = min(self.margin, float(res.detach().abs().min()))


def _base(ref, c, watch):
    """forward, BCE(sum), auxiliary loss and the gradients of their sum in train mode; -> (out, model, rng)"""
    import torch
    import torch.nn.functional as F
    spec = c["spec"]
    rng = np.random.default_rng(1000 + c["seed"] + sum(map(ord, c["name"])))
    torch.manual_seed(c["seed"])
    model = build_reference_model(ref, spec)
    G.randomise(model, rng)
    watch.attach(model)
    X, y = synth_inputs(spec, c["batch"], rng)
    out = {"spec": np.array(json.dumps(spec)), "X": X, "y": y}
    for k, v in model.state_dict().items():
        out["param/" + k] = v.detach().numpy().copy()
    cap = {}
    hook = model.out.register_forward_pre_hook(lambda m, inp: cap.__setitem__("logit", inp[0].detach().clone()))
    model.train()
    y_pred = model(torch.from_numpy(X)).squeeze()
    hook.remove()
    loss = F.binary_cross_entropy(y_pred, torch.from_numpy(y), reduction="sum")
    model.zero_grad()
    (loss + model.aux_loss).sum().backward()
    out["logit"] = cap["logit"].numpy().reshape(-1, 1)
    out["y_pred"] = y_pred.detach().numpy().reshape(-1, 1)
    out["loss"] = np.array(loss.item(), np.float64)
    out["aux_loss"] = model.aux_loss.detach().numpy().reshape(1).astype(np.float64)
    for k, p in model.named_parameters():
        out["grad/" + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()
    return out, model, rng


def _steps(model, names, Xs, ys, out):
    """3 steps of the reference's own train step (basemodel.py:242-262) per optimizer name, from the same start"""
    import torch
    start = {k: v.clone() for k, v in model.state_dict().items()}
    for opt_name in names:
        model.load_state_dict(start)
        model.compile("adagrad" if opt_name == "adagradp" else opt_name, "binary_crossentropy", metrics=[])
        if opt_name == "adagradp":
            for grp in model.optim.param_groups:
                for p in grp["params"]:
                    model.optim.state[p]["sum"].fill_(G.ADAGRAD_SUM0)
        model.train()
        losses = []
        for Xb, yb in zip(Xs, ys):
            yp = model(torch.from_numpy(Xb)).squeeze()
            model.optim.zero_grad()
            ls = model.loss_func(yp, torch.from_numpy(yb), reduction="sum")
            (ls + model.get_regularization_loss() + model.aux_loss).sum().backward()
            model.optim.step()
            losses.append(ls.item())
        out[opt_name + "3_loss"] = np.array(losses, np.float64)
        for k, v in model.state_dict().items():
            out[opt_name + "3/" + k] = v.detach().numpy().copy()


def _run(ref, c):
    import torch
    watch = Watch()
    spec = c["spec"]
    out, model, rng = _base(ref, dict(c, batch=FIT_BASE_BATCH) if c["mode"] == "fit" else c, watch)
    if c["steps"] or c["mode"] == "adam":
        Xs, ys = zip(*[synth_inputs(spec, c["batch"], rng) for _ in range(3)])
        out["X_steps"], out["y_steps"] = np.stack(Xs), np.stack(ys)
        _steps(model, ("adam",) if c["mode"] == "adam" else ("sgd", "adagrad", "adagradp"), Xs, ys, out)
    if c["mode"] == "fit":
        Xf, yf = synth_inputs(spec, G.FIT_ROWS, rng)
        out["fit_X"], out["fit_y"] = Xf, yf
        xin = feature_dict(spec, Xf)
        start = {k[6:]: torch.from_numpy(v) for k, v in out.items() if k.startswith("param/")}
        for tag, opt_name, l2, shuffle in G.FIT_RUNS:
            torch.manual_seed(c["seed"])
            m = build_reference_model(ref, spec, l2=l2)
            m.load_state_dict(start)
            watch.attach(m)
            m.compile(opt_name, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
            torch.manual_seed(G.FIT_SEED)
            hist = m.fit(xin, yf, batch_size=c["batch"], epochs=G.FIT_EPOCHS, verbose=2,
                         validation_split=G.FIT_SPLIT, shuffle=shuffle)
            for k, v in hist.history.items():
                out["fit_%s_hist/%s" % (tag, k)] = np.asarray(v, np.float64)
            out["fit_%s_pred" % tag] = m.predict(xin, batch_size=50)
    return out, watch.margin


def run(ref, c):
    for s in range(c["seed"], c["seed"] + MAX_TRIES):
        out, margin = _run(ref, dict(c, seed=s))
        if margin >= RELU_MARGIN:
            out["seed"] = np.array(s, np.int64)
            out["min_relu_margin"] = np.array(margin, np.float64)
            return out
    raise RuntimeError("%s: no seed in %d tries keeps every ReLU input %g away from 0" % (c["name"], MAX_TRIES,
                                                                                         RELU_MARGIN))


def init_fixture():
    """Freshly constructed reference models at their default seed and default regularisation."""
    out, configs = {}, []
    for i, kw in enumerate(INIT_CONFIGS):
        cols = _ref_neg if kw.get("use_negsampling") else _ref
        spec = {"model": "DIEN", "linear_columns": [], "dnn_columns": cols, "history_feature_list": _hist, "kwargs": kw}
        configs.append(spec)
        for k, v in build_reference_model(None, spec, l2=1e-6).state_dict().items():
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
        data = run(ref, c)
        path = os.path.join(OUT_DIR, c["name"] + ".npz")
        np.savez_compressed(path, **data)
        print("%-24s B=%-3d seed=%-3d margin=%.2e logit[min,max]=[%+.3f,%+.3f] loss=%.4f aux=%.4f -> %s (%.0f KB)" % (
            c["name"], c["batch"], int(data["seed"]), float(data["min_relu_margin"]), data["logit"].min(),
            data["logit"].max(), float(data["loss"]), float(data["aux_loss"][0]), os.path.relpath(path),
            os.path.getsize(path) / 1024))
    if not names or "init" in names:
        path = os.path.join(OUT_DIR, "init.npz")
        np.savez_compressed(path, **init_fixture())
        print("init -> %s (%.0f KB)" % (os.path.relpath(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main(sys.argv[1:] or None)
