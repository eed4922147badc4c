"""What the MLR suites share (tests/test_mlr_host.py, test_gpu_mlr_kernel.py, test_gpu_mlr_models.py): the fixtures of
tests/golden/mlr (tools/golden/make_mlr_golden.py), spec -> model, the bars, and the mixture's formulas (include/dctr.h,
dctr_mlr_fwd / _bwd) in numpy at a chosen precision."""
import json
import os

import numpy as np

from helpers import GOLDEN_DIR, feature_columns, load_golden

Y_TOL, GRAD_TOL, TRAJ_TOL = 1e-5, 2e-5, 2e-5
FORWARD = ["mlr_bias", "mlr_criteo", "mlr_two", "mlr_dense_only", "mlr_r8", "mlr_mixed", "mlr_regression", "mlr_base",
           "lazy_mlr", "fit_mlr"]
STEPS = ["mlr_criteo", "mlr_mixed", "mlr_regression", "mlr_base"]
FIT_RUNS = (("plain", "adagrad", 0.0, False), ("shuffled", "adagrad", 0.0, True), ("default", "adam", 1e-5, True))


def load(name):
    return load_golden("mlr/" + name)


def build(spec, device, **over):
    from deepctr_torch.models import MLR
    conv = lambda cols: None if cols is None else feature_columns(cols)      # noqa: E731
    kw = dict(spec["kwargs"])
    kw.update(over)
    return MLR(conv(spec["region_columns"]), conv(spec["base_columns"]), conv(spec["bias_columns"]), device=device, **kw)


def loaded(name, device, **over):
    import torch
    g = load(name)
    m = build(g["spec"], device, **over)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    return g, m


def loss_name(spec):
    return "binary_crossentropy" if spec["kwargs"].get("task", "binary") == "binary" else "mse"


def loss_sum(spec, y_pred, y):
    import torch.nn.functional as F
    fn = F.binary_cross_entropy if loss_name(spec) == "binary_crossentropy" else F.mse_loss
    return fn(y_pred, y, reduction="sum")


def grad_scale(key, ref):
    """The gradient bound's scale: max|g_ref| of the parameter.  The floor of 1 the other model suites use is NOT applied to
    the region and bias sides (their gradients are 0.04 .. 1 in these fixtures: a floor would hide them), as for ONN's pair
    tables."""
    top = float(np.max(np.abs(ref))) if ref.size else 0.0
    return top if key.startswith(("region_linear_model.", "bias_model.")) else max(1.0, top)


def init_configs():
    path = os.path.join(GOLDEN_DIR, "mlr", "init.npz")
    if not os.path.exists(path):
        return []
    z = np.load(path, allow_pickle=False)
    out = []
    for i, spec in enumerate(json.loads(str(z["configs"]))):
        pre = "%d/param/" % i
        out.append((spec, {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}))
    return out


def fit_inputs(model, X):
    """one array per feature of ``model.feature_index`` (what ``fit`` / ``predict`` take as a dict)"""
    return {n: X[:, lo:hi] for n, (lo, hi) in model.feature_index.items()}


# ---- the mixture (include/dctr.h) ------------------------------------------------------------------------------------
def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def mixture(Z, R, has_bias, binary, dtype=np.float64):
    """(y [B], dy/dz [B, H]) of the mixture over the head logits ``Z [B, H]``, every operation in ``dtype``"""
    Z = np.asarray(Z, dtype)
    zr = Z[:, :R]
    e = np.exp(zr - zr.max(axis=1, keepdims=True))
    s = e / e.sum(axis=1, keepdims=True)
    l = sigmoid(zr) if binary else zr
    p0 = (s * l).sum(axis=1, keepdims=True)
    c = sigmoid(Z[:, R:R + 1]) if has_bias else np.ones_like(p0)
    dl = l * (1 - l) if binary else np.ones_like(l)
    dz = np.zeros_like(Z)
    dz[:, :R] = c * (s * (l - p0) + s * dl)
    if has_bias:
        dz[:, R:R + 1] = p0 * c * (1 - c)
    return (p0 * c)[:, 0].astype(dtype), dz.astype(dtype)

