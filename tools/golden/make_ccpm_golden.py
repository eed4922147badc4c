"""Generate tests/golden/ccpm/*.npz by EXECUTING THE REFERENCE's CCPM (torch-CPU fp32).

Like tools/golden/make_onn_golden.py: a sub-directory of its own, and everything that drives the reference imported from
oracle/make_golden.py (the TensorFlow stub, the column builders, ``run_case`` unchanged): a fixture here holds exactly what a
fixture there holds, plus ``seed`` and ``min_topk_gap``.

    python tools/golden/make_ccpm_golden.py            # rewrites every fixture (deterministic)

TIE MARGIN.  k-max pooling is discontinuous in its gradient: two activations of one column that differ by less than the
rounding difference between two implementations can swap places, and the gradient is then routed to another element.  A
fixture on which that can happen tests nothing, so while ``run_case`` runs, the reference's ``KMaxPooling.forward`` is
wrapped to record the smallest difference between neighbours among the top ``k + 1`` sorted values of any column, over
every call (the forward, the 3-step runs, the lazy runs, ``fit`` / ``predict``).  A fixture is accepted only if that gap is
at least ``MIN_GAP``; otherwise the case's ``seed`` advances (at most ``MAX_TRIES`` tries).  ``MIN_GAP`` is 8 times the
largest |pooled value - fp64| tests/test_gpu_ccpm_kernel.py prints, or more (DESIGN.md quotes both numbers).

``init.npz`` holds the freshly constructed ``state_dict`` of the reference's own CCPM test configuration
(tests/models/CCPM_test.py: widths (3, 2), filters (2, 1), hidden [32], dnn_dropout 0.5) and of one 26-field model with
default keyword arguments: ``configs`` (json list of specs) and ``<i>/param/<key>``.
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

OUT_DIR = os.path.join(ROOT, "tests", "golden", "ccpm")
MIN_GAP = 4e-6
MAX_TRIES = 300

CASES = []


def case(name, lin, dnn, batch=64, seed=0, steps=False, lazy=False, fit=False, **kwargs):
    CASES.append({"name": name, "batch": batch, "seed": seed, "steps": steps, "lazy": lazy, "fit": fit,
                  "spec": {"model": "CCPM", "linear_columns": lin, "dnn_columns": dnn, "kwargs": kwargs}})


def _sparse_only(cols):
    return [c for c in cols if c["kind"] != "dense"]


_t = G.criteo_columns(2, 0, 7, 4)
case("ccpm_two", _t, _t, batch=33, steps=True, conv_kernel_width=(3, 2), conv_filters=(2, 1), dnn_hidden_units=(8,))
_h = G.criteo_columns(3, 0, 9, 4)
case("ccpm_three", _h, _h, batch=20, conv_kernel_width=(3, 2), conv_filters=(2, 1), dnn_hidden_units=(8,))
_c = G.criteo_columns(9, 4, 22, 8)
case("ccpm_criteo", _c, _sparse_only(_c), batch=40, steps=True, conv_kernel_width=(6, 5), conv_filters=(4, 4),
     dnn_hidden_units=(32, 16))
_f = G.criteo_columns(26, 0, 48, 16)
case("ccpm_f26", _f, _f, batch=16, conv_kernel_width=(6, 5), conv_filters=(4, 4), dnn_hidden_units=(32,))
_m = G.mixed_columns()
case("ccpm_mixed", _m, _sparse_only(_m), batch=33, conv_kernel_width=(3, 2), conv_filters=(3, 2), dnn_hidden_units=(16,))
_o = G.criteo_columns(6, 2, 11, 6)
case("ccpm_one_layer", _o, _sparse_only(_o), batch=24, conv_kernel_width=(4,), conv_filters=(3,), dnn_hidden_units=(16, 8))
_l3 = G.criteo_columns(9, 0, 13, 4)
case("ccpm_three_layers", _l3, _l3, batch=24, conv_kernel_width=(3, 3, 2), conv_filters=(3, 2, 2), dnn_hidden_units=(16,))
_s = G.criteo_columns(5, 0, 12, 6)
case("ccpm_nolinear", [], _s, batch=20, conv_kernel_width=(3, 2), conv_filters=(2, 2), dnn_hidden_units=(8,))
_b = G.criteo_columns(4, 0, 10, 8)
case("ccpm_bn", _b, _b, batch=24, dnn_use_bn=True, conv_kernel_width=(3, 2), conv_filters=(2, 2), dnn_hidden_units=(16, 8))
_z = G.criteo_columns(5, 0, 20, 8)
case("lazy_ccpm", _z, _z, batch=24, lazy=True, conv_kernel_width=(2, 2), conv_filters=(2, 2), dnn_hidden_units=(16, 8))
_q = G.criteo_columns(4, 0, 20, 8)
case("fit_ccpm", _q, _q, batch=64, fit=True, conv_kernel_width=(2, 1), conv_filters=(2, 2), dnn_hidden_units=(16, 8))

INIT_CONFIGS = [(2, 4, dict(conv_kernel_width=(3, 2), conv_filters=(2, 1), dnn_hidden_units=[32], dnn_dropout=0.5)),
                (26, 16, dict())]


class GapRecorder(object):
    """Wraps the imported reference's ``KMaxPooling.forward``; ``gap`` is the smallest neighbour difference among the top
    ``k + 1`` sorted values of any column seen since ``reset()``."""

    def __init__(self):
        import torch
        import deepctr_torch.layers.sequence as ref_sequence
        self.gap = float("inf")
        cls = ref_sequence.KMaxPooling
        inner = cls.forward
        rec = self

        def forward(mod, inputs):
            n = inputs.shape[mod.axis]
            if n > 1:
                top = torch.topk(inputs.detach().double(), k=min(mod.k + 1, n), dim=mod.axis, sorted=True)[0]
                lo = top.narrow(mod.axis, 1, top.shape[mod.axis] - 1)
                hi = top.narrow(mod.axis, 0, top.shape[mod.axis] - 1)
                rec.gap = min(rec.gap, float((hi - lo).min()))
            return inner(mod, inputs)
        cls.forward = forward

    def reset(self):
        self.gap = float("inf")


def run_with_margin(ref, rec, c):
    """``run_case`` at the first seed from the case's own on whose run no top-k decision is closer than MIN_GAP."""
    for s in range(c["seed"], c["seed"] + MAX_TRIES):
        cs = dict(c, seed=s)
        rec.reset()
        data = G.run_case(ref, cs)
        if rec.gap >= MIN_GAP:
            data["seed"] = np.array(s, np.int64)
            data["min_topk_gap"] = np.array(rec.gap, np.float64)
            return data
    raise RuntimeError("%s: no seed in %d tries reaches a top-k gap of %g" % (c["name"], MAX_TRIES, MIN_GAP))


def init_fixture():
    """Freshly constructed reference models at their default seed and default regularisation."""
    import deepctr_torch.inputs as ref_inputs
    import deepctr_torch.models as ref_models
    out, configs = {}, []
    for i, (n, dim, kw) in enumerate(INIT_CONFIGS):
        cols = G.criteo_columns(n, 0, 7, dim)
        spec = {"model": "CCPM", "linear_columns": cols, "dnn_columns": cols, "kwargs": kw}
        configs.append(spec)
        fc = G.ref_columns(ref_inputs, cols)
        m = ref_models.CCPM(fc, fc, device="cpu", **kw)
        for k, v in m.state_dict().items():
            out["%d/param/%s" % (i, k)] = v.detach().numpy().copy()
    out["configs"] = np.array(json.dumps(configs))
    return out


def main(names=None):
    offline_requests()
    ref = G.import_reference()
    rec = GapRecorder()
    os.makedirs(OUT_DIR, exist_ok=True)
    for c in CASES:
        if names and c["name"] not in names:
            continue
        data = run_with_margin(ref, rec, c)
        path = os.path.join(OUT_DIR, c["name"] + ".npz")
        np.savez_compressed(path, **data)
        print("%-20s B=%-3d seed=%-3d gap=%.2e logit[min,max]=[%+.3f,%+.3f] loss=%.4f  -> %s (%.0f KB)" % (
            c["name"], c["batch"], int(data["seed"]), float(data["min_topk_gap"]), data["logit"].min(),
            data["logit"].max(), float(data["loss"]), os.path.relpath(path), os.path.getsize(path) / 1024))
    if not names or "init" in names:
        path = os.path.join(OUT_DIR, "init.npz")
        np.savez_compressed(path, **init_fixture())
        print("init -> %s (%.0f KB)" % (os.path.relpath(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main(sys.argv[1:] or None)
