"""Generate tests/golden/onn/*.npz by EXECUTING THE REFERENCE's ONN (torch-CPU fp32).

Like tools/golden/make_iafm_golden.py: a sub-directory of its own (the suites that parametrise over ``tests/golden/*.npz``
check every fixture against the numpy oracle, which does not model the pair lookup), and everything that drives the
reference imported from oracle/make_golden.py (the TensorFlow stub, the column builders, ``run_case`` unchanged): a fixture
here holds exactly what a fixture there holds.  ``randomise`` reaches the pair tables because their keys contain
``embedding_dict``: emb1 and emb2 are both N(0, 0.15).

    python tools/golden/make_onn_golden.py            # rewrites every fixture (deterministic)

``init.npz`` holds the freshly constructed ``state_dict`` of the reference's own ONN test configuration
(tests/models/ONN_test.py: 2 sparse + 2 dense columns, embedding size 4, hidden (32, 32), dnn_dropout 0.5) at the default
seed and default regularisation, plus a 3-sparse variant: ``configs`` (json list of specs) and ``<i>/param/<key>``.
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

OUT_DIR = os.path.join(ROOT, "tests", "golden", "onn")

CASES = []


def case(name, lin, dnn, batch=64, seed=0, steps=False, lazy=False, fit=False, **kwargs):
    CASES.append({"name": name, "batch": batch, "seed": seed, "steps": steps, "lazy": lazy, "fit": fit,
                  "spec": {"model": "ONN", "linear_columns": lin, "dnn_columns": dnn, "kwargs": kwargs}})


_t = G.criteo_columns(2, 2, 7, 4)
case("onn_two", _t, _t, batch=33, steps=True, dnn_hidden_units=(8,))
_d = G.criteo_columns(3, 1, 11, 6)
case("onn_d6", _d, _d, batch=20, dnn_hidden_units=(16, 8))
_c = G.criteo_columns(9, 4, 22, 8)
case("onn_criteo", _c, _c, batch=40, steps=True, dnn_hidden_units=(32, 16))
_m = G.mixed_columns()
case("onn_mixed", _m, _m, batch=33, dnn_hidden_units=(16,))
_o = G.criteo_columns(1, 2, 9, 4)
case("onn_one_sparse", _o, _o, batch=17, dnn_hidden_units=(8,))
_s = G.criteo_columns(5, 2, 12, 6)
case("onn_nolinear", [], _s, batch=20, dnn_hidden_units=(8,))
_b = G.criteo_columns(4, 2, 10, 8)
case("onn_bn", _b, _b, batch=24, dnn_use_bn=True, dnn_hidden_units=(16, 8))
_l = G.criteo_columns(8, 3, 20, 8)
case("lazy_onn", _l, _l, batch=24, lazy=True, dnn_hidden_units=(16, 8))
case("fit_onn", _l, _l, batch=64, fit=True, dnn_hidden_units=(16, 8))

INIT_CONFIGS = [(2, dict(dnn_hidden_units=(32, 32), dnn_dropout=0.5)),
                (3, dict(dnn_hidden_units=(8,), init_std=0.01))]


def init_fixture():
    """Freshly constructed reference models at their default seed and default regularisation."""
    import deepctr_torch.inputs as ref_inputs
    import deepctr_torch.models as ref_models
    out, configs = {}, []
    for i, (n, kw) in enumerate(INIT_CONFIGS):
        cols = G.criteo_columns(n, n, 7, 4)
        spec = {"model": "ONN", "linear_columns": cols, "dnn_columns": cols, "kwargs": kw}
        configs.append(spec)
        fc = G.ref_columns(ref_inputs, cols)
        m = ref_models.ONN(fc, fc, device="cpu", **kw)
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
        data = G.run_case(ref, c)
        path = os.path.join(OUT_DIR, c["name"] + ".npz")
        np.savez_compressed(path, **data)
        print("%-24s B=%-3d logit[min,max]=[%+.3f,%+.3f] loss=%.4f  -> %s (%.0f KB)" % (
            c["name"], c["batch"], data["logit"].min(), data["logit"].max(), float(data["loss"]),
            os.path.relpath(path), os.path.getsize(path) / 1024))
    if not names or "init" in names:
        path = os.path.join(OUT_DIR, "init.npz")
        np.savez_compressed(path, **init_fixture())
        print("init -> %s (%.0f KB)" % (os.path.relpath(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main(sys.argv[1:] or None)
