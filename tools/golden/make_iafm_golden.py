"""Generate tests/golden/iafm/*.npz by EXECUTING THE REFERENCE's IFM and DIFM (torch-CPU fp32).

The fixtures of the other model families come from oracle/make_golden.py; these live in a sub-directory of their own
because the suites that parametrise over ``tests/golden/*.npz`` check every fixture against the numpy oracle, which does not
model the input-aware factor.  Everything that drives the reference is imported from oracle/make_golden.py (the TensorFlow
stub, the column builders, ``run_case``): a fixture here holds exactly what a fixture there holds.

    python tools/golden/make_iafm_golden.py            # rewrites every fixture (deterministic)

``init.npz`` holds, for the six configurations of the reference's own IFM / DIFM tests (1-3 sparse and as many dense
columns, their hidden sizes and head counts, dnn_dropout=0.5), the freshly constructed ``state_dict`` at the default seed:
``configs`` (json list of specs) and ``<i>/param/<key>``.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import make_golden as G  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "iafm")

CASES = []


def case(name, model, lin, dnn, batch=64, seed=0, steps=False, lazy=False, fit=False, **kwargs):
    CASES.append({"name": name, "batch": batch, "seed": seed, "steps": steps, "lazy": lazy, "fit": fit,
                  "spec": {"model": model, "linear_columns": lin, "dnn_columns": dnn, "kwargs": kwargs}})


_c = G.criteo_columns(9, 4, 22, 8)
case("ifm_criteo", "IFM", _c, _c, batch=40, steps=True, dnn_hidden_units=(32, 16))
_m = G.mixed_columns()
case("ifm_mixed", "IFM", _m, _m, batch=33, steps=True, dnn_hidden_units=(16,))
_w = G.criteo_columns(26, 13, 48, 16)
case("ifm_wide26", "IFM", _w, _w, batch=96, dnn_hidden_units=(64, 32))
_o = G.criteo_columns(1, 1, 15, 8)
case("ifm_one_field", "IFM", _o, _o, batch=17, dnn_hidden_units=(8,))
_s = G.criteo_columns(5, 2, 12, 6)
case("ifm_nolinear", "IFM", [], _s, batch=20, dnn_hidden_units=(8,))
case("ifm_dense_linear_only", "IFM", [c for c in _s if c["kind"] == "dense"], _s, batch=20, dnn_hidden_units=(8,))
_d = G.criteo_columns(7, 3, 20, 8)
case("difm_criteo", "DIFM", _d, _d, batch=40, steps=True, att_head_num=2, dnn_hidden_units=(32, 16))
case("difm_nores", "DIFM", _d, _d, batch=24, att_head_num=4, att_res=False, dnn_hidden_units=(16,))
case("difm_mixed", "DIFM", _m, _m, batch=33, att_head_num=2, dnn_hidden_units=(16,))
case("difm_d6", "DIFM", _s, _s, batch=20, att_head_num=3, dnn_hidden_units=(8,))
case("difm_one_field", "DIFM", _o, _o, batch=17, att_head_num=1, dnn_hidden_units=(4,))
_l = G.criteo_columns(8, 3, 20, 8)
case("lazy_ifm", "IFM", _l, _l, batch=24, lazy=True, dnn_hidden_units=(16, 8))
case("lazy_difm", "DIFM", _l, _l, batch=24, lazy=True, att_head_num=2, dnn_hidden_units=(16, 8))
case("fit_ifm", "IFM", _l, _l, batch=64, fit=True, dnn_hidden_units=(16, 8))
case("fit_difm", "DIFM", _l, _l, batch=64, fit=True, att_head_num=2, dnn_hidden_units=(16, 8))

# the reference's own model tests (tests/models/IFM_test.py, DIFM_test.py): embedding size 4, n sparse + n dense columns
INIT_CONFIGS = [("IFM", 3, dict(dnn_hidden_units=(32,), dnn_dropout=0.5)),
                ("IFM", 2, dict(dnn_hidden_units=(32,), dnn_dropout=0.5)),
                ("IFM", 1, dict(dnn_hidden_units=(32,), dnn_dropout=0.5)),
                ("DIFM", 2, dict(att_head_num=1, dnn_hidden_units=(4,), dnn_dropout=0.5)),
                ("DIFM", 2, dict(att_head_num=2, dnn_hidden_units=(4, 4), dnn_dropout=0.5)),
                ("DIFM", 1, dict(att_head_num=1, dnn_hidden_units=(4,), dnn_dropout=0.5))]


def init_fixture():
    """Freshly constructed reference models at their default seed and default regularisation."""
    import deepctr_torch.inputs as ref_inputs
    import deepctr_torch.models as ref_models
    out, configs = {}, []
    for i, (model, n, kw) in enumerate(INIT_CONFIGS):
        cols = G.criteo_columns(n, n, 7, 4)
        spec = {"model": model, "linear_columns": cols, "dnn_columns": cols, "kwargs": kw}
        configs.append(spec)
        fc = G.ref_columns(ref_inputs, cols)
        m = getattr(ref_models, model)(fc, fc, device="cpu", **kw)
        for k, v in m.state_dict().items():
            out["%d/param/%s" % (i, k)] = v.detach().numpy().copy()
    out["configs"] = np.array(json.dumps(configs))
    return out


def offline_requests():
    """Importing the reference starts a thread that asks a package index for the latest release.  A stand-in ``requests``
    whose ``get`` raises keeps the generator off the network: the reference catches the error and prints a hint."""
    mod = types.ModuleType("requests")

    def get(*args, **kwargs):
        raise OSError("offline")
    mod.get = get
    mod.codes = types.SimpleNamespace(ok=200)
    sys.modules["requests"] = mod


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
