#!/usr/bin/env python
"""Train-step time of the other BASELINE.json configurations (parity-test cases, not bench lines): xDeepFM
(CIN [128,128]), FiBiNET (bilinear 'interaction' + SENET), DCN, PNN, ... at the Criteo shape, batch 4096.  Default: Adagrad,
l2 = 0 (the numbers of earlier rounds).  ``--optimizer adam|rmsprop|sgd|adagrad`` compiles with that string;
``--reference-defaults`` keeps every model's own default L2 kwargs (the reference's ``l2_reg_* = 1e-5``) instead of 0.
Eager steps and hipGraph replays (two steps per graph) -- the replay only where ``_graph_safe_step()`` allows it, as in
``fit()``; ``--blocks N`` times N blocks of each and reports the median and the spread (max - min).
    python tools/bench_models.py [MODEL,MODEL...] [--optimizer adam] [--reference-defaults] > models.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deepctr-torch_amd"))
import torch  # noqa: E402

from deepctr_torch.inputs import DenseFeat, SparseFeat  # noqa: E402
from deepctr_torch import models as M  # noqa: E402
from deepctr_torch._hip.graph import GraphedTrainStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("models", nargs="?", default=None, help="comma-separated subset of the table below")
ap.add_argument("--optimizer", default="adagrad", choices=["sgd", "adagrad", "adam", "rmsprop"])
ap.add_argument("--reference-defaults", action="store_true", help="the models' default L2 kwargs instead of l2_reg_* = 0")
ap.add_argument("--blocks", type=int, default=1, help="timed blocks per route (median and spread are reported)")
args = ap.parse_args()
dev, B, V = "cuda:0", 4096, 1_000_000
cols = [SparseFeat("C%d" % i, V, 16) for i in range(26)] + [DenseFeat("I%d" % i, 1) for i in range(13)]
gen = torch.Generator().manual_seed(0)
n = B * 16
X = torch.cat([torch.randint(0, V, (n, 26), generator=gen).float(), torch.rand(n, 13, generator=gen)], 1).to(dev)
y = torch.randint(0, 2, (n,), generator=gen).float().to(dev)


def l2(**kw):
    """the l2_reg_* = 0 kwargs of a table entry; none of them in the reference-defaults mode"""
    return {} if args.reference_defaults else kw


Vs = 100_000      # ONN keeps one table per field PAIR: 26 x 26 tables; at V = 1e6 that is 43 GB before any optimizer state
cols_onn = [SparseFeat("C%d" % i, Vs, 16) for i in range(26)] + [DenseFeat("I%d" % i, 1) for i in range(13)]
spec = {
    "DeepFM": lambda: M.DeepFM(cols, cols, dnn_hidden_units=(256, 128), device=dev, **l2(l2_reg_linear=0, l2_reg_embedding=0)),
    "xDeepFM": lambda: M.xDeepFM(cols, cols, dnn_hidden_units=(256, 256), cin_layer_size=(128, 128), cin_split_half=True,
                                 device=dev, **l2(l2_reg_linear=0, l2_reg_embedding=0)),
    "FiBiNET": lambda: M.FiBiNET(cols, cols, dnn_hidden_units=(128, 128), device=dev, **l2(l2_reg_linear=0, l2_reg_embedding=0)),
    "DCN": lambda: M.DCN(cols, cols, dnn_hidden_units=(256, 128), device=dev, **l2(l2_reg_linear=0, l2_reg_embedding=0)),
    "DCN_matrix": lambda: M.DCN(cols, cols, cross_parameterization="matrix", dnn_hidden_units=(256, 128), device=dev,
                                **l2(l2_reg_linear=0, l2_reg_embedding=0, l2_reg_cross=0)),
    "PNN": lambda: M.PNN(cols, dnn_hidden_units=(256, 128), device=dev, **l2(l2_reg_embedding=0)),
    "NFM": lambda: M.NFM(cols, cols, dnn_hidden_units=(256, 128), device=dev, **l2(l2_reg_linear=0, l2_reg_embedding=0)),
    "WDL": lambda: M.WDL(cols, cols, dnn_hidden_units=(256, 128), device=dev, **l2(l2_reg_linear=0, l2_reg_embedding=0)),
    "AutoInt": lambda: M.AutoInt(cols, cols, att_layer_num=3, att_head_num=2, dnn_hidden_units=(256, 128),
                                 device=dev, **l2(l2_reg_embedding=0)),
    "DCNMix": lambda: M.DCNMix(cols, cols, dnn_hidden_units=(256, 128), device=dev,
                               **l2(l2_reg_linear=0, l2_reg_embedding=0, l2_reg_cross=0)),
    "AFM": lambda: M.AFM(cols, cols[:26], attention_factor=8, device=dev,
                         **l2(l2_reg_linear=0, l2_reg_embedding=0, l2_reg_att=0)),
    "IFM": lambda: M.IFM(cols, cols, dnn_hidden_units=(256, 128), device=dev, **l2(l2_reg_linear=0, l2_reg_embedding=0)),
    "DIFM": lambda: M.DIFM(cols, cols, dnn_hidden_units=(256, 128), device=dev, **l2(l2_reg_linear=0, l2_reg_embedding=0)),
    "CCPM": lambda: M.CCPM(cols[:26], cols[:26], dnn_hidden_units=(256,), device=dev,
                           **l2(l2_reg_linear=0, l2_reg_embedding=0)),
    "ONN": lambda: M.ONN(cols_onn, cols_onn, dnn_hidden_units=(128, 128), device=dev,
                         **l2(l2_reg_linear=0, l2_reg_embedding=0)),
}
res = {}
only = set(args.models.split(",")) if args.models else None


def timed(fn, steps, blocks):
    """-> (median, spread) seconds per step over `blocks` blocks of `steps` steps"""
    per = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(steps)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / steps)
    per.sort()
    return per[len(per) // 2], per[-1] - per[0]


for name, make in spec.items():
    if only is not None and name not in only:
        continue
    try:
        m = make()
        m.compile(args.optimizer, "binary_crossentropy", metrics=[])
        m.train()

        def batch(i):
            j = i % 16
            return X[j * B:(j + 1) * B], y[j * B:(j + 1) * B]

        for i in range(3):
            m._train_step(*batch(i))

        def eager_steps(k):
            for i in range(k):
                m._train_step(*batch(i))

        eager, spread = timed(eager_steps, 20, args.blocks)
        r = {"eager_ms": eager * 1e3, "eager_spread_ms": spread * 1e3, "eager_samples_per_s": B / eager,
             "fused_step": bool(m._fused and m._fused.get("ok")), "optimizer": args.optimizer,
             "reference_defaults": bool(args.reference_defaults), "update": list(m.model_plan().update)}
        try:
            if not m._graph_safe_step():
                raise RuntimeError("the step is not replay-safe (_graph_safe_step)")
            gs = GraphedTrainStep(m, *batch(0), steps_per_graph=2).capture(*batch(0))
            for i in range(6):
                gs(*batch(i))
            gs.flush()

            def graph_steps(k):
                for i in range(k):
                    gs(*batch(i))
                gs.flush()

            gt, gspread = timed(graph_steps, 60, args.blocks)
            r.update(graph_ms=gt * 1e3, graph_spread_ms=gspread * 1e3, graph_samples_per_s=B / gt)
        except Exception as exc:  # noqa: BLE001
            r["graph_error"] = "%s: %s" % (type(exc).__name__, str(exc)[:200])
            torch.cuda.synchronize()
        m.model_plan().check_ids()
        res[name] = r
        del m
        torch.cuda.empty_cache()
    except Exception as exc:  # noqa: BLE001
        res[name] = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:300])}
print(json.dumps(res, indent=1))
