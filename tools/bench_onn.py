#!/usr/bin/env python
"""Timing of ONN's pair lookup (csrc/pair_embed.hip) and of the model that uses it.  Writes profiles/onn_*.json.

    python tools/bench_onn.py kernel [--out DIR] [--rowbench FILE]
        dctr_pair_embed_fwd and _bwd at F = 26 (325 pairs, 650 tables), D = 16, 1 M rows per table (bench.py's vocabulary),
        uniform ids, B = 4096 and 262144, against two baselines in the same process:
          (a) "embed+mul": what the library offered before -- dctr_embed_fwd over the same 650 fields into [B, 650 * 16]
              followed by one torch multiply of the two halves of every pair; backward two torch multiplies into the
              row-gradient layout;
          (b) "torch": the reference's formulation (models/onn.py:98-120) on the GPU -- 650 F.embedding, 325 multiplies, a
              cat, and autograd's backward (650 dense [V, D] gradients).
        Each measured as a captured hipGraph of one call, replayed; after 20 warm-up replays the median of 5 repeats of
        >= 0.5 s of replays by device events.  The row-read rate (B * 650 rows per forward) is set against
        tools/micro/rowbench.hip's `read64_sat_u8` when its output (run on the same device) is given with --rowbench.
    python tools/bench_onn.py model [--out DIR]
        ms per ONN train step through hipGraph replay at the Criteo shape (26 sparse, 13 dense, D = 16, batch 4096),
        Adagrad with l2 = 0 and the reference's default kwargs (L2 + Adam).  --vocab rows per table (default 100 000: the
        reference's constructor draws every pair table twice on the host, 650 tables of 1 M rows take minutes there).
    python tools/bench_onn.py trace-model
        a few eager Adagrad steps, for `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_onn.py
        trace-model` (on its own, without counters)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deepctr-torch_amd"))
import torch  # noqa: E402

DEV = "cuda:0"
F, D, N_DENSE = 26, 16, 13


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def replay_ms(fn, seconds=0.5, repeats=5, warm=20):
    """median ms per call of `fn` captured as a hipGraph and replayed (no launch overhead of the host in the figure)"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(warm):
        g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    runs = []
    for _ in range(repeats):
        n, total, calls = 4, 0.0, 0
        while total < seconds * 1e3:
            a.record()
            for _ in range(n):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            total += a.elapsed_time(b)
            calls += n
            n = min(n * 2, 1024)
        runs.append(total / calls)
    return statistics.median(runs), runs


def kernel_setup(V):
    from deepctr_torch._hip.plan import EmbeddingPlan
    from deepctr_torch.inputs import DenseFeat, SparseFeat, build_input_features
    from deepctr_torch.models.basemodel import Linear
    cols = [SparseFeat("C%d" % i, V, D) for i in range(F)] + [DenseFeat("I%d" % i, 1) for i in range(N_DENSE)]
    fi = build_input_features(cols)
    lin = Linear(cols, fi, device=DEV).to(DEV)
    pairs = [(i, j) for i in range(F - 1) for j in range(i + 1, F)]
    fields = []
    for (i, j) in pairs:
        for e, f in ((1, i), (2, j)):
            w = torch.nn.Parameter(torch.randn(V, D, device=DEV) * 0.1)
            fields.append(("C%d+C%d.emb%d" % (i, j, e), w, fi["C%d" % f][0]))
    kw = dict(deep_columns=cols, deep_fields=fields, wide_columns=cols, wide_tables=lin.embedding_dict,
              wide_dense_weight=lin.weight)
    return fi, lin, pairs, fields, EmbeddingPlan(fi, pair=True, **kw), EmbeddingPlan(fi, **kw)


def cmd_kernel(out, V, rowbench):
    from deepctr_torch._hip import lib as L
    lib = L.lib()
    fi, lin, pairs, fields, pplan, eplan = kernel_setup(V)
    P = len(pairs)
    cp, ce = pplan.bind(DEV), eplan.bind(DEV)
    s = lambda: L.stream_handle(DEV)      # noqa: E731
    rate = None
    if rowbench and os.path.exists(rowbench):
        with open(rowbench) as f:
            rate = json.load(f)["read64_sat_u8"]["Mrows_per_s"] * 1e6
    res = {"what": __doc__.split("python tools/bench_onn.py model")[0].strip(), "device": torch.cuda.get_device_name(0),
           "F": F, "pairs": P, "D": D, "vocab": V, "rowbench_read64_rows_per_s": rate, "shapes": []}
    g = torch.Generator().manual_seed(0)
    for B in (4096, 262144):
        X = torch.cat([torch.randint(0, V, (B, F), generator=g).float(), torch.rand(B, N_DENSE, generator=g)], 1).to(DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        out_p = torch.empty((B, pplan.ld_out), device=DEV)
        wide = torch.empty((B,), device=DEV)
        g_out = torch.randn((B, pplan.ld_out), device=DEV)
        g_rows = torch.empty((B, pplan.ld_rows), device=DEV)
        out_e = torch.empty((B, eplan.ld_out), device=DEV)
        prod = torch.empty((B, P, D), device=DEV)
        rows_a = torch.empty((B, P, 2, D), device=DEV)

        def fused_fwd():
            L.check(lib.dctr_pair_embed_fwd(cp, _ptr(X), X.stride(0), B, _ptr(out_p), pplan.ld_out, _ptr(wide), 1, _ptr(err),
                                            s()), "pair fwd")

        def fused_bwd():
            L.check(lib.dctr_pair_embed_bwd(cp, _ptr(X), X.stride(0), B, _ptr(g_out), pplan.ld_out, _ptr(g_rows),
                                            pplan.ld_rows, s()), "pair bwd")

        def a_fwd():
            L.check(lib.dctr_embed_fwd(ce, _ptr(X), X.stride(0), B, _ptr(out_e), eplan.ld_out, _ptr(wide), 1, None, _ptr(err),
                                       None, 0, None, None, None, 0, s()), "embed fwd")
            e = out_e[:, :2 * P * D].view(B, P, 2, D)
            torch.mul(e[:, :, 0], e[:, :, 1], out=prod)

        def a_bwd():       # (the rows saved by the forward: no second lookup)
            e = out_e[:, :2 * P * D].view(B, P, 2, D)
            gp = g_out[:, :P * D].view(B, P, D)
            torch.mul(gp, e[:, :, 1], out=rows_a[:, :, 0])
            torch.mul(gp, e[:, :, 0], out=rows_a[:, :, 1])

        tabs = [f[1] for f in fields]
        idx = [X[:, f[2]].long() for f in fields]

        def b_fwd_bwd():
            embs = [torch.nn.functional.embedding(idx[2 * p], tabs[2 * p]) *
                    torch.nn.functional.embedding(idx[2 * p + 1], tabs[2 * p + 1]) for p in range(P)]
            o = torch.cat(embs + [X[:, F:]], dim=-1)
            torch.autograd.grad([o], tabs, [g_out[:, :o.shape[1]]])

        def b_fwd():
            with torch.no_grad():
                embs = [torch.nn.functional.embedding(idx[2 * p], tabs[2 * p]) *
                        torch.nn.functional.embedding(idx[2 * p + 1], tabs[2 * p + 1]) for p in range(P)]
                torch.cat(embs + [X[:, F:]], dim=-1)

        e = {"B": B}
        for tag, fn in (("fused_fwd", fused_fwd), ("a_embed_mul_fwd", a_fwd), ("fused_bwd", fused_bwd),
                        ("a_embed_mul_bwd", a_bwd), ("b_torch_fwd", b_fwd), ("b_torch_fwd_bwd", b_fwd_bwd)):
            if tag.startswith("b_") and B > 4096 and os.environ.get("ONN_BENCH_TORCH_LARGE", "0") != "1":
                continue      # (650 dense [1M, 16] gradients per call at B = 262144: ONN_BENCH_TORCH_LARGE=1 to include)
            try:
                med, runs = replay_ms(fn)
            except Exception as exc:  # noqa: BLE001   (a torch op that cannot be captured: recorded, not fatal)
                if not tag.startswith("b_"):
                    raise
                e[tag + "_error"] = "%s: %s" % (type(exc).__name__, str(exc)[:200])
                torch.cuda.synchronize()
                continue
            e[tag + "_ms"] = med
            e[tag + "_runs_ms"] = runs
        e["fwd_speedup_vs_a"] = e["a_embed_mul_fwd_ms"] / e["fused_fwd_ms"]
        e["bwd_ratio_vs_a"] = e["a_embed_mul_bwd_ms"] / e["fused_bwd_ms"]
        e["fwd_rows_per_s"] = B * 2.0 * P / (e["fused_fwd_ms"] * 1e-3)
        e["bwd_rows_per_s"] = B * 2.0 * P / (e["fused_bwd_ms"] * 1e-3)
        if rate:
            e["fwd_fraction_of_rowbench"] = e["fwd_rows_per_s"] / rate
            e["bwd_fraction_of_rowbench"] = e["bwd_rows_per_s"] / rate
        e["fused_fwd_faster_than_a"] = bool(e["fused_fwd_ms"] < e["a_embed_mul_fwd_ms"])
        assert int(err.item()) == 0
        res["shapes"].append(e)
        print(json.dumps(e))
        del out_p, g_out, g_rows, out_e, prod, rows_a
        torch.cuda.empty_cache()
    with open(os.path.join(out, "onn_kernel.json"), "w") as f:
        json.dump(res, f, indent=1)
    if not all(e["fused_fwd_faster_than_a"] for e in res["shapes"]):
        sys.exit("the fused forward is not faster than dctr_embed_fwd + multiply: a finding to explain")


def criteo_onn(V, kw):
    from deepctr_torch import models as M
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    cols = [SparseFeat("C%d" % i, V, D) for i in range(F)] + [DenseFeat("I%d" % i, 1) for i in range(N_DENSE)]
    return M.ONN(cols, cols, dnn_hidden_units=(128, 128), device=DEV, **kw)


def criteo_data(V, B, n_batches=8):
    g = torch.Generator().manual_seed(0)
    n = B * n_batches
    X = torch.cat([torch.randint(0, V, (n, F), generator=g).float(), torch.rand(n, N_DENSE, generator=g)], 1).to(DEV)
    y = torch.randint(0, 2, (n,), generator=g).float().to(DEV)
    return X, y


def cmd_model(out, V):
    from deepctr_torch._hip.graph import GraphedTrainStep
    B = 4096
    X, y = criteo_data(V, B)

    def batch(i):
        j = i % 8
        return X[j * B:(j + 1) * B], y[j * B:(j + 1) * B]

    res = {"what": "ms per ONN train step through hipGraph replay, Criteo shape (26 sparse x %d rows, 13 dense, D = 16: 325 "
                   "pairs, 650 pair tables), batch 4096, dnn (128, 128); host clock around replays that end in a device "
                   "synchronise, 3 repeats of >= 1 s" % V, "device": torch.cuda.get_device_name(0), "vocab": V, "configs": {}}
    for tag, opt, kw in (("adagrad_l2_0", "adagrad", dict(l2_reg_linear=0, l2_reg_embedding=0)),
                         ("default_kwargs_adam", "adam", {})):
        m = criteo_onn(V, kw)
        m.compile(opt, "binary_crossentropy", metrics=[])
        m.train()
        for i in range(3):
            m._train_step(*batch(i))
        torch.cuda.synchronize()
        r = {"update": list(map(str, m.model_plan().update))}
        try:
            gs = GraphedTrainStep(m, *batch(0), steps_per_graph=2).capture(*batch(0))
            for i in range(10):
                gs(*batch(i))
            gs.flush()
            torch.cuda.synchronize()
            runs = []
            for _ in range(3):
                n, t0 = 0, time.perf_counter()
                while True:
                    for i in range(50):
                        gs(*batch(n + i))
                    n += 50
                    gs.flush()
                    torch.cuda.synchronize()
                    if time.perf_counter() - t0 >= 1.0:
                        break
                runs.append((time.perf_counter() - t0) / n * 1e3)
            r["graph_ms"] = runs
        except Exception as exc:  # noqa: BLE001
            r["graph_error"] = "%s: %s" % (type(exc).__name__, str(exc)[:300])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(30):
                m._train_step(*batch(i))
            torch.cuda.synchronize()
            r["eager_ms"] = (time.perf_counter() - t0) / 30 * 1e3
        m.model_plan().check_ids()
        res["configs"][tag] = r
        print(tag, json.dumps(r))
        del m
        torch.cuda.empty_cache()
    with open(os.path.join(out, "onn_models.json"), "w") as f:
        json.dump(res, f, indent=1)


def cmd_trace_model(V):
    B = 4096
    X, y = criteo_data(V, B, 4)
    m = criteo_onn(V, dict(l2_reg_linear=0, l2_reg_embedding=0))
    m.compile("adagrad", "binary_crossentropy", metrics=[])
    m.train()
    for i in range(10):
        j = i % 4
        m._train_step(X[j * B:(j + 1) * B], y[j * B:(j + 1) * B])
    torch.cuda.synchronize()
    print(json.dumps({"model": "ONN", "steps": 10, "batch": B, "vocab": V}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["kernel", "model", "trace-model"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--vocab", type=int, default=None)
    ap.add_argument("--rowbench", default=None, help="output of tools/micro/rowbench run on this device (json)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_onn.py measures on the GPU: no device found")
    os.makedirs(a.out, exist_ok=True)
    if a.cmd == "kernel":
        cmd_kernel(a.out, a.vocab or 1_000_000, a.rowbench)
    elif a.cmd == "model":
        cmd_model(a.out, a.vocab or 100_000)
    else:
        cmd_trace_model(a.vocab or 100_000)
