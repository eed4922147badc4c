#!/usr/bin/env python
"""Timing of CCPM's conv stack (csrc/ccpm.hip) and of the model that uses it.  Writes profiles/ccpm_*.json.

    python tools/bench_ccpm.py kernel [--out DIR]
        ConvLayer at the Criteo shape (26 fields of 16, widths (6, 5), filters (4, 4): k = 13, 3): the fused forward +
        backward pair (dctr_ccpm_fwd with a selection buffer, dctr_ccpm_bwd and its reduce) at B = 4096 and 262144, and at
        B = 4096 the layer's own torch-op route -- the reference's formulation on PyTorch-ROCm: F.pad, a library
        convolution, tanh, torch.topk per layer and autograd's backward.  Both through ``ConvLayer`` itself (forward, then
        torch.autograd.grad for the input and the four parameters), each captured as a hipGraph of one call and replayed;
        after 20 warm-up replays the median of 5 repeats of >= 0.5 s of replays by device events.  The forward alone
        (no selection buffer, as predict() runs it) is timed the same way.  B = 262144 is the kernel alone: the library
        convolution on a [262144, C, 26, 16] image did not finish its first call within seven minutes on an MI355X
        (CCPM_BENCH_TORCH_LARGE=1 to try).
    python tools/bench_ccpm.py model [--out DIR]
        ms per CCPM train step through hipGraph replay at the Criteo shape (26 sparse, 13 dense on the linear side, D = 16,
        batch 4096, dnn (256,)), Adagrad with l2 = 0 and the reference's default kwargs (L2 + Adam).
    python tools/bench_ccpm.py trace-model
        a few eager Adagrad steps, for `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_ccpm.py
        trace-model` (on its own, without counters)."""
import argparse
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
WIDTHS, FILTERS = (6, 5), (4, 4)


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


def cmd_kernel(out):
    from deepctr_torch.layers import ConvLayer
    torch.manual_seed(0)
    layer = ConvLayer(F, WIDTHS, FILTERS, device=DEV)
    params = list(layer.parameters())
    assert layer._kernel_fits(F, D, *layer._spec())
    res = {"what": __doc__.split("python tools/bench_ccpm.py model")[0].strip(), "device": torch.cuda.get_device_name(0),
           "F": F, "D": D, "widths": WIDTHS, "filters": FILTERS, "k": layer._spec()[2], "shapes": []}
    for B in (4096, 262144):
        x = (torch.randn(B, 1, F, D, device=DEV) * 0.3).requires_grad_(True)
        go = torch.randn(B, FILTERS[-1], layer.filed_shape, D, device=DEV)

        def fused_pair():
            torch.autograd.grad(layer(x), [x] + params, go)

        def torch_pair():
            torch.autograd.grad(layer.conv_layer(x), [x] + params, go)

        def fused_fwd():
            with torch.no_grad():
                layer(x)

        def torch_fwd():
            with torch.no_grad():
                layer.conv_layer(x)

        e = {"B": B}
        res["shapes"].append(e)
        # the fused route first; every figure is printed and saved as soon as it exists (the library convolution may spend
        # minutes choosing its algorithm at a shape it has not seen)
        for tag, fn in (("fused_fwd_bwd", fused_pair), ("fused_fwd", fused_fwd), ("torch_fwd_bwd", torch_pair),
                        ("torch_fwd", torch_fwd)):
            if tag.startswith("torch") and B > 4096 and os.environ.get("CCPM_BENCH_TORCH_LARGE", "0") != "1":
                continue
            t0 = time.perf_counter()
            try:
                med, runs = replay_ms(fn)
            except Exception as exc:  # noqa: BLE001   (a torch op that cannot be captured: recorded, not fatal)
                if tag.startswith("fused"):
                    raise
                e[tag + "_error"] = "%s: %s" % (type(exc).__name__, str(exc)[:200])
                torch.cuda.synchronize()
                continue
            e[tag + "_ms"] = med
            e[tag + "_runs_ms"] = runs
            print("B=%d %s: %.4f ms (measured in %.1f s)" % (B, tag, med, time.perf_counter() - t0), flush=True)
            if "torch_fwd_bwd_ms" in e:
                e["pair_speedup_vs_torch"] = e["torch_fwd_bwd_ms"] / e["fused_fwd_bwd_ms"]
                e["fused_pair_faster_than_torch"] = bool(e["fused_fwd_bwd_ms"] < e["torch_fwd_bwd_ms"])
            if "torch_fwd_ms" in e:
                e["fwd_speedup_vs_torch"] = e["torch_fwd_ms"] / e["fused_fwd_ms"]
            with open(os.path.join(out, "ccpm_kernel.json"), "w") as f:
                json.dump(res, f, indent=1)
        del x, go
        torch.cuda.empty_cache()


def criteo_ccpm(V, kw):
    from deepctr_torch import models as M
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    sparse = [SparseFeat("C%d" % i, V, D) for i in range(F)]
    dense = [DenseFeat("I%d" % i, 1) for i in range(N_DENSE)]
    return M.CCPM(sparse + dense, sparse, conv_kernel_width=WIDTHS, conv_filters=FILTERS, dnn_hidden_units=(256,),
                  device=DEV, **kw)


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

    res = {"what": "ms per CCPM train step through hipGraph replay, Criteo shape (26 sparse x %d rows, 13 dense on the linear "
                   "side, D = 16, widths (6, 5), filters (4, 4)), batch 4096, dnn (256,); host clock around replays that end "
                   "in a device synchronise, 3 repeats of >= 1 s" % V, "device": torch.cuda.get_device_name(0), "vocab": V,
           "configs": {}}
    for tag, opt, kw in (("adagrad_l2_0", "adagrad", dict(l2_reg_linear=0, l2_reg_embedding=0)),
                         ("default_kwargs_adam", "adam", {})):
        m = criteo_ccpm(V, kw)
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
    with open(os.path.join(out, "ccpm_models.json"), "w") as f:
        json.dump(res, f, indent=1)


def cmd_trace_model(V):
    B = 4096
    X, y = criteo_data(V, B, 4)
    m = criteo_ccpm(V, dict(l2_reg_linear=0, l2_reg_embedding=0))
    m.compile("adagrad", "binary_crossentropy", metrics=[])
    m.train()
    for i in range(10):
        j = i % 4
        m._train_step(X[j * B:(j + 1) * B], y[j * B:(j + 1) * B])
    torch.cuda.synchronize()
    print(json.dumps({"model": "CCPM", "steps": 10, "batch": B, "vocab": V}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["kernel", "model", "trace-model"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--vocab", type=int, default=100_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_ccpm.py measures on the GPU: no device found")
    os.makedirs(a.out, exist_ok=True)
    if a.cmd == "kernel":
        cmd_kernel(a.out)
    elif a.cmd == "model":
        cmd_model(a.out, a.vocab)
    else:
        cmd_trace_model(a.vocab)
