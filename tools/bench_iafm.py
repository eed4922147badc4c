#!/usr/bin/env python
"""Timing of the input-aware FM (csrc/iafm.hip) and of the two models that use it.  Writes profiles/iafm_*.json.

    python tools/bench_iafm.py kernel [--out DIR]    dctr_iafm_fwd + _bwd against the reference's formulation as torch ops on
                                                     the same device (softmax, * F, the two broadcasts, FM's sum / pow / sub,
                                                     the refined wide sum, and autograd's backward of all of it), both in
                                                     one process, alternating, after warm-up, device events over >= 1 s of
                                                     work each, three repeats; (B, F, D) = (4096, 26, 16), (262144, 26, 16)
    python tools/bench_iafm.py trace-kernel          the fused pair alone at the saturating size, for a separate
                                                     `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bench_iafm.py trace-kernel`
    python tools/bench_iafm.py model [--out DIR]     ms per train step of IFM and DIFM through graph replay at bench.py's
                                                     Criteo shape (26 sparse x 1 M rows, 13 dense, D = 16, batch 4096), Adagrad
                                                     with l2 = 0 and the reference's default kwargs, DeepFM beside them
    python tools/bench_iafm.py trace-model NAME      a few eager steps of one model, for a kernel trace of one step

Algorithmic bytes per sample (floats x 4): forward reads F*D + 2F + 1 and writes F + 2; backward reads F*D + 2F + 2 and
writes F*D + 2F + 1."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deepctr-torch_amd"))
import torch  # noqa: E402

DEV = "cuda:0"
SHAPES = [(4096, 26, 16), (262144, 26, 16)]


def algorithmic_bytes(B, F, D):
    fwd = (F * D + 2 * F + 1) + (F + 2)
    bwd = (F * D + 2 * F + 2) + (F * D + 2 * F + 1)
    return 4 * B * fwd, 4 * B * bwd


def torch_formulation(G, Wl, Z1, F, D):
    """ifm.py:77-83 + basemodel.py:80-91 as the reference spells them (IFM: softmax mode)."""
    B = G.shape[0]
    m = F * Z1.softmax(1)
    emb = G[:, :F * D].reshape(B, F, D)
    lin = torch.sum(torch.cat([Wl[:, f:f + 1].unsqueeze(1) for f in range(F)], dim=-1) * m.unsqueeze(1), dim=-1)
    lin = lin + Wl[:, F:F + 1]
    v = emb * m.unsqueeze(-1)
    square_of_sum = torch.pow(torch.sum(v, dim=1, keepdim=True), 2)
    sum_of_square = torch.sum(v * v, dim=1, keepdim=True)
    fm = 0.5 * torch.sum(square_of_sum - sum_of_square, dim=2, keepdim=False)
    return lin, fm


def kernel_inputs(B, F, D):
    g = torch.Generator().manual_seed(0)
    ld = (F * D + 13 + 3) // 4 * 4
    G = (torch.randn(B, ld, generator=g) * 0.3).to(DEV).requires_grad_(True)
    Wl = torch.randn(B, F + 1, generator=g).to(DEV).requires_grad_(True)
    Z1 = torch.randn(B, F, generator=g).to(DEV).requires_grad_(True)
    r = torch.randn(B, 1, generator=g).to(DEV)
    return G, Wl, Z1, r


def step_fn(kind, G, Wl, Z1, r, F, D):
    from deepctr_torch._hip import ops

    def fused():
        lin, fm = ops.iafm(G, Wl, Z1, None, True, F, D)
        torch.autograd.grad([lin, fm], [G, Wl, Z1], [r, r])

    def ref():
        lin, fm = torch_formulation(G, Wl, Z1, F, D)
        torch.autograd.grad([lin, fm], [G, Wl, Z1], [r, r])
    return fused if kind == "fused" else ref


def timed(fn, seconds):
    """ms per call by device events over at least `seconds` of device work"""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total, calls = 8, 0.0, 0
    while total < seconds * 1e3:
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
        calls += n
        n = min(n * 2, 4096)
    return total / calls


def cmd_kernel(out):
    res = {"what": "dctr_iafm_fwd + dctr_iafm_bwd (through ops.iafm + autograd) against the reference's formulation as torch "
                   "ops, IFM mode; ms per forward + backward by device events, 3 alternating repeats of >= 1 s each",
           "shapes": []}
    for B, F, D in SHAPES:
        G, Wl, Z1, r = kernel_inputs(B, F, D)
        fns = {k: step_fn(k, G, Wl, Z1, r, F, D) for k in ("fused", "torch")}
        for fn in fns.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        runs = {"fused": [], "torch": []}
        for _ in range(3):
            for k in ("fused", "torch"):
                runs[k].append(timed(fns[k], 1.0))
        fb, bb = algorithmic_bytes(B, F, D)
        e = {"B": B, "F": F, "D": D, "fused_ms": runs["fused"], "torch_ms": runs["torch"],
             "fused_spread_ms": max(runs["fused"]) - min(runs["fused"]),
             "torch_spread_ms": max(runs["torch"]) - min(runs["torch"]),
             "speedup_of_medians": sorted(runs["torch"])[1] / sorted(runs["fused"])[1],
             "algorithmic_bytes": {"fwd": fb, "bwd": bb}}
        spread = max(e["fused_spread_ms"], e["torch_spread_ms"])
        e["fused_not_slower"] = bool(sorted(runs["fused"])[1] <= sorted(runs["torch"])[1] + spread)
        res["shapes"].append(e)
        print(json.dumps(e))
    with open(os.path.join(out, "iafm_kernel.json"), "w") as f:
        json.dump(res, f, indent=1)
    if not all(e["fused_not_slower"] for e in res["shapes"]):
        sys.exit("the fused pair is slower than the torch formulation by more than the measured spread")


def cmd_trace_kernel():
    B, F, D = SHAPES[1]
    G, Wl, Z1, r = kernel_inputs(B, F, D)
    fn = step_fn("fused", G, Wl, Z1, r, F, D)
    for _ in range(50):
        fn()
    torch.cuda.synchronize()
    fb, bb = algorithmic_bytes(B, F, D)
    print(json.dumps({"B": B, "F": F, "D": D, "launches_each": 50, "algorithmic_bytes": {"fwd": fb, "bwd": bb}}))


def criteo_models():
    from deepctr_torch import models as M
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    V = 1_000_000
    cols = [SparseFeat("C%d" % i, V, 16) for i in range(26)] + [DenseFeat("I%d" % i, 1) for i in range(13)]
    l2 = dict(l2_reg_linear=0, l2_reg_embedding=0)
    return cols, V, {
        "DeepFM": lambda kw: M.DeepFM(cols, cols, dnn_hidden_units=(256, 128), device=DEV, **kw),
        "IFM": lambda kw: M.IFM(cols, cols, dnn_hidden_units=(256, 128), device=DEV, **kw),
        "DIFM": lambda kw: M.DIFM(cols, cols, att_head_num=4, dnn_hidden_units=(256, 128), device=DEV, **kw),
    }, l2


def criteo_data(V, B, n_batches=16):
    g = torch.Generator().manual_seed(0)
    n = B * n_batches
    X = torch.cat([torch.randint(0, V, (n, 26), generator=g).float(), torch.rand(n, 13, generator=g)], 1).to(DEV)
    y = torch.randint(0, 2, (n,), generator=g).float().to(DEV)
    return X, y


def cmd_model(out):
    from deepctr_torch._hip.graph import GraphedTrainStep
    B = 4096
    cols, V, makes, l2zero = criteo_models()
    X, y = criteo_data(V, B)

    def batch(i):
        j = i % 16
        return X[j * B:(j + 1) * B], y[j * B:(j + 1) * B]

    res = {"what": "ms per train step through hipGraph replay, Criteo shape (26 x 1M rows, 13 dense, D = 16), batch 4096; "
                   "host clock around replays that end in a device synchronise, 3 repeats of >= 1 s",
           "configs": {}}
    for tag, opt, kw in (("adagrad_l2_0", "adagrad", l2zero), ("default_kwargs_adam", "adam", {})):
        for name, make in makes.items():
            m = make(kw)
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
                        for i in range(100):
                            gs(*batch(n + i))
                        n += 100
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
                for i in range(50):
                    m._train_step(*batch(i))
                torch.cuda.synchronize()
                r["eager_ms"] = (time.perf_counter() - t0) / 50 * 1e3
            m.model_plan().check_ids()
            res["configs"].setdefault(tag, {})[name] = r
            print(tag, name, json.dumps(r))
            del m
            torch.cuda.empty_cache()
    with open(os.path.join(out, "iafm_models.json"), "w") as f:
        json.dump(res, f, indent=1)


def cmd_trace_model(name):
    B = 4096
    cols, V, makes, l2zero = criteo_models()
    X, y = criteo_data(V, B, 4)
    m = makes[name](l2zero)
    m.compile("adagrad", "binary_crossentropy", metrics=[])
    m.train()
    for i in range(10):
        j = i % 4
        m._train_step(X[j * B:(j + 1) * B], y[j * B:(j + 1) * B])
    torch.cuda.synchronize()
    print(json.dumps({"model": name, "steps": 10, "batch": B}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["kernel", "trace-kernel", "model", "trace-model"])
    ap.add_argument("name", nargs="?", default="IFM")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_iafm.py measures on the GPU: no device found")
    os.makedirs(a.out, exist_ok=True)
    if a.cmd == "kernel":
        cmd_kernel(a.out)
    elif a.cmd == "trace-kernel":
        cmd_trace_kernel()
    elif a.cmd == "model":
        cmd_model(a.out)
    else:
        cmd_trace_model(a.name)
