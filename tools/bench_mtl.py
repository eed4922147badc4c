#!/usr/bin/env python
"""Timing of the multi-task gate mix (csrc/gate_mix.hip).  Writes profiles/mtl_kernel.json.

    python tools/bench_mtl.py [--out DIR]
        (a) kernel level, B = 4096: ``_hip.ops.gate_mix`` on the fused route (dctr_gate_mix_fwd with the weights buffer,
            dctr_gate_mix_bwd and its reduce) against the same gating as PyTorch-ROCm ops (``gate_mix_torch``: the
            reference's Linear / softmax / stack / matmul per gate, and autograd's backward), forward alone and forward +
            backward (torch.autograd.grad for every expert output, gate input and gate weight):
              mmoe      MMOE's defaults: P 3, G 2 (every gate over the whole pool), dim 128, H 64
              ple_3_3   one CGC level of PLE with 3 shared and 3 specific experts, two tasks: P 9, G 3 (two task gates
                        over 6 members, the shared gate over 9), dim 128, H 64
        (b) the whole train step (``_train_step``: lookup, every DNN, gates, heads, list-loss, backward with the table
            update inside, dense Adagrad) of MMOE and PLE(3, 3, 3 levels) at their default widths on Criteo-shaped columns
            (26 sparse of 16, 13 dense), B = 4096, with DCTR_GATE_MIX on and off.
    Everything is captured as a hipGraph and replayed; after 20 warm-up replays, 5 repeats of >= 0.5 s of replays timed by
    device events: the median and every repeat are kept.  Both routes are measured in this one process on one device."""
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
B, DIM, H = 4096, 128, 64
KERNEL_CASES = {
    "mmoe": (3, [(0, 1, 2)] * 2),
    "ple_3_3": (9, [(0, 1, 2, 6, 7, 8), (3, 4, 5, 6, 7, 8), tuple(range(9))]),
}


def timed_ms(launch, seconds=0.5, repeats=5, warm=20):
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    runs = []
    for _ in range(repeats):
        n, total, calls = 4, 0.0, 0
        while total < seconds * 1e3:
            a.record()
            for _ in range(n):
                launch()
            b.record()
            torch.cuda.synchronize()
            total += a.elapsed_time(b)
            calls += n
            n = min(n * 2, 1024)
        runs.append(total / calls)
    return statistics.median(runs), runs


def replay_ms(fn):
    """median ms per call of ``fn`` captured as a hipGraph and replayed (no launch overhead of the host in the figure)"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return timed_ms(g.replay)


def kernel_level(res):
    from deepctr_torch._hip import ops
    for name, (P, members) in KERNEL_CASES.items():
        torch.manual_seed(0)
        xs = [(torch.randn(B, DIM, device=DEV) * 0.5).requires_grad_(True) for _ in range(P)]
        hs = [(torch.randn(B, H, device=DEV) * 0.5).requires_grad_(True) for _ in members]
        Ws = [(torch.randn(len(m), H, device=DEV) / H ** 0.5).requires_grad_(True) for m in members]
        gos = [torch.randn(B, DIM, device=DEV) for _ in members]
        assert ops.gate_mix_fused(xs, hs, Ws, members)
        leaves = xs + hs + Ws

        def fused_pair():
            torch.autograd.grad(ops.gate_mix(xs, hs, Ws, members), leaves, gos)

        def torch_pair():
            torch.autograd.grad(ops.gate_mix_torch(xs, hs, Ws, members), leaves, gos)

        def fused_fwd():
            with torch.no_grad():
                ops.gate_mix(xs, hs, Ws, members)

        def torch_fwd():
            with torch.no_grad():
                ops.gate_mix_torch(xs, hs, Ws, members)

        e = {"case": name, "B": B, "P": P, "G": len(members), "n": [len(m) for m in members], "dim": DIM, "H": H}
        res["kernel"].append(e)
        for tag, fn in (("fused_fwd_bwd", fused_pair), ("fused_fwd", fused_fwd), ("torch_fwd_bwd", torch_pair),
                        ("torch_fwd", torch_fwd)):
            t0 = time.perf_counter()
            e[tag + "_ms"], e[tag + "_runs_ms"] = replay_ms(fn)
            print("%s %s: %.4f ms, repeats %s (measured in %.1f s)" % (
                name, tag, e[tag + "_ms"], " ".join("%.4f" % r for r in e[tag + "_runs_ms"]), time.perf_counter() - t0),
                flush=True)
        e["pair_speedup_vs_torch"] = e["torch_fwd_bwd_ms"] / e["fused_fwd_bwd_ms"]
        e["fwd_speedup_vs_torch"] = e["torch_fwd_ms"] / e["fused_fwd_ms"]


def train_step(res):
    from deepctr_torch._hip.graph import GraphedTrainStep
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    from deepctr_torch.models import MMOE, PLE
    cols = [SparseFeat("C%d" % i, 1000 + 37 * i, 16) for i in range(26)] + [DenseFeat("I%d" % i, 1) for i in range(13)]
    gen = torch.Generator().manual_seed(0)
    X = torch.cat([torch.stack([torch.randint(0, 1000 + 37 * i, (B,), generator=gen).float() for i in range(26)], 1),
                   torch.rand(B, 13, generator=gen)], 1).to(DEV)
    y = torch.randint(0, 2, (B, 2), generator=gen).float().to(DEV)
    for name, make in (("MMOE", lambda: MMOE(cols, device=DEV)),
                       ("PLE_3_3_3", lambda: PLE(cols, shared_expert_num=3, specific_expert_num=3, num_levels=3,
                                                 device=DEV))):
        e = {"model": name, "B": B}
        res["train_step"].append(e)
        for tag, switch in (("fused", "1"), ("torch", "0")):
            os.environ["DCTR_GATE_MIX"] = switch
            torch.manual_seed(0)
            m = make()
            m.compile("adagrad", ["binary_crossentropy"] * 2, metrics=[])
            m.train()
            for _ in range(3):
                m._train_step(X, y)
            torch.cuda.synchronize()
            gr = GraphedTrainStep(m, X, y).capture(X, y)
            t0 = time.perf_counter()
            e[tag + "_ms"], e[tag + "_runs_ms"] = timed_ms(lambda: gr(X, y))
            print("%s step, gate mix %s: %.4f ms, repeats %s (measured in %.1f s)" % (
                name, tag, e[tag + "_ms"], " ".join("%.4f" % r for r in e[tag + "_runs_ms"]), time.perf_counter() - t0),
                flush=True)
        os.environ.pop("DCTR_GATE_MIX", None)
        e["step_speedup_vs_torch"] = e["torch_ms"] / e["fused_ms"]


def main(out):
    res = {"what": __doc__.strip(), "device": torch.cuda.get_device_name(0), "kernel": [], "train_step": []}
    for part in (kernel_level, train_step):
        part(res)
        with open(os.path.join(out, "mtl_kernel.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_mtl.py measures on the GPU: no device found")
    os.makedirs(a.out, exist_ok=True)
    main(a.out)
