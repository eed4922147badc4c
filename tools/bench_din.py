#!/usr/bin/env python
"""Timing of DIN's attention pooling (csrc/din.hip).  Writes profiles/din_kernel.json.

    python tools/bench_din.py [--out DIR]
        AttentionSequencePoolingLayer at B = 4096, T = 50, E = 32, hidden (64, 16), ``sigmoid``, lengths uniform in 0..50:
        the fused route (dctr_din_attn_fwd with the weights buffer, dctr_din_attn_bwd and its reduce) against the layer's
        own torch-op route -- the reference's formulation on PyTorch-ROCm: expand, cat to [B, T, 4E], two nn.Linear over
        B*T rows, where, bmm, and autograd's backward.  Both through the layer itself (forward, then torch.autograd.grad
        for query, keys and the six parameters), each captured as a hipGraph of one call and replayed; after 20 warm-up
        replays, 5 repeats of >= 0.5 s of replays by device events: the median and every repeat are kept.  The forward
        alone (no weights buffer, as predict() runs it) is timed the same way, with and without weight normalisation."""
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
B, T, E, HIDDEN, ACT = 4096, 50, 32, (64, 16), "sigmoid"


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


def main(out):
    from deepctr_torch.layers import AttentionSequencePoolingLayer
    res = {"what": __doc__.strip(), "device": torch.cuda.get_device_name(0), "B": B, "T": T, "E": E, "hidden": HIDDEN,
           "activation": ACT, "configs": []}
    gen = torch.Generator().manual_seed(0)
    lengths = torch.randint(0, T + 1, (B, 1), generator=gen).to(DEV)
    res["mean_length"] = float(lengths.float().mean())
    for softmax in (False, True):
        torch.manual_seed(0)
        layer = AttentionSequencePoolingLayer(HIDDEN, ACT, weight_normalization=softmax, embedding_dim=E).to(DEV)
        with torch.no_grad():
            for fc in layer.local_att.dnn.linears:
                fc.weight.normal_(0, 1.0 / fc.in_features ** 0.5)
        params = list(layer.parameters())
        q = (torch.randn(B, 1, E, device=DEV) * 0.3).requires_grad_(True)
        k = (torch.randn(B, T, E, device=DEV) * 0.3).requires_grad_(True)
        go = torch.randn(B, 1, E, device=DEV)
        assert layer.kernel_route(T, [E], (q, k), True) == ACT
        valid = layer._valid(k, lengths, None)

        def fused_pair():
            torch.autograd.grad(layer(q, k, lengths), [q, k] + params, go)

        def torch_pair():
            torch.autograd.grad(layer._forward_torch(q, k, valid), [q, k] + params, go)

        def fused_fwd():
            with torch.no_grad():
                layer(q, k, lengths)

        def torch_fwd():
            with torch.no_grad():
                layer._forward_torch(q, k, valid)

        e = {"weight_normalization": softmax}
        res["configs"].append(e)
        for tag, fn in (("fused_fwd_bwd", fused_pair), ("fused_fwd", fused_fwd), ("torch_fwd_bwd", torch_pair),
                        ("torch_fwd", torch_fwd)):
            t0 = time.perf_counter()
            med, runs = replay_ms(fn)
            e[tag + "_ms"] = med
            e[tag + "_runs_ms"] = runs
            print("softmax=%d %s: %.4f ms, repeats %s (measured in %.1f s)" % (
                softmax, tag, med, " ".join("%.4f" % r for r in runs), time.perf_counter() - t0), flush=True)
        e["pair_speedup_vs_torch"] = e["torch_fwd_bwd_ms"] / e["fused_fwd_bwd_ms"]
        e["fwd_speedup_vs_torch"] = e["torch_fwd_ms"] / e["fused_fwd_ms"]
        with open(os.path.join(out, "din_kernel.json"), "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_din.py measures on the GPU: no device found")
    os.makedirs(a.out, exist_ok=True)
    main(a.out)
