#!/usr/bin/env python
"""Timing of AFN's logarithmic transformation layer (csrc/log_transform.hip) and of the model that uses it.  Writes
profiles/afn_kernel.json.

    python tools/bench_afn.py [--out DIR]
        ``LogTransformLayer`` at the Criteo shape (B 4096, 26 fields of 16, 256 logarithmic neurons) in train mode: the
        forward alone and forward + backward (torch.autograd.grad for the input and the six parameters), the fused route
        against the layer's own torch-op route (the reference's op sequence on PyTorch-ROCm).  Each captured as a hipGraph
        of one call and replayed; after 20 warm-up replays the median of 5 repeats of >= 0.5 s of replays by device events.
        The forward is also set against its byte floor: one write of the [B, E*H] output plus one read of the input, at
        the streaming rate given with --stream-gbs (default 4000 GB/s; DESIGN.md quotes the measured rate of the pool).
        Then ms per AFN train step (26 sparse fields, D 16, batch 4096, default layer sizes, Adagrad with l2 = 0), eager
        steps timed by the host clock around a device synchronise, both routes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deepctr-torch_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_ccpm import replay_ms  # noqa: E402

DEV = "cuda:0"
B, F, E, H = 4096, 26, 16, 256


def layer_times(res, out):
    from deepctr_torch.layers import LogTransformLayer
    torch.manual_seed(0)
    layer = LogTransformLayer(F, E, H).to(DEV).train()
    params = list(layer.parameters())
    x = (torch.randn(B, F, E, device=DEV) * 0.15).requires_grad_(True)
    go = torch.randn(B, E * H, device=DEV)

    def fwd():
        with torch.no_grad():
            layer(x)

    def pair():
        torch.autograd.grad(layer(x), [x] + params, go)

    for route, env in (("fused", "1"), ("torch", "0")):
        os.environ["DCTR_LOG_TRANSFORM"] = env
        for tag, fn in (("fwd", fwd), ("fwd_bwd", pair)):
            med, runs = replay_ms(fn)
            res["%s_%s_ms" % (route, tag)], res["%s_%s_runs_ms" % (route, tag)] = med, runs
            print("%s %s: %.4f ms" % (route, tag, med), flush=True)
            with open(out, "w") as f:
                json.dump(res, f, indent=1)
    os.environ.pop("DCTR_LOG_TRANSFORM")
    res["fwd_speedup_vs_torch"] = res["torch_fwd_ms"] / res["fused_fwd_ms"]
    res["pair_speedup_vs_torch"] = res["torch_fwd_bwd_ms"] / res["fused_fwd_bwd_ms"]
    res["fused_loses"] = [t for t in ("fwd", "fwd_bwd") if res["fused_%s_ms" % t] >= res["torch_%s_ms" % t]]
    floor_bytes = 4 * (B * E * H + B * F * E)
    res["fwd_byte_floor_ms"] = floor_bytes / (res["stream_gbs"] * 1e9) * 1e3
    res["fwd_over_byte_floor"] = res["fused_fwd_ms"] / res["fwd_byte_floor_ms"]


def model_times(res, vocab):
    from deepctr_torch.inputs import SparseFeat
    from deepctr_torch.models import AFN
    g = torch.Generator().manual_seed(0)
    X = torch.randint(0, vocab, (B * 4, F), generator=g).float().to(DEV)
    y = torch.randint(0, 2, (B * 4,), generator=g).float().to(DEV)
    for route, env in (("fused", "1"), ("torch", "0")):
        os.environ["DCTR_LOG_TRANSFORM"] = env
        cols = [SparseFeat("C%d" % i, vocab, E) for i in range(F)]
        m = AFN(cols, cols, l2_reg_linear=0, l2_reg_embedding=0, device=DEV)
        m.compile("adagrad", "binary_crossentropy", metrics=[])
        m.train()
        for i in range(5):
            m._train_step(X[(i % 4) * B:(i % 4 + 1) * B], y[(i % 4) * B:(i % 4 + 1) * B])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(40):
            m._train_step(X[(i % 4) * B:(i % 4 + 1) * B], y[(i % 4) * B:(i % 4 + 1) * B])
        torch.cuda.synchronize()
        res["%s_train_step_eager_ms" % route] = (time.perf_counter() - t0) / 40 * 1e3
        res["update"] = list(map(str, m.model_plan().update))
        print("%s train step: %.4f ms" % (route, res["%s_train_step_eager_ms" % route]), flush=True)
        del m
        torch.cuda.empty_cache()
    os.environ.pop("DCTR_LOG_TRANSFORM")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--stream-gbs", type=float, default=4000.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_afn.py measures on the GPU: no device found")
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "afn_kernel.json")
    res = {"what": __doc__.strip(), "device": torch.cuda.get_device_name(0), "B": B, "F": F, "E": E, "H": H,
           "stream_gbs": a.stream_gbs}
    layer_times(res, path)
    model_times(res, a.vocab)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k.endswith("_ms") or "speedup" in k or "floor" in k}))
