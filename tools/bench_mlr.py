#!/usr/bin/env python
"""Timing of MLR's mixture kernels (csrc/mlr.hip) and of the model that uses them.  Writes profiles/mlr_kernel.json.

    python tools/bench_mlr.py [--out DIR] [--vocab N] [--batch B]

Shape: Criteo -- 26 sparse columns of ``--vocab`` rows (default 1 M, bench.py's vocabulary) + 13 dense, uniform ids, batch
4096, region_num 4, without and with a bias side of 4 sparse columns of its own: 104 / 108 four-byte row reads per sample.
Per configuration, on ONE model whose route is switched by DCTR_MLR between measurements (fused: csrc/mlr.hip; composed:
one per-field dctr_embed_fwd on the same plan + torch ops), the two routes alternating inside every repeat:

  fwd            dctr_mlr_fwd alone through the C ABI, a captured hipGraph of one call replayed: after 20 warm-up replays the
                 median of 5 repeats of >= 0.3 s of replays by device events; rows / s = B * n_wide / time
  fwd_bwd        model forward + backward of sum(y) including the in-kernel Adagrad table update (no regulariser, no dense
                 optimizer step), as a replayed hipGraph (same protocol) and eagerly (host clock around 3 x >= 0.3 s of
                 calls ending in a device synchronise)
  train_step     ``_train_step`` (Adagrad, BCE): eagerly, and as fit() runs it -- a hipGraph of the step replayed
                 (GraphedTrainStep), host clock around replays that end in a synchronise.  The step includes what the
                 reference's MLR does every step besides the mixture: the L2 term and the dense Adagrad step of the dead
                 ``embedding_dict`` / ``linear_model`` (O(vocabulary), the same on both routes)."""
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
F, N_DENSE, N_BIAS, R = 26, 13, 4, 4
ROUTES = (("fused", "1"), ("composed", "0"))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def capture(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    return g


def replay_once(g, seconds=0.3):
    """ms per replay over >= ``seconds`` of replays, by device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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
    return total / calls


def host_once(fn, seconds=0.3):
    """ms per call over >= ``seconds`` of calls, host clock around work that ends in a device synchronise"""
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(20):
            fn()
        n += 20
        torch.cuda.synchronize()
        if time.perf_counter() - t0 >= seconds:
            return (time.perf_counter() - t0) / n * 1e3


def alternate(makers, once, repeats):
    """{route: [ms per repeat]}: ``makers[route]()`` sets the route and returns what ``once`` times; routes alternate"""
    things = {}
    for tag, env in ROUTES:
        os.environ["DCTR_MLR"] = env
        things[tag] = makers(tag)
    runs = {tag: [] for tag, _ in ROUTES}
    for _ in range(repeats):
        for tag, env in ROUTES:
            os.environ["DCTR_MLR"] = env
            runs[tag].append(once(things[tag]))
    return runs


def summary(runs):
    return {tag: {"median_ms": statistics.median(v), "runs_ms": v} for tag, v in runs.items()}


def build(V, with_bias):
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    from deepctr_torch.models import MLR
    region = [SparseFeat("C%d" % i, V, 4) for i in range(F)] + [DenseFeat("I%d" % i, 1) for i in range(N_DENSE)]
    bias = [SparseFeat("B%d" % i, V, 4) for i in range(N_BIAS)] if with_bias else None
    m = MLR(region, bias_feature_columns=bias, region_num=R, device=DEV)
    with torch.no_grad():       # trained-like weights: with the default init_std every gate is uniform
        for k, p in m.named_parameters():
            if k.startswith("region_linear_model."):
                p.normal_(0, 0.3)
            elif k.startswith("bias_model."):
                p.normal_(0, 0.2)
    return m


def data(m, V, B, n_batches=8):
    g = torch.Generator().manual_seed(0)
    n = B * n_batches
    nc = max(hi for _, hi in m.feature_index.values())
    X = torch.rand(n, nc, generator=g)
    for name, (lo, hi) in m.feature_index.items():
        if name[0] in "CB":
            X[:, lo] = torch.randint(0, V, (n,), generator=g).float()
    return X.to(DEV), torch.randint(0, 2, (n,), generator=g).float().to(DEV)


def bench_config(V, B, with_bias):
    from deepctr_torch._hip import lib as L
    from deepctr_torch._hip.graph import GraphedTrainStep
    lib = L.lib()
    m = build(V, with_bias)
    m.compile("adagrad", "binary_crossentropy", metrics=[])
    m.train()
    X, y = data(m, V, B)
    plan, heads = m.model_plan(), m.mlr_heads()

    def batch(i):
        j = i % 8
        return X[j * B:(j + 1) * B], y[j * B:(j + 1) * B]

    Xb = batch(0)[0]
    n_wide = len(plan.wide)
    res = {"bias_side": bool(with_bias), "B": B, "region_num": R, "n_wide_fields": n_wide, "n_dense_weights": heads.n_dense,
           "update": list(map(str, plan.update)), "supported": bool(heads.supported(DEV))}

    # ---- the forward kernel alone ---------------------------------------------------------------------------------------
    cplan, cmlr = plan.bind(DEV), heads.bind(DEV)
    yb = torch.empty((B,), device=DEV)
    zb = torch.empty((B, heads.n_heads), device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)

    def fwd():
        L.check(lib.dctr_mlr_fwd(cplan, cmlr, _ptr(Xb), Xb.stride(0), B, _ptr(yb), _ptr(zb), zb.stride(0), _ptr(err), None,
                                 None, None, 0, L.stream_handle(DEV)), "dctr_mlr_fwd")
    g = capture(fwd)
    runs = [replay_once(g) for _ in range(5)]
    res["fwd"] = {"median_ms": statistics.median(runs), "runs_ms": runs,
                  "rows_per_s": B * n_wide / (statistics.median(runs) * 1e-3)}
    assert int(err.item()) == 0

    # ---- forward + backward with the table update, both routes ----------------------------------------------------------
    gy = torch.ones((B, 1), device=DEV)

    def fwd_bwd():
        m(Xb).backward(gy)

    try:
        res["fwd_bwd_graph"] = summary(alternate(lambda tag: capture(fwd_bwd), replay_once, 5))
    except Exception as exc:  # noqa: BLE001   (capture is how fit() runs the step; recorded if it cannot be taken here)
        res["fwd_bwd_graph_error"] = "%s: %s" % (type(exc).__name__, str(exc)[:300])
        torch.cuda.synchronize()
    res["fwd_bwd_eager"] = summary(alternate(lambda tag: fwd_bwd, host_once, 3))

    # ---- the train step, eagerly and as fit() replays it --------------------------------------------------------------
    state = {"i": 0}

    def step():
        state["i"] += 1
        m._train_step(*batch(state["i"]))

    res["train_step_eager"] = summary(alternate(lambda tag: step, host_once, 3))

    def graphed(tag):
        for i in range(3):
            m._train_step(*batch(i))
        torch.cuda.synchronize()
        gs = GraphedTrainStep(m, *batch(0), steps_per_graph=1).capture(*batch(0))
        for i in range(10):
            gs(*batch(i))
        gs.flush()
        torch.cuda.synchronize()

        def one():
            state["i"] += 1
            gs(*batch(state["i"]))
        return one

    try:
        res["train_step_graph"] = summary(alternate(graphed, host_once, 3))
    except Exception as exc:  # noqa: BLE001
        res["train_step_graph_error"] = "%s: %s" % (type(exc).__name__, str(exc)[:300])
        torch.cuda.synchronize()
    plan.check_ids()
    for key in ("fwd_bwd_graph", "fwd_bwd_eager", "train_step_eager", "train_step_graph"):
        if key in res:
            res[key]["composed_over_fused"] = res[key]["composed"]["median_ms"] / res[key]["fused"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_mlr.py measures on the GPU: no device found")
    os.makedirs(a.out, exist_ok=True)
    res = {"what": __doc__.strip(), "device": torch.cuda.get_device_name(0), "vocab": a.vocab, "configs": []}
    for with_bias in (False, True):
        r = bench_config(a.vocab, a.batch, with_bias)
        res["configs"].append(r)
        print(json.dumps(r))
        torch.cuda.empty_cache()
    os.environ.pop("DCTR_MLR", None)
    with open(os.path.join(a.out, "mlr_kernel.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
