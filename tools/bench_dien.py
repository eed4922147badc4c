#!/usr/bin/env python
"""Timing of DIEN's recurrences (csrc/gru_seq.hip) and of the whole DIEN train step.  Writes profiles/dien_kernel.json.

    python tools/bench_dien.py [--out DIR]
        B = 4096, T = 50, H = 32, lengths uniform in 0..50.
        (1) The recurrence alone, per mode (GRU, AIGRU, AGRU, AUGRU), forward and forward + backward (gradients of the
            input, the scores and the four parameter tensors):
              fused        ``layers.sequence.gru_sequence`` -> dctr_gru_seq_fwd / _bwd, captured as a hipGraph and replayed;
              torch_masked the same layer as PyTorch-ROCm ops on padded tensors (``gru_sequence_torch``, what
                           ``DCTR_GRU_SEQ=0`` runs: one batched input projection, then T masked cell steps), captured
                           and replayed as well;
              torch_packed the reference's formulation: rows of length 0 dropped, ``pack_padded_sequence`` with
                           ``lengths.cpu()``, then ``nn.GRU`` (GRU, AIGRU) or the ``DynamicGRU`` loop over the packed time
                           steps (AGRU, AUGRU), then ``pad_packed_sequence``.  Its device-to-host copy of the lengths
                           cannot be captured, so it is timed EAGERLY: device events around n calls with a
                           synchronisation after them, host launch overhead included -- that overhead is part of what
                           this route costs inside ``fit()``.
        (2) The whole train step of DIEN (item 16 + category 16 over T = 50, user 8, tower (256, 128), adagrad) for
            gru_type GRU and AUGRU, with and without negative sampling, fused against ``DCTR_GRU_SEQ=0``: a replayed
            hipGraph of ``_train_step`` where it captures, else eager calls (``route`` says which).  Every configuration
            runs in a process of its own.
    After warm-up, 5 repeats of >= 0.3 s by device events: the median and every repeat are kept."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deepctr-torch_amd"))
import torch  # noqa: E402

DEV = "cuda:0"
B, T, H = 4096, 50, 32
MODES = ("GRU", "AIGRU", "AGRU", "AUGRU")


def _timed(call, seconds=0.3, repeats=5):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    runs = []
    for _ in range(repeats):
        n, total, calls = 2, 0.0, 0
        while total < seconds * 1e3:
            a.record()
            for _ in range(n):
                call()
            b.record()
            torch.cuda.synchronize()
            total += a.elapsed_time(b)
            calls += n
            n = min(n * 2, 1024)
        runs.append(total / calls)
    return statistics.median(runs), runs


def replay_ms(fn, warm=20):
    """median ms per call of `fn` captured as a hipGraph and replayed"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(warm):
        g.replay()
    torch.cuda.synchronize()
    return _timed(g.replay)


def eager_ms(fn, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    return _timed(fn)


def bench_layers(res):
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    from deepctr_torch.layers import DynamicGRU
    from deepctr_torch.layers.sequence import gru_sequence, gru_sequence_torch
    gen = torch.Generator().manual_seed(0)
    lengths = torch.randint(0, T + 1, (B,), generator=gen).to(DEV)
    res["mean_length"] = float(lengths.float().mean())
    x = torch.randn(B, T, H, device=DEV).requires_grad_(True)
    att = torch.rand(B, T, device=DEV).requires_grad_(True)
    g_last = torch.randn(B, H, device=DEV)
    for mode in MODES:
        torch.manual_seed(0)
        gru = torch.nn.GRU(H, H, batch_first=True).to(DEV)
        cell = DynamicGRU(H, H, gru_type=mode if mode in ("AGRU", "AUGRU") else "AGRU").to(DEV)
        with torch.no_grad():
            for p in gru.parameters():
                p.normal_(0, 0.2)
            for p, q in zip((cell.rnn.weight_ih, cell.rnn.weight_hh, cell.rnn.bias_ih, cell.rnn.bias_hh),
                            (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)):
                p.copy_(q)
        w = [gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0]
        a = None if mode == "GRU" else att
        wrt = [x] + ([att] if a is not None else []) + w

        def fused():
            return gru_sequence(x.reshape(B, T * H), [(H, 0, H)], T, lengths, a, mode, *w, want_states=False)[1]

        def masked():
            return gru_sequence_torch(x, a, lengths, *w, gru_type=mode)[1]

        def packed():
            keep = lengths > 0
            n = lengths[keep]
            xs = x[keep] * att[keep].unsqueeze(-1) if mode == "AIGRU" else x[keep]
            px = pack_padded_sequence(xs, n.cpu(), batch_first=True, enforce_sorted=False)
            if mode in ("GRU", "AIGRU"):
                last = gru(px)[1].squeeze(0)
            else:
                pa = pack_padded_sequence(att[keep], n.cpu(), batch_first=True, enforce_sorted=False)
                states, _ = pad_packed_sequence(cell(px, pa), batch_first=True, total_length=T)
                last = states[torch.arange(states.shape[0], device=DEV), n - 1]
            out = x.new_zeros((B, H))
            out[keep] = last
            return out

        def pair(f, params):
            return lambda: torch.autograd.grad(f(), params, g_last)

        def fwd(f):
            def run():
                with torch.no_grad():
                    f()
            return run
        e = {"mode": mode}
        res["layers"].append(e)
        cell_w = [cell.rnn.weight_ih, cell.rnn.weight_hh, cell.rnn.bias_ih]
        packed_wrt = wrt if mode in ("GRU", "AIGRU") else [x, att] + cell_w
        for tag, timer, fn in (("fused_fwd", replay_ms, fwd(fused)), ("fused_fwd_bwd", replay_ms, pair(fused, wrt)),
                               ("torch_masked_fwd", replay_ms, fwd(masked)),
                               ("torch_masked_fwd_bwd", replay_ms, pair(masked, wrt)),
                               ("torch_packed_fwd_eager", eager_ms, fwd(packed)),
                               ("torch_packed_fwd_bwd_eager", eager_ms, pair(packed, packed_wrt))):
            t0 = time.perf_counter()
            med, runs = timer(fn)
            e[tag + "_ms"], e[tag + "_runs_ms"] = med, runs
            print("%-5s %-28s %.4f ms, repeats %s (measured in %.1f s)" % (
                mode, tag, med, " ".join("%.4f" % r for r in runs), time.perf_counter() - t0), flush=True)


def one_step(gru_type, neg, fused):
    """this process: one whole-step configuration -> a JSON line on stdout"""
    os.environ["DCTR_GRU_SEQ"] = "1" if fused else "0"
    import numpy as np
    from deepctr_torch.inputs import SparseFeat, VarLenSparseFeat
    from deepctr_torch.models import DIEN
    feats = [("item", 5000, 16), ("cate", 200, 16)]
    cols = [SparseFeat("user", 10000, 8)] + [SparseFeat(n, v, d) for n, v, d in feats]
    for prefix in ["hist_"] + (["neg_hist_"] if neg else []):
        cols += [VarLenSparseFeat(SparseFeat(prefix + n, v, d, embedding_name=n), T, length_name="seq_length")
                 for n, v, d in feats]
    torch.manual_seed(0)
    m = DIEN(cols, ["item", "cate"], gru_type=gru_type, use_negsampling=neg, alpha=0.5, init_std=0.05, device=DEV)
    m.compile("adagrad", "binary_crossentropy", metrics=[])
    m.train()
    rng = np.random.RandomState(0)
    n = rng.randint(0, T + 1, B)
    X = np.zeros((B, max(hi for _, hi in m.feature_index.values())), np.float32)
    for c in cols:
        lo, hi = m.feature_index[c.name]
        if isinstance(c, VarLenSparseFeat):
            ids = rng.randint(1, c.vocabulary_size, (B, T))
            ids[np.arange(T)[None, :] >= n[:, None]] = 0
            X[:, lo:hi] = ids
        else:
            X[:, lo] = rng.randint(0, c.vocabulary_size, B)
    X[:, m.feature_index["seq_length"][0]] = n
    X, y = torch.from_numpy(X).to(DEV), torch.from_numpy(rng.randint(0, 2, B).astype(np.float32)).to(DEV)
    for _ in range(3):
        m._train_step(X, y)
    torch.cuda.synchronize()
    route = "eager"
    if os.environ.get("DCTR_BENCH_GRAPH", "1") != "0":
        try:
            med, runs = replay_ms(lambda: m._train_step(X, y))
            route = "graph"
        except Exception as exc:            # a step that does not capture: say so, measure in a fresh process
            print(json.dumps({"capture_failed": "%s: %s" % (type(exc).__name__, str(exc).splitlines()[0])}), flush=True)
            os._exit(3)
    if route == "eager":
        med, runs = eager_ms(lambda: m._train_step(X, y))
    print(json.dumps({"gru_type": gru_type, "use_negsampling": neg, "fused": fused, "route": route, "step_ms": med,
                      "step_runs_ms": runs}), flush=True)


def bench_steps(res):
    for gru_type in ("GRU", "AUGRU"):
        for neg in (False, True):
            for fused in (True, False):
                arg = "%s:%d:%d" % (gru_type, neg, fused)
                env, note = dict(os.environ), None
                for attempt in range(2):
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", arg], env=env,
                                       capture_output=True, text=True, timeout=300)
                    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
                    if p.returncode == 0 and lines:
                        e = lines[-1]
                        if note:
                            e["capture_failed"] = note
                        res["steps"].append(e)
                        print("step %-5s neg=%d fused=%d %s: %.4f ms" % (gru_type, neg, fused, e["route"], e["step_ms"]),
                              flush=True)
                        break
                    if p.returncode == 3 and lines:
                        note = lines[-1]["capture_failed"]
                        env["DCTR_BENCH_GRAPH"] = "0"
                        continue
                    raise RuntimeError("step %s failed (exit %d): %s" % (arg, p.returncode, p.stderr[-2000:]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--one", default=None, help="internal: one whole-step configuration, gru_type:neg:fused")
    ap.add_argument("--skip-steps", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_dien.py measures on the GPU: no device found")
    if a.one:
        gt, neg, fused = a.one.split(":")
        one_step(gt, bool(int(neg)), bool(int(fused)))
        sys.exit(0)
    os.makedirs(a.out, exist_ok=True)
    res = {"what": __doc__.strip(), "device": torch.cuda.get_device_name(0), "B": B, "T": T, "H": H, "layers": [],
           "steps": []}
    bench_layers(res)
    with open(os.path.join(a.out, "dien_kernel.json"), "w") as f:
        json.dump(res, f, indent=1)
    if not a.skip_steps:
        bench_steps(res)
        with open(os.path.join(a.out, "dien_kernel.json"), "w") as f:
            json.dump(res, f, indent=1)
