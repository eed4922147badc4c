"""GPU: ``LogTransformFunction`` (csrc/log_transform.hip) alone against the float64 restatement in tests/mock_afn.py --
forward and backward in train mode, the one-launch forward in eval mode, ``keep`` on and off.

BOUND.  The layer's error depends on the data (1/x of the log, exp, batch statistics over few samples), so it is not fixed
in advance.  Per case the layer's own torch route -- the reference's op sequence -- runs on the CPU in float32 on the same
inputs; its deviation from float64, per tensor and scaled by max|value64|, is what a correct float32 implementation shows
on this data.  The kernel has to stay within 4 x that (2 for device exp / log being 1 ulp off the CPU's, 2 for a different
but equally valid reduction order) and never has to do better than 1e-6 x scale.  For the batch statistics the float32 side
is torch's mean / var of the same logs and exponentials.  Both numbers are printed per case (``-s``).

Shapes, chosen where indexing can break: B 1, 2, 33, 65, 257 (tile and partial boundaries) and 1100 / 4129 (more tiles than
workgroups along B: the grid-stride loops of the forward and of the backward's main pass; more samples than BN0
workgroups); F 1 (a degenerate norm), 3, 26, 27 (odd: the MFMA's K is padded); E 1, 5, 16; H 1, 7, 32, 33, 256 (two
128-column slices).  A strided input starting mid-row; inputs with exact 0, +-1e-7, +-5e-8 (mask and sign checked element
by element); a shape outside the envelope; two runs bit for bit.

MEASURED on the MI355X: every case holds, the largest kernel / bound is 0.448 (the strided case).  The hardest case is
``B33-F1-E5-H1``: its one-element ``ltl_weights`` gradient is a sum that cancels to 1/188 of its terms (BatchNorm's backward
projects out what exp(z) ~ 1 + z is made of when F = H = 1).  With ``logf`` / ``expf`` and float statistics the kernel was at
3.2e-5 there against a bound of 1.86e-6 (torch-float32: 4.7e-7); with the statistics, the log and the exp in double it is at
0.28 of the bound."""
import ctypes

import numpy as np
import pytest
import torch

import mock_afn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENOSUP = -2
FLOOR, FACTOR = 1e-6, 4.0
NAMES = ["ltl_weights", "ltl_biases", "bn.0.weight", "bn.0.bias", "bn.1.weight", "bn.1.bias"]
_worst = {"ratio": 0.0, "kernel": 0.0, "torch32": 0.0}

CASES = [  # B, F, E, H
    (1, 3, 5, 7), (2, 1, 1, 33), (33, 26, 16, 256), (65, 27, 5, 32), (257, 3, 16, 33), (33, 1, 5, 1), (65, 26, 16, 7),
    (2, 27, 1, 256), (1100, 3, 1, 7), (4129, 3, 2, 7)]


def make(B, F, E, H, seed, special=False):
    rng = np.random.RandomState(seed)
    X = rng.normal(0, 0.15, (B, F, E)).astype(np.float32)
    if special:
        vals = np.array([0.0, 1e-7, -1e-7, 5e-8, -5e-8, -0.3], np.float32)
        flat = X.reshape(-1)
        idx = rng.choice(flat.size, size=min(flat.size // 2, 4 * vals.size), replace=False)
        flat[idx] = vals[np.arange(idx.size) % vals.size]
    p = {"ltl_weights": rng.normal(0, 0.3 / np.sqrt(max(F, 4) / 4.0), (F, H)), "ltl_biases": rng.normal(0, 0.05, (1, 1, H)),
         "bn.0.weight": 1 + 0.3 * rng.normal(0, 1, E), "bn.0.bias": 0.1 * rng.normal(0, 1, E),
         "bn.1.weight": 1 + 0.3 * rng.normal(0, 1, E), "bn.1.bias": 0.1 * rng.normal(0, 1, E)}
    p = {k: v.astype(np.float32) for k, v in p.items()}
    run = [rng.normal(-2.5, 0.3, E), rng.uniform(0.5, 2.0, E), rng.uniform(0.8, 1.5, E), rng.uniform(0.5, 3.0, E)]
    gout = rng.normal(0, 1, (B, E * H)).astype(np.float32)
    return X, p, [r.astype(np.float32) for r in run], gout


def torch32(X, p, run, gout, train):
    """the layer's torch route on the CPU in float32 -> out, gradients, the float32 batch statistics"""
    from deepctr_torch.layers import LogTransformLayer
    F, H = p["ltl_weights"].shape
    layer = LogTransformLayer(F, X.shape[2], H)
    sd = {k: torch.from_numpy(v) for k, v in p.items()}
    for i in range(2):
        sd["bn.%d.running_mean" % i], sd["bn.%d.running_var" % i] = torch.from_numpy(run[2 * i]), torch.from_numpy(run[2 * i + 1])
        sd["bn.%d.num_batches_tracked" % i] = torch.tensor(0)
    layer.load_state_dict(sd)
    layer.train(train)
    x = torch.from_numpy(X).clone().requires_grad_(train)
    out = layer._torch_route(x)
    res = {"out": out.detach().numpy()}
    if train:
        gs = torch.autograd.grad(out, [x] + [dict(layer.named_parameters())[k] for k in NAMES], torch.from_numpy(gout))
        res.update({k: g.numpy() for k, g in zip(["gX"] + NAMES, gs)})
        with torch.no_grad():
            a = torch.log(torch.clamp(torch.abs(x), min=1e-7)).transpose(1, 2)
            n = layer.bn[0](a)
            y = torch.exp(torch.matmul(n, layer.ltl_weights) + layer.ltl_biases)
            res["stats"] = torch.stack([a.mean((0, 2)), a.var((0, 2), unbiased=False), y.mean((0, 2)),
                                        y.var((0, 2), unbiased=False)]).numpy()
    return res


def float64(X, p, run, gout, train):
    args = [p[k] for k in NAMES]
    if not train:
        return {"out": mock_afn.forward(X, *args, stats=run)[0]}
    out, stats, _ = mock_afn.forward(X, *args)
    r = mock_afn.backward(X, p["ltl_weights"], p["ltl_biases"], p["bn.0.weight"], p["bn.0.bias"], p["bn.1.weight"], stats,
                          gout)
    return {"out": out, "stats": stats, "gX": r["gX"], "ltl_weights": r["gW"], "ltl_biases": r["gbias"].reshape(1, 1, -1),
            "bn.0.weight": r["g_bn0_w"], "bn.0.bias": r["g_bn0_b"], "bn.1.weight": r["g_bn1_w"], "bn.1.bias": r["g_bn1_b"]}


def kernel(Xd, p, run, gout, train, keep):
    """``LogTransformFunction`` on device tensors (``Xd`` may be a strided view) -> the same dict"""
    from deepctr_torch._hip.ops import LogTransformFunction
    x = Xd.detach().requires_grad_(keep)
    ps = [torch.from_numpy(p[k]).to(DEV).requires_grad_(keep) for k in NAMES]
    rs = [torch.from_numpy(r).to(DEV) for r in run]
    out, stats = LogTransformFunction.apply(x, *ps, *rs, train, keep)
    res = {"out": out.detach().cpu().numpy(), "stats": stats.cpu().numpy()}
    if keep:
        gs = torch.autograd.grad(out, [x] + ps, torch.from_numpy(gout).to(DEV))
        res.update({k: g.cpu().numpy() for k, g in zip(["gX"] + NAMES, gs)})
    torch.cuda.synchronize()
    return res


def check(tag, got, ref32, ref64):
    worst = 0.0
    for k, want in ref64.items():
        want = np.asarray(want, np.float64)
        for i in range(4 if k == "stats" else 1):      # each statistic on its own scale
            w = want[i] if k == "stats" else want
            g, r = (got[k][i], ref32[k][i]) if k == "stats" else (got[k], ref32[k])
            scale = float(np.max(np.abs(w)))
            if scale == 0.0:
                assert float(np.max(np.abs(g))) <= 1e-12, k
                continue
            dev32 = float(np.max(np.abs(np.asarray(r, np.float64).reshape(w.shape) - w))) / scale
            devk = float(np.max(np.abs(np.asarray(g, np.float64).reshape(w.shape) - w))) / scale
            bound = max(FACTOR * dev32, FLOOR)
            print("afn kernel %s %-12s%s kernel %.3e  torch32 %.3e  bound %.3e" % (tag, k, "[%d]" % i if k == "stats" else "",
                                                                                  devk, dev32, bound))
            _worst["ratio"] = max(_worst["ratio"], devk / bound)
            _worst["kernel"], _worst["torch32"] = max(_worst["kernel"], devk), max(_worst["torch32"], dev32)
            worst = max(worst, devk / bound)
            assert np.all(np.isfinite(g)), k
            assert devk <= bound, "%s %s: kernel %.3e > bound %.3e (torch32 %.3e)" % (tag, k, devk, bound, dev32)
    print("afn kernel %s: worst kernel / bound %.3f (largest so far: ratio %.3f, kernel %.3e, torch32 %.3e)" % (
        tag, worst, _worst["ratio"], _worst["kernel"], _worst["torch32"]))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-F%d-E%d-H%d" % c)
def test_train_forward_and_backward_against_float64(case):
    B, F, E, H = case
    X, p, run, gout = make(B, F, E, H, seed=B + 10 * F + 100 * E + H)
    ref64, ref32 = float64(X, p, run, gout, True), torch32(X, p, run, gout, True)
    Xd = torch.from_numpy(X).to(DEV)
    got = kernel(Xd, p, run, gout, True, True)
    print()
    check("train %s" % (case,), got, ref32, ref64)
    again = kernel(Xd, p, run, gout, True, True)
    for k in got:
        assert np.array_equal(got[k], again[k]), "two runs differ in %s" % k
    nokeep = kernel(Xd, p, run, gout, True, False)
    assert np.array_equal(nokeep["out"], got["out"]) and np.array_equal(nokeep["stats"], got["stats"])


@pytest.mark.parametrize("case", [(1, 3, 5, 7), (33, 26, 16, 256), (65, 27, 5, 33), (1100, 1, 1, 1)],
                         ids=lambda c: "B%d-F%d-E%d-H%d" % c)
def test_eval_forward_against_float64(case):
    B, F, E, H = case
    X, p, run, gout = make(B, F, E, H, seed=7 + B + F)
    ref64, ref32 = float64(X, p, run, gout, False), torch32(X, p, run, gout, False)
    got = kernel(torch.from_numpy(X).to(DEV), p, run, gout, False, False)
    assert got["stats"].size == 0
    print()
    check("eval %s" % (case,), {"out": got["out"]}, ref32, ref64)


def test_eval_mode_has_no_backward():
    X, p, run, gout = make(3, 2, 2, 4, seed=1)
    with pytest.raises(RuntimeError, match="train=True"):
        kernel(torch.from_numpy(X).to(DEV), p, run, gout, False, True)


def test_strided_input_starting_mid_row():
    """the gathered row of a model: the view starts 3 floats into a row 11 floats wider than F * E; the gradient of the
    input comes back dense"""
    B, F, E, H = 33, 3, 5, 33
    X, p, run, gout = make(B, F, E, H, seed=11)
    wide = torch.full((B, F * E + 11), 7.0, device=DEV)
    wide[:, 3:3 + F * E] = torch.from_numpy(X).to(DEV).reshape(B, F * E)
    view = wide[:, 3:3 + F * E].view(B, F, E)
    assert not view.is_contiguous()
    got = kernel(view, p, run, gout, True, True)
    dense = kernel(torch.from_numpy(X).to(DEV), p, run, gout, True, True)
    for k in got:
        assert np.array_equal(got[k], dense[k]), k
    print()
    check("strided", got, torch32(X, p, run, gout, True), float64(X, p, run, gout, True))


def test_clamp_mask_and_sign_element_by_element():
    """|x| < 1e-7 (0, +-5e-8): the clamp is active, gradient exactly 0.  |x| == 1e-7: ``torch.clamp`` passes the gradient
    at equality, d log|x| / dx = 1 / x carries the sign of x."""
    B, F, E, H = 33, 3, 5, 7
    X, p, run, gout = make(B, F, E, H, seed=5, special=True)
    tiny = np.float32(1e-7)
    assert (X == 0).any() and (X == tiny).any() and (X == -tiny).any() and (np.abs(X) == np.float32(5e-8)).any()
    ref64, ref32 = float64(X, p, run, gout, True), torch32(X, p, run, gout, True)
    got = kernel(torch.from_numpy(X).to(DEV), p, run, gout, True, True)
    print()
    check("special", got, ref32, ref64)
    clamped = np.abs(X) < tiny
    assert np.array_equal(got["gX"] == 0, clamped) and np.array_equal(ref32["gX"] == 0, clamped)
    live = ~clamped
    assert np.array_equal(np.sign(got["gX"][live]), np.sign(ref64["gX"][live]))
    edge = np.abs(X) == tiny
    assert np.all(np.sign(got["gX"][edge]) == np.sign(ref64["gX"][edge])) and np.all(got["gX"][edge] != 0)


def test_outside_the_envelope(monkeypatch):
    from deepctr_torch._hip import lib as L
    from deepctr_torch.layers import LogTransformLayer
    lib, st = L.lib(), L.stream_handle(torch.device(DEV))
    assert lib.dctr_log_transform_workspace_floats(4, 65, 4, 8) == 0
    buf = torch.zeros(65 * 1025, device=DEV)
    q = ctypes.c_void_p(buf.data_ptr())
    for F, E, H in ((65, 4, 8), (4, 65, 8), (4, 4, 1025)):
        assert lib.dctr_log_transform_fwd_train(q, F * E, 2, F, E, H, q, q, q, q, q, q, q, E * H, q, q, st) == ENOSUP
        assert lib.dctr_log_transform_fwd_eval(q, F * E, 2, F, E, H, q, q, q, q, q, q, q, q, q, q, q, E * H, st) == ENOSUP
        assert lib.dctr_log_transform_bwd(q, F * E, 2, F, E, H, q, q, q, q, q, q, q, E * H, q, F * E, q, q, q, q, q, q, q,
                                          st) == ENOSUP
    assert lib.dctr_log_transform_fwd_train(None, 0, 0, 3, 4, 8, *([None] * 7), 0, None, None, st) == 0      # B == 0
    torch.cuda.synchronize()
    assert LogTransformLayer._kernel_fits(64, 64, 1024) and not LogTransformLayer._kernel_fits(65, 4, 8)
    taken = []
    layer = LogTransformLayer(65, 4, 8).to(DEV)
    inner = layer._torch_route
    monkeypatch.setattr(layer, "_torch_route", lambda x: taken.append(1) or inner(x))
    x = torch.randn(6, 65, 4, device=DEV) * 0.2
    out = layer(x)
    assert taken == [1] and tuple(out.shape) == (6, 32)
    ok = LogTransformLayer(3, 4, 8).to(DEV)
    monkeypatch.setattr(ok, "_torch_route", lambda x: taken.append(2))
    assert tuple(ok(torch.randn(6, 3, 4, device=DEV)).shape) == (6, 32) and taken == [1]
