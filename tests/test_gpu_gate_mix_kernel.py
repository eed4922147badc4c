"""GPU: the gate mix through the C ABI (csrc/gate_mix.hip: dctr_gate_mix_fwd / _bwd) against float64 torch autograd on the
CPU of the reference's formulation, per gate

    matmul(softmax(h @ W.T, 1).unsqueeze(1), stack(members, 1)).squeeze(1)

Values (out, w) within 1e-5 x max|ref|, gradients (g_x, g_h, gW) within 2e-5 x max|ref|: the project's tolerances against
float64 (tests/test_gpu_ccpm_kernel.py, tests/test_gpu_din_kernel.py).  ``-s`` prints the largest deviation seen, relative
to its bound.

Every buffer the kernels read or write row by row is STRIDED here (a leading dimension larger than the row) and the padding
is filled with a sentinel that must be unchanged afterwards; gW keeps the weight's leading dimension and its padding
columns must come back 0.  Shapes, the smallest at which it can go wrong: the minimal call; n = 1; odd dim / H (5, 65, 130 /
3, 64, 67, 300: below, at and above one 64-lane pass); MMOE's pattern (every gate over the whole pool) and PLE's (a pool of
5, gates over {0,1,4}, {2,3,4}, {0..4}: an expert's gradient is a sum over gates); two gates reading one h; a NULL gate
gradient; logits of +-100; B = 33, 257, 4100 (4100 samples on at most 4096 waves: the forward's grid-stride loop and more than
one sample per wave in the backward); the envelope's corner G = 8, n = 16, P = 32, dim = H = 1152; two backward runs with
identical bits; B = 0; every refusal."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, ENOSUP = -1, -2
VALUE_TOL, GRAD_TOL = 1e-5, 2e-5
SENTINEL = -777.25
_worst = {"value": 0.0, "grad": 0.0}


def _lib():
    from deepctr_torch._hip import lib as L
    return L, L.lib()


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*[int(v) for v in vals])


def strided(B, n, pad, fill=None, gen=None, scale=1.0):
    """-> (the [B, n] view, its [B, n + pad] buffer): random values (or ``fill``) in the view, SENTINEL in the padding"""
    buf = torch.full((B, n + pad), SENTINEL, dtype=torch.float32)
    if fill is None:
        buf[:, :n] = torch.randn(B, n, generator=gen) * scale
    else:
        buf[:, :n] = fill
    buf = buf.to(DEV)
    return buf[:, :n], buf


def padding_intact(buf, n):
    return buf.shape[1] == n or bool((buf[:, n:] == SENTINEL).all())


class Case(object):
    """One pool, its gates, and the kernels' results.  ``shared_h``: {gate: earlier gate whose h tensor it reads}."""

    def __init__(self, B, P, dim, gates, pad=3, seed=0, scale=1.0, null=(), shared_h=None, w_scale=None):
        L, lib = _lib()
        self.L, self.lib = L, lib
        gen = torch.Generator().manual_seed(seed)
        self.B, self.P, self.dim, self.G, self.null, self.pad = B, P, dim, len(gates), set(null), pad
        self.members = [list(m) for m, _ in gates]
        self.H = [H for _, H in gates]
        self.x = [strided(B, dim, pad, gen=gen) for _ in range(P)]
        self.h = []
        for g, H in enumerate(self.H):
            src = (shared_h or {}).get(g)
            self.h.append(self.h[src] if src is not None else strided(B, H, pad, gen=gen, scale=scale))
        self.W = [strided(len(m), H, pad, gen=gen, scale=(w_scale if w_scale is not None else 1.0 / np.sqrt(H)))
                  for m, H in gates]
        self.out = [strided(B, dim, pad, fill=0.0) for _ in range(self.G)]
        self.w = [torch.full((B, len(m)), SENTINEL, dtype=torch.float32, device=DEV) for m in self.members]
        self.gout = [None if g in self.null else strided(B, dim, pad, gen=gen) for g in range(self.G)]
        self.gx = [strided(B, dim, pad, fill=0.0) for _ in range(P)]
        self.gh = [strided(B, H, pad, fill=0.0) for H in self.H]
        self.gW = [torch.full((len(m), H + pad), SENTINEL, dtype=torch.float32, device=DEV) for m, H in gates]

    def descriptors(self):
        gates = (self.L.Gate * self.G)()
        for g, q in enumerate(gates):
            q.h, q.ld_h, q.H = self.h[g][0].data_ptr(), self.h[g][1].shape[1], self.H[g]
            q.W, q.ld_w, q.n = self.W[g][0].data_ptr(), self.W[g][1].shape[1], len(self.members[g])
            q.out, q.ld_out = self.out[g][0].data_ptr(), self.out[g][1].shape[1]
            q.w = self.w[g].data_ptr()
            if self.gout[g] is not None:
                q.g_out, q.ld_gout = self.gout[g][0].data_ptr(), self.gout[g][1].shape[1]
            q.g_h, q.ld_gh = self.gh[g][0].data_ptr(), self.gh[g][1].shape[1]
            q.gW = self.gW[g].data_ptr()
            for j, e in enumerate(self.members[g]):
                q.member[j] = e
        return gates

    def pool(self, which):
        return (ctypes.c_void_p * self.P)(*[v.data_ptr() for v, _ in which]), \
            (ctypes.c_int64 * self.P)(*[b.shape[1] for _, b in which])

    def forward(self):
        xp, xl = self.pool(self.x)
        rc = self.lib.dctr_gate_mix_fwd(xp, xl, self.P, self.dim, self.B, self.descriptors(), self.G, None)
        torch.cuda.synchronize()
        return rc

    def backward(self):
        xp, xl = self.pool(self.x)
        gp, gl = self.pool(self.gx)
        n = self.lib.dctr_gate_mix_bwd_workspace_floats(self.B, self.G, _i32([len(m) for m in self.members]),
                                                        _i32([b.shape[1] for _, b in self.W]))
        ws = torch.empty((max(1, n),), dtype=torch.float32, device=DEV)
        rc = self.lib.dctr_gate_mix_bwd(xp, xl, self.P, self.dim, self.B, self.descriptors(), self.G, gp, gl,
                                        ctypes.c_void_p(ws.data_ptr()), None)
        torch.cuda.synchronize()
        return rc

    def reference(self):
        """float64 autograd on the CPU -> (outs, ws, g_x, g_h per gate, gW per gate)"""
        x = [v.cpu().double().requires_grad_() for v, _ in self.x]
        hs = [v.cpu().double().requires_grad_() for v, _ in self.h]       # one leaf PER GATE, shared tensors included
        Ws = [v.cpu().double().requires_grad_() for v, _ in self.W]
        outs, ws = [], []
        for g in range(self.G):
            w = torch.softmax(hs[g] @ Ws[g].T, 1)
            outs.append(torch.matmul(w.unsqueeze(1), torch.stack([x[e] for e in self.members[g]], 1)).squeeze(1))
            ws.append(w)
        live = [g for g in range(self.G) if g not in self.null]
        torch.autograd.backward([outs[g] for g in live], [self.gout[g][0].cpu().double() for g in live])
        zero = torch.zeros_like
        return outs, ws, [t.grad if t.grad is not None else zero(t) for t in x], \
            [t.grad if t.grad is not None else zero(t) for t in hs], [t.grad if t.grad is not None else zero(t) for t in Ws]

    def check(self):
        assert self.forward() == 0
        assert self.backward() == 0
        outs, ws, gx, gh, gW = self.reference()
        for g in range(self.G):
            close(self.out[g][0], outs[g], VALUE_TOL, "value", "out[%d]" % g)
            close(self.w[g], ws[g], VALUE_TOL, "value", "w[%d]" % g)
            close(self.gh[g][0], gh[g], GRAD_TOL, "grad", "g_h[%d]" % g)
            H = self.H[g]
            close(self.gW[g][:, :H], gW[g], GRAD_TOL, "grad", "gW[%d]" % g)
            assert bool((self.gW[g][:, H:] == 0).all()), "gW[%d]: padding columns are not 0" % g
            if g in self.null:
                assert float(self.gh[g][0].abs().max()) == 0.0 and float(self.gW[g].abs().max()) == 0.0
            assert padding_intact(self.out[g][1], self.dim) and padding_intact(self.gh[g][1], H)
            assert padding_intact(self.h[g][1], H) and padding_intact(self.W[g][1], H)
        for e in range(self.P):
            close(self.gx[e][0], gx[e], GRAD_TOL, "grad", "g_x[%d]" % e)
            assert padding_intact(self.gx[e][1], self.dim) and padding_intact(self.x[e][1], self.dim)
        assert all(torch.isfinite(o[0]).all() for o in self.out)
        return self


def close(got, ref, tol, kind, what):
    got, ref = got.detach().cpu().double(), ref.detach().double()
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    if scale > 0:
        _worst[kind] = max(_worst[kind], err / (tol * scale))
    assert err <= tol * scale, "%s: max|d| = %.3e, max|ref| = %.3g" % (what, err, scale)


def teardown_module(module):
    print("\ngate mix: largest deviation / bound: values %.3f, gradients %.3f" % (_worst["value"], _worst["grad"]))


ALL3 = (0, 1, 2)
PLE = [((0, 1, 4), 8), ((2, 3, 4), 8), ((0, 1, 2, 3, 4), 8)]


def test_minimal():
    Case(B=1, P=2, dim=1, gates=[((0, 1), 1)], pad=0).check()


def test_single_member_has_weight_one_and_no_gate_gradient():
    c = Case(B=9, P=2, dim=5, gates=[((1,), 6), ((0, 1), 6)]).check()
    assert bool((c.w[0] == 1).all())
    assert float(c.gh[0][0].abs().max()) == 0.0 and float(c.gW[0].abs().max()) == 0.0
    assert torch.equal(c.out[0][0], c.x[1][0])


@pytest.mark.parametrize("dim", [5, 65, 130])
@pytest.mark.parametrize("H", [3, 64, 67, 300])
def test_odd_sizes_strided(dim, H):
    Case(B=7, P=3, dim=dim, gates=[(ALL3, H), ((2, 0), H)], pad=3, seed=dim + H).check()


def test_mmoe_pattern():
    Case(B=33, P=3, dim=16, gates=[(ALL3, 8)] * 3).check()


def test_ple_pattern_sums_an_experts_gradient_over_gates():
    c = Case(B=33, P=5, dim=16, gates=PLE).check()
    # expert 4 is mixed by all three gates: its gradient is the sum, in gate order, of the three shares
    w = [c.w[g].double() for g in range(3)]
    want = w[0][:, 2:3] * c.gout[0][0].double() + w[1][:, 2:3] * c.gout[1][0].double() + w[2][:, 4:5] * c.gout[2][0].double()
    close(c.gx[4][0], want.cpu(), GRAD_TOL, "grad", "g_x[4] as a sum over gates")


def test_repeated_member_gets_both_shares():
    Case(B=5, P=2, dim=7, gates=[((0, 1, 0), 4)]).check()


def test_aliased_gate_input_gets_one_gradient_buffer_per_gate():
    c = Case(B=17, P=3, dim=8, gates=[(ALL3, 12), (ALL3, 12)], shared_h={1: 0}).check()
    assert c.h[0][0].data_ptr() == c.h[1][0].data_ptr() and c.gh[0][0].data_ptr() != c.gh[1][0].data_ptr()
    assert not torch.equal(c.gh[0][0], c.gh[1][0])


@pytest.mark.parametrize("null", [(2,), (0, 1)])
def test_null_gate_gradient(null):
    Case(B=33, P=5, dim=16, gates=PLE, null=null).check()


def test_all_gate_gradients_null_writes_zeros():
    c = Case(B=6, P=3, dim=4, gates=[(ALL3, 4)], null=(0,))
    assert c.forward() == 0 and c.backward() == 0
    assert all(float(v.abs().max()) == 0.0 for v, _ in c.gx) and float(c.gW[0].abs().max()) == 0.0


def test_large_logits_are_stable():
    c = Case(B=33, P=4, dim=9, gates=[((0, 1, 2, 3), 16), ((3, 1), 16)], scale=25.0, w_scale=1.0).check()
    z = c.h[0][0].cpu().double() @ c.W[0][0].cpu().double().T
    assert float(z.abs().max()) > 100.0
    assert all(torch.isfinite(w).all() for w in c.w)


@pytest.mark.parametrize("B", [33, 257, 4100])
def test_batch_sizes(B):
    Case(B=B, P=3, dim=16, gates=[(ALL3, 8), (ALL3, 8)], seed=B).check()


def test_envelope_corner():
    L, lib = _lib()
    P, G, n, wide = L.GATE_MAX_POOL, L.GATE_MAX_GATES, L.GATE_MAX_MEMBERS, L.GATE_MAX_WIDTH
    assert (P, G, n, wide) == (32, 8, 16, 1152)
    gates = [(tuple((g * 3 + j * 2) % P for j in range(n)), wide) for g in range(G)]
    assert lib.dctr_gate_mix_supported(P, wide, G, _i32([n] * G), _i32([wide] * G)) == 1
    Case(B=5, P=P, dim=wide, gates=gates, pad=1).check()


def test_backward_is_deterministic():
    c = Case(B=4100, P=5, dim=16, gates=PLE, seed=3)
    assert c.forward() == 0 and c.backward() == 0
    first = [t.clone() for t in c.gW] + [v.clone() for v, _ in c.gx] + [v.clone() for v, _ in c.gh]
    for t in c.gW:
        t.fill_(SENTINEL)
    assert c.backward() == 0
    again = list(c.gW) + [v for v, _ in c.gx] + [v for v, _ in c.gh]
    assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_empty_batch_touches_nothing():
    L, lib = _lib()
    gates = (L.Gate * 1)()          # no buffer at all
    assert lib.dctr_gate_mix_fwd(None, None, 3, 8, 0, gates, 1, None) == 0
    assert lib.dctr_gate_mix_bwd(None, None, 3, 8, 0, gates, 1, None, None, None, None) == 0
    assert lib.dctr_gate_mix_bwd_workspace_floats(0, 1, _i32([3]), _i32([8])) == 0


def test_refusals():
    L, lib = _lib()
    ok = dict(P=3, dim=8, G=2, n=[3, 2], H=[8, 8])

    def supported(**kw):
        a = dict(ok, **kw)
        return lib.dctr_gate_mix_supported(a["P"], a["dim"], a["G"], _i32(a["n"]), _i32(a["H"]))
    assert supported() == 1
    assert supported(P=33) == 0 and supported(dim=1153) == 0 and supported(n=[17, 2]) == 0 and supported(H=[8, 1153]) == 0
    assert supported(G=9, n=[2] * 9, H=[8] * 9) == 0
    assert supported(P=32, dim=1152, n=[16, 1], H=[1152, 1]) == 1
    # the entry points refuse the same shapes, forward and backward, before they look at a buffer's contents
    for kw in (dict(P=33), dict(dim=1153), dict(n=17), dict(H=1153), dict(G=9)):
        P, dim, G = kw.get("P", 3), kw.get("dim", 8), kw.get("G", 1)
        n, H = kw.get("n", 2), kw.get("H", 8)
        c = Case(B=2, P=P, dim=dim, gates=[(tuple(j % P for j in range(min(n, 16))), H)] * min(G, 8), pad=0)
        gates = (L.Gate * G)()
        for g, q in enumerate(c.descriptors()):
            ctypes.memmove(ctypes.byref(gates[g]), ctypes.byref(q), ctypes.sizeof(L.Gate))
            gates[g].n = n          # (17: one more than a descriptor can list)
        if G > 8:
            ctypes.memmove(ctypes.byref(gates[8]), ctypes.byref(gates[0]), ctypes.sizeof(L.Gate))
        xp, xl = c.pool(c.x)
        gp, gl = c.pool(c.gx)
        ws = torch.empty((1 << 16,), dtype=torch.float32, device=DEV)
        assert lib.dctr_gate_mix_fwd(xp, xl, P, dim, 2, gates, G, None) == ENOSUP, kw
        assert lib.dctr_gate_mix_bwd(xp, xl, P, dim, 2, gates, G, gp, gl, ctypes.c_void_p(ws.data_ptr()), None) == ENOSUP, kw
    torch.cuda.synchronize()
    # inconsistent arguments are invalid, not unsupported
    c = Case(B=2, P=3, dim=8, gates=[(ALL3, 8)], pad=0)
    gates = c.descriptors()
    gates[0].member[1] = 3
    xp, xl = c.pool(c.x)
    assert lib.dctr_gate_mix_fwd(xp, xl, 3, 8, 2, gates, 1, None) == EINVAL
    gates = c.descriptors()
    gates[0].ld_h = 4
    assert lib.dctr_gate_mix_fwd(xp, xl, 3, 8, 2, gates, 1, None) == EINVAL
