"""GPU: DIN's attention pooling through the C ABI (csrc/din.hip: dctr_din_attn_fwd / _bwd) against float64.

The float64 side is torch autograd on the CPU over the layer's formula, written out here: ``[q, k, q - k, q * k]``, the hidden
layers, the 1-unit dense, ``where`` with 0 or ``-2**32 + 1``, the optional softmax, the weighted sum.

  (a) out within 1e-5 x max|ref|; gQ, gK and g_params within 2e-5 x max|ref| (each over its whole tensor);
  (b) two backward runs give identical bits;
  (c) every buffer is filled with a sentinel first: what lies outside the segments (and behind ``out``'s E floats) still
      holds it afterwards, and every element inside was written -- zeros at invalid positions included;
  (d) B = 0 returns OK whatever the buffers; T = 129, E = 65 and four hidden layers return DCTR_ENOSUP; frozen Dice has a
      forward and no backward.

Shapes, the smallest that can go wrong: B = T = E = 1 with one hidden unit; segments (8, 4) in the model's in-row layout
(Q == K, ``k_step = dim``) and an odd (5,) in the contiguous one; T = 4 with the lengths {-1, 0, 1, 3, 4, 7}; T = 17, 50, 128
(33 and more valid positions: a second pass of 32 / 16 rows); hidden (64, 16), (80, 40), (128, 128, 128), the last also at
E = 64, T = 128, the corner of the LDS budget; the mask input with empty rows; softmax on and off; every activation; strided
out / g_out / gradient rows; B = 33, 257 and 4100 (more samples than workgroups in both directions: the grid-stride loop).
The largest deviations from float64 are printed (``-s``)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENOSUP = -2
OUT_TOL, GRAD_TOL = 1e-5, 2e-5
SENT = 777.0
ACT = {"linear": 0, "relu": 1, "sigmoid": 2, "prelu": 3, "dice": 4}
_worst = {"out": 0.0, "grad": 0.0}


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _i32(v):
    return (ctypes.c_int32 * len(v))(*[int(x) for x in v])


def _i64(v):
    return (ctypes.c_int64 * len(v))(*[int(x) for x in v])


def make_params(rng, E, hidden, act):
    """(packed float32 vector, [(W, b, extra)] + dense as float64 tensors that require grad, in the packed order)"""
    parts, inn = [], 4 * E
    for H in hidden:
        parts.append(rng.normal(0, 1.0 / np.sqrt(inn), H * inn))
        parts.append(rng.normal(0, 0.2, H))
        if act == "prelu":
            parts.append(rng.normal(0.25, 0.5, 1))
        if act == "dice":
            parts += [rng.normal(0, 0.5, H), rng.uniform(0.5, 1.5, H), rng.normal(0, 0.3, H)]
        inn = H
    parts += [rng.normal(0, 1.0 / np.sqrt(inn), inn), rng.normal(0, 0.2, 1)]
    return np.concatenate(parts).astype(np.float32)


def ref_forward(q, k, valid, params, E, hidden, act, softmax):
    """float64 torch: q [B, E], k [B, T, E], valid [B, T] bool, params packed -> out [B, E]"""
    off, inn = 0, 4 * E
    qq = q[:, None, :].expand(-1, k.shape[1], -1)
    a = torch.cat([qq, k, qq - k, qq * k], dim=-1)
    for H in hidden:
        W = params[off:off + H * inn].reshape(H, inn)
        off += H * inn
        z = a @ W.t() + params[off:off + H]
        off += H
        if act == "relu":
            a = torch.relu(z)
        elif act == "sigmoid":
            a = torch.sigmoid(z)
        elif act == "prelu":
            a = torch.where(z > 0, z, params[off] * z)
            off += 1
        elif act == "dice":
            al, s, t = params[off:off + H], params[off + H:off + 2 * H], params[off + 2 * H:off + 3 * H]
            a = z * (al + (1 - al) * torch.sigmoid(s * z + t))
            off += 3 * H
        else:
            a = z
        inn = H
    score = a @ params[off:off + inn] + params[off + inn]
    assert off + inn + 1 == params.numel()
    if softmax:
        w = torch.softmax(torch.where(valid, score, torch.full_like(score, float(-2 ** 32 + 1))), dim=-1)
    else:
        w = torch.where(valid, score, torch.zeros_like(score))
    return torch.einsum("bt,bte->be", w, k)


class Case(object):
    def __init__(self, dims, T, hidden, act, softmax, B, layout="row", lens=None, use_mask=False, pad=0, seed=0):
        from deepctr_torch._hip import lib as L
        self.L, self.lib = L, L.lib()
        rng = np.random.RandomState(seed)
        self.dims, self.T, self.hidden, self.act, self.softmax, self.B = list(dims), T, list(hidden), act, softmax, B
        E = self.E = sum(dims)
        self.params_h = make_params(rng, E, hidden, act)
        if layout == "row":        # [3 other | queries | 2 other | history feature by feature | 1 other], Q == K
            self.seg_dims = list(dims)
            self.q_off, self.k_off, self.k_step, o = [], [], [], 3
            for d in dims:
                self.q_off.append(o)
                o += d
            o += 2
            for d in dims:
                self.k_off.append(o)
                self.k_step.append(d)
                o += T * d
            self.ld_q = self.ld_k = o + 1 + pad
            rows = rng.normal(0, 0.5, (B, self.ld_q)).astype(np.float32)
            self.Q = self.K = torch.from_numpy(rows).to(DEV)
        else:                      # query [B, E], keys [B, T, E]: one segment
            self.seg_dims, self.q_off, self.k_off, self.k_step = [E], [0], [0], [E]
            self.ld_q, self.ld_k = E + pad, T * E + pad
            self.Q = torch.from_numpy(rng.normal(0, 0.5, (B, self.ld_q)).astype(np.float32)).to(DEV)
            self.K = torch.from_numpy(rng.normal(0, 0.5, (B, self.ld_k)).astype(np.float32)).to(DEV)
        if use_mask:
            m = rng.rand(B, T) < 0.5
            m[0] = False
            if B > 1:
                m[1] = True
            self.valid = m
            self.len_t, self.mask_t = None, torch.from_numpy(m.astype(np.uint8)).to(DEV)
        else:
            n = rng.randint(0, T + 1, B) if lens is None else np.resize(np.asarray(lens), B)
            self.valid = np.arange(T)[None, :] < n[:, None]
            self.len_t, self.mask_t = torch.from_numpy(n.astype(np.int32)).to(DEV), None
        self.params = torch.from_numpy(self.params_h).to(DEV)
        self.ld_out = E + pad
        self.ld_g = E + pad
        self.gout = torch.from_numpy(rng.normal(0, 1.0, (B, self.ld_g)).astype(np.float32)).to(DEV)
        self.stream = L.stream_handle(torch.device(DEV))

    def _head(self):
        return (_ptr(self.Q), self.ld_q, _ptr(self.K), self.ld_k, self.B, self.T, len(self.seg_dims), _i32(self.seg_dims),
                _i64(self.q_off), _i64(self.k_off), _i64(self.k_step), _ptr(self.len_t), _ptr(self.mask_t),
                len(self.hidden), _i32(self.hidden), ACT[self.act], int(self.softmax), _ptr(self.params))

    def segments(self, rows, offs, steps, T):
        """[B, ld] host rows -> [B, T, E] (float64) and the bool map of what belongs to a segment"""
        inside = np.zeros(rows.shape[1], bool)
        parts = []
        for d, o, st in zip(self.seg_dims, offs, steps):
            parts.append(np.stack([rows[:, o + t * st:o + t * st + d] for t in range(T)], axis=1))
            for t in range(T):
                inside[o + t * st:o + t * st + d] = True
        return np.concatenate(parts, axis=-1).astype(np.float64), inside

    def forward(self, keep=True):
        self.out = torch.full((self.B, self.ld_out), SENT, dtype=torch.float32, device=DEV)
        self.wts = torch.full((self.B, self.T), SENT, dtype=torch.float32, device=DEV) if keep else None
        rc = self.lib.dctr_din_attn_fwd(*(self._head() + (_ptr(self.out), self.ld_out, _ptr(self.wts), self.stream)))
        torch.cuda.synchronize()
        return rc

    def backward(self):
        self.gQ = torch.full((self.B, self.ld_q), SENT, dtype=torch.float32, device=DEV)
        self.gK = self.gQ if self.K is self.Q else torch.full((self.B, self.ld_k), SENT, dtype=torch.float32, device=DEV)
        self.gP = torch.full((self.params.numel(),), SENT, dtype=torch.float32, device=DEV)
        n_ws = self.lib.dctr_din_attn_bwd_workspace_floats(self.B, self.params.numel())
        ws = torch.full((max(1, n_ws),), SENT, dtype=torch.float32, device=DEV)
        rc = self.lib.dctr_din_attn_bwd(*(self._head() + (_ptr(self.wts), _ptr(self.gout), self.ld_g, _ptr(self.gQ),
                                                          self.ld_q, _ptr(self.gK), self.ld_k, _ptr(self.gP), _ptr(ws),
                                                          self.stream)))
        torch.cuda.synchronize()
        return rc

    def reference(self, grad=True):
        q, self.q_in = self.segments(self.Q.cpu().numpy(), self.q_off, [0] * len(self.q_off), 1)
        k, self.k_in = self.segments(self.K.cpu().numpy(), self.k_off, self.k_step, self.T)
        q = torch.from_numpy(q[:, 0]).requires_grad_(grad)
        k = torch.from_numpy(k).requires_grad_(grad)
        p = torch.from_numpy(self.params_h.astype(np.float64)).requires_grad_(grad)
        out = ref_forward(q, k, torch.from_numpy(self.valid), p, self.E, self.hidden, self.act, self.softmax)
        if not grad:
            return out.detach().numpy(), None
        g = self.gout.cpu().numpy()[:, :self.E].astype(np.float64)
        return out.detach().numpy(), torch.autograd.grad(out, [q, k, p], torch.from_numpy(g))

    def check(self, grad=True):
        assert self.forward(keep=grad) == 0
        ref_out, grads = self.reference(grad)
        out = self.out.cpu().numpy()
        scale = max(float(np.abs(ref_out).max()), 1e-30)
        err = float(np.abs(out[:, :self.E] - ref_out).max())
        _worst["out"] = max(_worst["out"], err / scale)
        print("out: max|d| %.3e  max|ref| %.3g  (worst ratio so far %.3e)" % (err, scale, _worst["out"]))
        assert err <= OUT_TOL * scale
        assert np.all(out[:, self.E:] == SENT)
        if not grad:
            return
        w = self.wts.cpu().numpy()
        assert np.all(w[~self.valid & self.valid.any(axis=1, keepdims=True)] == 0.0)      # exactly 0 beside a valid position
        if self.softmax:
            assert np.all(w[~self.valid.any(axis=1)] == np.float32(1.0) / np.float32(self.T))
        assert self.backward() == 0
        first = [t.clone() for t in (self.gQ, self.gK, self.gP)]
        gq_ref, gk_ref, gp_ref = [t.numpy() for t in grads]
        gQ, gK = self.gQ.cpu().numpy(), self.gK.cpu().numpy()
        got_q, _ = self.segments(gQ, self.q_off, [0] * len(self.q_off), 1)
        got_k, _ = self.segments(gK, self.k_off, self.k_step, self.T)
        for name, got, ref in (("gQ", got_q[:, 0], gq_ref), ("gK", got_k, gk_ref), ("g_params", self.gP.cpu().numpy(), gp_ref)):
            sc = max(float(np.abs(ref).max()), 1e-30)
            e = float(np.abs(got - ref).max())
            _worst["grad"] = max(_worst["grad"], e / sc)
            print("%s: max|d| %.3e  max|ref| %.3g  (worst ratio so far %.3e)" % (name, e, sc, _worst["grad"]))
            assert e <= GRAD_TOL * sc, name
        # invalid positions: written, and exactly 0 unless the row is an empty softmax row
        plain = ~self.valid & (self.valid.any(axis=1, keepdims=True) | (not self.softmax))
        assert np.all(got_k[plain] == 0.0)
        # nothing outside the segments was touched
        if self.K is self.Q:
            assert np.all(gQ[:, ~(self.q_in | self.k_in)] == SENT)
        else:
            assert np.all(gQ[:, ~self.q_in] == SENT) and np.all(gK[:, ~self.k_in] == SENT)
        assert self.backward() == 0
        for a, b in zip(first, (self.gQ, self.gK, self.gP)):
            assert torch.equal(a, b)


LENS = [-1, 0, 1, 3, 4, 7]


def test_smallest_shape():
    for sm in (False, True):
        Case([1], 1, [1], "sigmoid", sm, 1, layout="contig", lens=[1]).check()
        Case([1], 1, [1], "relu", sm, 1, layout="contig", lens=[0]).check()


@pytest.mark.parametrize("act", ["linear", "relu", "sigmoid", "prelu"])
@pytest.mark.parametrize("softmax", [False, True])
def test_every_activation_in_row_layout(act, softmax):
    Case([8, 4], 4, [16, 8], act, softmax, 6, layout="row", lens=LENS, seed=1).check()


@pytest.mark.parametrize("softmax", [False, True])
def test_frozen_dice_is_forward_only(softmax):
    c = Case([8, 4], 4, [16, 8], "dice", softmax, 6, layout="row", lens=LENS, seed=2)
    c.check(grad=False)
    c.forward(keep=True)
    assert c.backward() == ENOSUP
    assert float(c.gP.min()) == SENT and float(c.gQ.min()) == SENT


@pytest.mark.parametrize("dims,T,hidden,act,softmax,B,layout", [
    ([5], 17, [64, 16], "relu", False, 33, "contig"),
    ([5], 17, [7], "prelu", True, 9, "contig"),
    ([16, 16], 50, [64, 16], "sigmoid", False, 33, "row"),
    ([16, 16], 50, [64, 16], "sigmoid", True, 9, "row"),
    ([32], 128, [80, 40], "prelu", True, 9, "contig"),
    ([8, 8, 8, 8], 128, [80, 40], "sigmoid", False, 5, "row"),
    ([8], 17, [128, 128, 128], "relu", False, 33, "contig"),
    ([64], 128, [128, 128, 128], "sigmoid", True, 3, "contig"),
    ([16, 16, 16, 16], 128, [128, 128, 128], "prelu", False, 3, "row"),
])
def test_shapes(dims, T, hidden, act, softmax, B, layout):
    c = Case(dims, T, hidden, act, softmax, B, layout=layout, seed=3)
    if B >= 3:          # an empty, a one-position and a full row in every batch
        n = c.len_t.cpu().numpy()
        n[:3] = [0, 1, T]
        c.len_t = torch.from_numpy(n).to(DEV)
        c.valid = np.arange(T)[None, :] < n[:, None]
    c.check()


@pytest.mark.parametrize("softmax", [False, True])
@pytest.mark.parametrize("layout", ["contig", "row"])
def test_mask_input(softmax, layout):
    Case([8, 4], 17, [16, 8], "sigmoid", softmax, 12, layout=layout, use_mask=True, seed=4).check()


@pytest.mark.parametrize("layout", ["contig", "row"])
def test_strided_out_and_gradients(layout):
    Case([8, 4], 4, [16, 8], "relu", True, 7, layout=layout, lens=LENS, pad=5, seed=5).check()


@pytest.mark.parametrize("B", [33, 257, 4100])
def test_batch_sizes(B):
    Case([8, 4], 4, [8, 4], "sigmoid", B == 257, B, layout="row", seed=6).check()


def test_empty_batch_and_envelope():
    from deepctr_torch._hip import lib as L
    lib = L.lib()
    tail = (None, 4, None, L.stream_handle(torch.device(DEV)))
    head = lambda T, dims, hidden: (None, 0, None, 0, 0, T, len(dims), _i32(dims), _i64([0] * len(dims)),     # noqa: E731
                                    _i64([0] * len(dims)), _i64(dims), None, None, len(hidden), _i32(hidden), 2, 0, None)
    assert lib.dctr_din_attn_fwd(*(head(4, [4], [8, 4]) + tail)) == 0
    assert lib.dctr_din_attn_fwd(*(head(129, [4], [8, 4]) + tail)) == 0          # B == 0 comes first
    gp = torch.full((4 * 4 * 8 + 8 + 8 * 4 + 4 + 4 + 1,), SENT, dtype=torch.float32, device=DEV)
    assert lib.dctr_din_attn_bwd(*(head(4, [4], [8, 4]) + (None, None, 4, None, 4, None, 16, _ptr(gp), None,
                                                         L.stream_handle(torch.device(DEV))))) == 0
    torch.cuda.synchronize()
    assert float(gp.abs().max()) == 0.0
    assert lib.dctr_din_attn_supported(128, 1, _i32([64]), 3, _i32([128, 128, 128]), 3) == 1
    for T, dims, hidden in ((129, [4], [8, 4]), (4, [65], [8, 4]), (4, [33, 32], [8]), (4, [4], [8, 4, 4, 4]), (4, [4], [129])):
        assert lib.dctr_din_attn_supported(T, len(dims), _i32(dims), len(hidden), _i32(hidden), 2) == 0
        c = Case([4], 4, [8, 4], "sigmoid", False, 2, layout="contig")
        c.T, c.seg_dims, c.hidden = T, dims, hidden
        c.q_off, c.k_off, c.k_step = [0] * len(dims), [0] * len(dims), list(dims)
        c.out = torch.full((2, 80), SENT, dtype=torch.float32, device=DEV)
        rc = lib.dctr_din_attn_fwd(*(c._head() + (_ptr(c.out), 80, None, c.stream)))
        torch.cuda.synchronize()
        assert rc == ENOSUP and float(c.out.min()) == SENT


def test_zz_report():
    print("largest |out - float64| / max|ref| = %.3e, largest gradient deviation / max|ref| = %.3e" %
          (_worst["out"], _worst["grad"]))
