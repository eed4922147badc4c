"""GPU: DIEN's recurrences through the C ABI (csrc/gru_seq.hip: dctr_gru_seq_fwd / _bwd) against float64.

The float64 side is torch autograd on the CPU over the cell loop of tests/dien_helpers.py (``recurrence``), computed once
per case and shared.  The inputs are those tests/test_dien_host.py has shown float32 arithmetic itself to hold within a
quarter of the tolerances.

  (a) states and last within 1e-5 x max|ref|; gX, g_att and g_params within 2e-5 x max|ref| (each over its whole tensor);
  (b) two backward runs give identical bits;
  (c) every buffer is filled with a sentinel first: what lies outside the segments (and behind a row's T*H / H floats)
      still holds it afterwards, and every element inside was written -- padded ``states`` and the invalid positions of gX
      and g_att are exactly 0, and so are AGRU's z rows of g_params;
  (d) the forward with only the outputs asked for (no gates) gives the bits of the one a backward follows;
  (e) B = 0 returns OK whatever the buffers; H = 65, T = 129 and 5 segments return DCTR_ENOSUP, a missing att in modes 1
      to 3 is refused.

Shapes (tests/dien_helpers.py, CASES), the smallest that can go wrong: B = T = H = 1 in every mode; H = 5 (one padded tile
of 16), 12 as segments 8 + 4 read in place from a wider row, 33 (padded to 64), 32 and 64; T = 1, 4, 7, 50, 128 with the
corner H 64 / T 128 at B = 48; the lengths {-1, 0, 1, 3, T-1, T, T+3}; a whole tile of length 0 next to one of length T; only
zero lengths; B = 4100 at H 12 / T 6 (a last tile of 4 samples; 257 forward and 129 backward tiles, one per workgroup) and at
H 33 / T 3 (513 backward tiles of 8 over 512 workgroups: the grid-stride loop, with the weight and bias gradients carried
from a workgroup's first tile into its second); states only, last only, both; strided states.  The largest deviations
from float64 are printed (``-s``)."""
import ctypes

import numpy as np
import pytest
import torch

import dien_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENOSUP = -2
SENT = 777.0
_worst = {}


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _i32(v):
    return (ctypes.c_int32 * len(v))(*[int(x) for x in v])


def _i64(v):
    return (ctypes.c_int64 * len(v))(*[int(x) for x in v])


def _sent(*shape):
    return torch.full(shape, SENT, dtype=torch.float32, device=DEV)


class Run(object):
    """one case on the GPU: the operands laid out as the case asks, both directions, everything back on the host"""

    def __init__(self, name):
        from deepctr_torch._hip import lib as L
        self.L, self.lib = L, L.lib()
        c = self.c = H.CASES[name]
        a = self.a = H.case_inputs(c)
        dims, T, B = c["dims"], c["T"], c["B"]
        Hd = self.H = sum(dims)
        self.n = np.clip(a["lens"].astype(np.int64), 0, T)
        if c["layout"] == "row":       # [3 other | segment 0, T positions | 2 other | segment 1 | ... | 1 other + 4 pad]
            self.x_off, self.x_step, o = [], [], 3
            for d in dims:
                self.x_off.append(o)
                self.x_step.append(d)
                o += T * d + 2
            self.ld_x = o + 3
        else:
            self.x_off, self.x_step, self.ld_x = [0], [Hd], T * Hd
            dims = (Hd,)
        self.seg_dims = list(dims)
        rows = np.random.RandomState(5).normal(0, 1, (B, self.ld_x)).astype(np.float32)
        e = 0
        for d, o, st in zip(self.seg_dims, self.x_off, self.x_step):
            for t in range(T):
                rows[:, o + t * st:o + t * st + d] = a["x"][:, t, e:e + d]
            e += d
        self.inside = np.zeros(self.ld_x, bool)
        for d, o, st in zip(self.seg_dims, self.x_off, self.x_step):
            for t in range(T):
                self.inside[o + t * st:o + t * st + d] = True
        self.X = torch.from_numpy(rows).to(DEV)
        self.att = torch.from_numpy(a["att"]).to(DEV) if c["mode"] else None
        self.lens = torch.from_numpy(a["lens"]).to(DEV)
        self.params = torch.from_numpy(a["params"]).to(DEV)
        self.ld_s, self.ld_l = T * Hd + c["ld_extra"], Hd + c["ld_extra"]
        self.want_s, self.want_l = c["outputs"] in ("both", "states"), c["outputs"] in ("both", "last")

    def _fwd(self, states, last, gates):
        c = self.c
        return self.lib.dctr_gru_seq_fwd(_ptr(self.X), self.ld_x, c["B"], c["T"], len(self.seg_dims), _i32(self.seg_dims),
                                         _i64(self.x_off), _i64(self.x_step), _ptr(self.lens), _ptr(self.att), c["mode"],
                                         _ptr(self.params), _ptr(states), self.ld_s, _ptr(last), self.ld_l, _ptr(gates),
                                         self.L.stream_handle(torch.device(DEV)))

    def forward(self):
        c, B, T, Hd = self.c, self.c["B"], self.c["T"], self.H
        # as a prediction asks for it: only the wanted outputs, no gates
        s0 = _sent(B, self.ld_s) if self.want_s else None
        l0 = _sent(B, self.ld_l) if self.want_l else None
        assert self._fwd(s0, l0, None) == 0
        # as a training step asks for it
        self.states, self.last, self.gates = _sent(B, self.ld_s), _sent(B, self.ld_l), _sent(B, T, 4, Hd)
        assert self._fwd(self.states, self.last, self.gates) == 0
        torch.cuda.synchronize()
        if s0 is not None:
            assert torch.equal(s0, self.states)
        if l0 is not None:
            assert torch.equal(l0, self.last)
        s, la = self.states.cpu().numpy(), self.last.cpu().numpy()
        assert (s[:, T * Hd:] == SENT).all() and (la[:, Hd:] == SENT).all()
        return s[:, :T * Hd].reshape(B, T, Hd), la[:, :Hd]

    def backward(self):
        c, B, T, Hd = self.c, self.c["B"], self.c["T"], self.H
        gs = gl = None
        if self.want_s:
            gs = _sent(B, self.ld_s)
            gs[:, :T * Hd] = torch.from_numpy(self.a["g_states"].reshape(B, T * Hd)).to(DEV)
        if self.want_l:
            gl = _sent(B, self.ld_l)
            gl[:, :Hd] = torch.from_numpy(self.a["g_last"]).to(DEV)
        ws = torch.empty((max(1, self.lib.dctr_gru_seq_bwd_workspace_floats(B, Hd)),), dtype=torch.float32, device=DEV)
        outs = []
        for _ in range(2):
            gX, gA, gP = _sent(B, self.ld_x), (_sent(B, T) if c["mode"] else None), _sent(6 * Hd * Hd + 6 * Hd)
            ws.fill_(SENT)
            rc = self.lib.dctr_gru_seq_bwd(_ptr(self.X), self.ld_x, B, T, len(self.seg_dims), _i32(self.seg_dims),
                                           _i64(self.x_off), _i64(self.x_step), _ptr(self.lens), _ptr(self.att), c["mode"],
                                           _ptr(self.params), _ptr(self.states), self.ld_s, _ptr(self.gates), _ptr(gs),
                                           self.ld_s, _ptr(gl), self.ld_l, _ptr(gX), self.ld_x, _ptr(gA), _ptr(gP), _ptr(ws),
                                           self.L.stream_handle(torch.device(DEV)))
            assert rc == 0
            torch.cuda.synchronize()
            outs.append((gX.cpu().numpy(), gA.cpu().numpy() if gA is not None else None, gP.cpu().numpy()))
        (gX, gA, gP), (gX2, gA2, gP2) = outs
        assert np.array_equal(gX, gX2) and np.array_equal(gP, gP2) and (gA is None or np.array_equal(gA, gA2))   # (b)
        assert (gX[:, ~self.inside] == SENT).all()                                                              # (c)
        gx = np.zeros((B, T, Hd), np.float32)
        e = 0
        for d, o, st in zip(self.seg_dims, self.x_off, self.x_step):
            for t in range(T):
                gx[:, t, e:e + d] = gX[:, o + t * st:o + t * st + d]
            e += d
        return gx, gA, gP


def _check(name):
    r = Run(name)
    c, ref, T, Hd = r.c, H.reference(name), r.c["T"], r.H
    states, last = r.forward()
    gx, ga, gp = r.backward()
    pad = np.arange(T)[None, :] >= r.n[:, None]
    assert not states[pad].any() and not gx[pad].any()                     # exact zeros, and nothing left of the sentinel
    assert not last[r.n == 0].any()
    got = dict(states=states, last=last, gx=gx, g_params=gp)
    if c["mode"]:
        assert not ga[pad].any()
        got["g_att"] = ga
    if c["mode"] == 2:                                                     # AGRU does not use z
        for W in (gp[:3 * Hd * Hd].reshape(3 * Hd, Hd), gp[3 * Hd * Hd:6 * Hd * Hd].reshape(3 * Hd, Hd)):
            assert not W[Hd:2 * Hd].any()
        assert not gp[6 * Hd * Hd + Hd:6 * Hd * Hd + 2 * Hd].any() and not gp[6 * Hd * Hd + 4 * Hd:6 * Hd * Hd + 5 * Hd].any()
    dev = H.deviations(got, ref)
    for k, (err, scale) in dev.items():
        rel = err / scale if scale else 0.0
        _worst[k] = max(_worst.get(k, 0.0), rel)
        print("%-16s %-9s max|d|=%.3e max|ref|=%.3g (%.2e of it; worst so far %.2e)" % (name, k, err, scale, rel, _worst[k]))
    for k, (err, scale) in dev.items():
        assert err <= H.BOUNDS[k] * scale, "%s %s: %.3e against %.3g" % (name, k, err, scale)
    return r, got


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_case_matches_float64(name):
    _check(name)


def test_only_zero_lengths_give_exact_zeros():
    r, got = _check("allzero")
    for k, v in got.items():
        assert not np.asarray(v).any(), k


def test_b0_returns_ok_before_any_buffer_check():
    from deepctr_torch._hip import lib as L
    lib = L.lib()
    st = L.stream_handle(torch.device(DEV))
    assert lib.dctr_gru_seq_fwd(None, 0, 0, 4, 1, _i32([3]), _i64([0]), _i64([3]), None, None, 0, None, None, 0, None, 0,
                                None, st) == 0
    gp = _sent(6 * 9 + 18)
    assert lib.dctr_gru_seq_bwd(None, 0, 0, 4, 1, _i32([3]), _i64([0]), _i64([3]), None, None, 0, None, None, 0, None, None,
                                0, None, 0, None, 0, None, _ptr(gp), None, st) == 0
    torch.cuda.synchronize()
    assert not gp.cpu().numpy().any()


def test_refusals():
    from deepctr_torch._hip import lib as L
    lib = L.lib()
    st = L.stream_handle(torch.device(DEV))
    assert lib.dctr_gru_seq_supported(128, 4, _i32([16, 16, 16, 16]), 3) == 1
    assert lib.dctr_gru_seq_supported(4, 1, _i32([65]), 0) == 0
    assert lib.dctr_gru_seq_supported(129, 1, _i32([4]), 0) == 0
    assert lib.dctr_gru_seq_supported(4, 5, _i32([1, 1, 1, 1, 1]), 0) == 0
    assert lib.dctr_gru_seq_bwd_workspace_floats(4100, 12) >= 6 * 144 + 72 and lib.dctr_gru_seq_bwd_workspace_floats(0, 12) == 0

    def fwd(T, dims, mode, att):
        Hd, B = sum(dims), 2
        X = torch.zeros((B, T * Hd), dtype=torch.float32, device=DEV)
        off, o = [], 0
        for d in dims:
            off.append(o)
            o += d
        p = torch.zeros((6 * Hd * Hd + 6 * Hd,), dtype=torch.float32, device=DEV)
        n = torch.ones((B,), dtype=torch.int32, device=DEV)
        last = _sent(B, Hd)
        a = torch.zeros((B, T), dtype=torch.float32, device=DEV) if att else None
        rc = lib.dctr_gru_seq_fwd(_ptr(X), T * Hd, B, T, len(dims), _i32(dims), _i64(off), _i64([Hd] * len(dims)), _ptr(n),
                                  _ptr(a), mode, _ptr(p), None, 0, _ptr(last), Hd, None, st)
        torch.cuda.synchronize()
        return rc, last.cpu().numpy()
    for T, dims in ((4, [65]), (129, [4]), (4, [1, 1, 1, 1, 1])):
        rc, last = fwd(T, dims, 0, False)
        assert rc == ENOSUP and (last == SENT).all()
    for mode in (1, 2, 3):
        rc, last = fwd(4, [4], mode, False)
        assert rc != 0 and (last == SENT).all()
        assert fwd(4, [4], mode, True)[0] == 0
