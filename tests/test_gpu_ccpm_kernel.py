"""GPU: CCPM's conv stack through the C ABI (csrc/ccpm.hip: dctr_ccpm_fwd / _bwd) against float64.

k-max pooling is discontinuous in its gradient: two activations of a column closer than fp32 rounding may swap places
between two implementations, and the gradient then belongs to another element.  So nothing here depends on WHICH of two
such rows is taken.  With ``sel`` as the kernel wrote it:

  (a) the selection is a valid top-k of the float64 activations: distinct rows, every selected value >= every unselected
      value of its column - 2e-5, the output descending to the same slack;
  (b) the pooled values equal the float64 activations at ``sel`` within 1e-5 x max|ref| -- for the full stack and for every
      prefix of it (the packed parameters of the first i layers are a valid stack of their own), which is how the
      intermediate images are seen;
  (c) gE and g_params equal float64 autograd ROUTED BY THE KERNEL'S ``sel`` within 2e-5 x max|ref|;
  (d) two backward runs give identical bits;
  (e) the tie rule: constant columns select rows 0..k-1, and the gradient lands there;
  (f) B = 0 returns OK whatever the buffers, F = 65 and five layers return DCTR_ENOSUP.

The float64 side is torch on the CPU: F.pad, F.conv2d, tanh, gather.  The largest |pooled - float64| over all cases is
printed (``-s``): tools/golden/make_ccpm_golden.py's MIN_GAP must be at least 8 times that number.

Shapes, the smallest that can go wrong: F = 2 (k = 1, 1) at B = 1 and 33; F = 3; one layer of width 1 at F = 2 (k clamps to
2) and F = 5; even widths 2, 4, 6 (asymmetric padding) with D = 5; a filter wider than the image (w = 6, F = 3) with D = 6;
three layers (k = 8, 3, 3); the Criteo shape at B = 96 and 257; strided E / out / g_out; the envelope's corner F = D = 64,
w = 16; B = 4100 (more samples than workgroups: the grid-stride loop)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENOSUP = -2
SLACK, VALUE_TOL, GRAD_TOL = 2e-5, 1e-5, 2e-5
_worst = {"value": 0.0}


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*[int(v) for v in vals])


def pool_sizes(n, n_layers):
    """the k of every layer, from the function ConvLayer itself takes them from (its values are pinned below)"""
    from deepctr_torch.layers.interaction import ccpm_pool_sizes
    return ccpm_pool_sizes(n, n_layers)


def n_params_of(widths, filters):
    return sum(c * ci * w + c for c, ci, w in zip(filters, [1] + list(filters[:-1]), widths))


def unpack(params, widths, filters):
    out, off, cin = [], 0, 1
    for w, c in zip(widths, filters):
        W = params[off:off + c * cin * w].reshape(c, cin, w, 1)
        off += c * cin * w
        out.append((W, params[off:off + c]))
        off += c
        cin = c
    return out


def ref_forward(E, params, widths, filters, sels):
    """float64 torch: E [B, F, D], sels [B, C_i, k_i, D] per layer -> (pooled per layer, activations per layer)"""
    x = E[:, None]
    pooled, acts = [], []
    for (W, b), w, s in zip(unpack(params, widths, filters), widths, sels):
        top = (w - 1) // 2
        y = torch.tanh(F_.conv2d(F_.pad(x, [0, 0, top, w - 1 - top]), W, b))
        x = torch.gather(y, 2, s)
        acts.append(y)
        pooled.append(x)
    return pooled, acts


def split_sel(sel, B, filters, ks, D):
    out, off = [], 0
    for c, k in zip(filters, ks):
        out.append(sel[:, off:off + c * k * D].reshape(B, c, k, D).long())
        off += c * k * D
    return out


class Run(object):
    """One stack on one batch: device buffers, the kernel's forward (with sel) and backward."""

    def __init__(self, Fn, D, widths, filters, B, pad_e=0, pad_out=0, seed=0, zero_E=False, zero_bias_below_last=False):
        from deepctr_torch._hip import lib as L
        self.L, self.lib = L, L.lib()
        self.F, self.D, self.B, self.widths, self.filters = Fn, D, B, list(widths), list(filters)
        self.ks = pool_sizes(Fn, len(filters))
        rng = np.random.RandomState(seed)
        self.n_params = n_params_of(widths, filters)
        p, cin = [], 1
        for i, (w, c) in enumerate(zip(widths, filters)):
            lim = np.sqrt(6.0 / (cin * w + c * w))                     # xavier_uniform_, as Conv2dSame draws it
            p.append(rng.uniform(-lim, lim, c * cin * w))
            p.append(np.zeros(c) if zero_bias_below_last and i < len(filters) - 1 else rng.normal(0, 0.2, c))
            cin = c
        self.params = torch.from_numpy(np.concatenate(p).astype(np.float32)).to(DEV)
        self.ld_e = Fn * D + pad_e
        Eh = np.zeros((B, self.ld_e), np.float32) if zero_E else rng.normal(0, 0.4, (B, self.ld_e)).astype(np.float32)
        self.E = torch.from_numpy(Eh).to(DEV)
        self.n_out = filters[-1] * self.ks[-1] * D
        self.n_sel = sum(c * k for c, k in zip(filters, self.ks)) * D
        self.ld_out = self.n_out + pad_out
        self.gout = torch.from_numpy(rng.normal(0, 1, (B, self.ld_out)).astype(np.float32)).to(DEV)

    def forward(self, n_layers=None, want_sel=True):
        nl = len(self.filters) if n_layers is None else n_layers
        n_out = self.filters[nl - 1] * self.ks[nl - 1] * self.D
        n_sel = sum(c * k for c, k in zip(self.filters[:nl], self.ks[:nl])) * self.D
        ld = n_out + (self.ld_out - self.n_out)
        out = torch.full((self.B, ld), 7.0, dtype=torch.float32, device=DEV)
        sel = torch.full((self.B, n_sel), 255, dtype=torch.uint8, device=DEV) if want_sel else None
        rc = self.lib.dctr_ccpm_fwd(_ptr(self.E), self.ld_e, self.B, self.F, self.D, nl, _i32(self.widths[:nl]),
                                    _i32(self.filters[:nl]), _i32(self.ks[:nl]), _ptr(self.params), _ptr(out), ld, _ptr(sel),
                                    self.L.stream_handle(torch.device(DEV)))
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((out[:, n_out:] == 7.0).all())                     # the padding of a strided out is not written
        return out[:, :n_out].cpu(), (sel.cpu() if want_sel else None)

    def backward(self, sel):
        gE = torch.full((self.B, self.F * self.D + 3), 7.0, dtype=torch.float32, device=DEV)
        gP = torch.full((self.n_params,), 7.0, dtype=torch.float32, device=DEV)
        ws = torch.empty((max(1, self.lib.dctr_ccpm_bwd_workspace_floats(self.B, self.n_params)),), dtype=torch.float32,
                         device=DEV)
        seld = sel.to(DEV)
        rc = self.lib.dctr_ccpm_bwd(_ptr(self.E), self.ld_e, self.B, self.F, self.D, len(self.filters), _i32(self.widths),
                                    _i32(self.filters), _i32(self.ks), _ptr(self.params), _ptr(seld), _ptr(self.gout),
                                    self.ld_out, _ptr(gE), self.F * self.D + 3, _ptr(gP), _ptr(ws),
                                    self.L.stream_handle(torch.device(DEV)))
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((gE[:, self.F * self.D:] == 7.0).all())
        return gE[:, :self.F * self.D].cpu(), gP.cpu()

    def host64(self):
        E = self.E.cpu()[:, :self.F * self.D].double().reshape(self.B, self.F, self.D)
        return E, self.params.cpu().double(), self.gout.cpu()[:, :self.n_out].double()


def check_against_float64(r, sel, out, gE, gP):
    """(a), (b) for the full stack, (c)"""
    B, D = r.B, r.D
    sels = split_sel(sel, B, r.filters, r.ks, D)
    E, P, gout = r.host64()
    E.requires_grad_(True)
    P.requires_grad_(True)
    pooled, acts = ref_forward(E, P, r.widths, r.filters, sels)
    n_in = r.F
    for y, s, x, k in zip(acts, sels, pooled, r.ks):
        y, x = y.detach(), x.detach()
        assert int(s.max()) < n_in
        mask = torch.zeros_like(y, dtype=torch.bool).scatter_(2, s, True)
        assert bool((mask.sum(2) == k).all()), "a row selected twice"
        lo = torch.where(mask, y, torch.full_like(y, float("inf"))).amin(2)
        hi = torch.where(~mask, y, torch.full_like(y, -float("inf"))).amax(2)
        assert bool((lo >= hi - SLACK).all()), "not a top-k: %.3e" % float((hi - lo).max())
        if k > 1:
            assert bool((x[:, :, :-1] >= x[:, :, 1:] - SLACK).all()), "not descending"
        n_in = k
    ref = pooled[-1].detach().reshape(B, -1)
    dev = float((out.double() - ref).abs().max())
    _worst["value"] = max(_worst["value"], dev)
    assert dev <= VALUE_TOL * float(ref.abs().max()), "pooled values: %.3e" % dev
    gE_ref, gP_ref = torch.autograd.grad(pooled[-1], [E, P], gout.reshape(pooled[-1].shape))
    for name, got, want in (("gE", gE, gE_ref.reshape(B, -1)), ("g_params", gP, gP_ref)):
        err = float((got.double() - want).abs().max())
        assert err <= GRAD_TOL * float(want.abs().max()), "%s: max|d|=%.3e max|ref|=%.3g" % (name, err, want.abs().max())
    return dev


CASES = [  # F, D, widths, filters, B, pad_e, pad_out
    (2, 4, (3, 2), (2, 1), 1, 0, 0),
    (2, 4, (3, 2), (2, 1), 33, 0, 0),
    (3, 4, (3, 2), (2, 1), 33, 0, 0),
    (2, 4, (1,), (1,), 5, 0, 0),
    (5, 4, (1,), (1,), 5, 0, 0),
    (7, 5, (2, 4, 6), (2, 3, 2), 17, 0, 0),
    (3, 6, (6, 5), (4, 4), 17, 0, 0),
    (9, 4, (3, 3, 2), (3, 2, 2), 17, 0, 0),
    (26, 16, (6, 5), (4, 4), 96, 0, 0),
    (26, 16, (6, 5), (4, 4), 257, 0, 0),
    (5, 4, (3, 2), (2, 2), 33, 12, 5),
    (64, 64, (16,), (1,), 3, 0, 0),
    (2, 4, (3, 2), (2, 1), 4100, 0, 0),
]


def test_pool_sizes_are_the_cases_the_issue_names():
    assert pool_sizes(2, 2) == [1, 1] and pool_sizes(2, 1) == [2] and pool_sizes(5, 1) == [3]
    assert pool_sizes(9, 3) == [8, 3, 3] and pool_sizes(26, 2) == [13, 3] and pool_sizes(7, 3) == [6, 2, 2]
    assert pool_sizes(3, 2) == [1, 1] and pool_sizes(64, 1) == [3] and pool_sizes(26, 3) == [23, 8, 3]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "F%d-D%d-w%s-c%s-B%d%s" % (
    c[0], c[1], "x".join(map(str, c[2])), "x".join(map(str, c[3])), c[4], "-strided" if c[5] else ""))
def test_forward_and_backward_against_float64(case):
    Fn, D, widths, filters, B, pad_e, pad_out = case
    r = Run(Fn, D, widths, filters, B, pad_e, pad_out, seed=Fn * 100 + D + B)
    out, sel = r.forward()
    out_nosel, _ = r.forward(want_sel=False)
    assert torch.equal(out, out_nosel)                                  # the selection buffer is optional
    gE, gP = r.backward(sel)
    dev = check_against_float64(r, sel, out, gE, gP)
    # (b) for every prefix of the stack: the intermediate images
    for nl in range(1, len(filters)):
        o, s = r.forward(n_layers=nl)
        assert torch.equal(s, sel[:, :s.shape[1]])
        sels = split_sel(s, B, filters[:nl], r.ks[:nl], D)
        E, P, _ = r.host64()
        ref = ref_forward(E, P[:n_params_of(widths[:nl], filters[:nl])], widths[:nl], filters[:nl], sels)[0][-1]
        d = float((o.double() - ref.reshape(B, -1)).abs().max())
        _worst["value"] = max(_worst["value"], d)
        assert d <= VALUE_TOL * float(ref.abs().max())
        dev = max(dev, d)
    print("\nccpm kernel %s: max|pooled - fp64| = %.3e (largest so far %.3e)" % (case, dev, _worst["value"]))
    # (d)
    gE2, gP2 = r.backward(sel)
    assert torch.equal(gE, gE2) and torch.equal(gP, gP2)


@pytest.mark.parametrize("widths,filters,zero_bias", [((3,), (2,), False), ((3, 2), (2, 2), True)])
def test_tie_rule(widths, filters, zero_bias):
    """E = 0 (and, for two layers, no bias below the last one, so that the zero padding does not show): every column of
    every layer is constant.  sel is rows 0..k-1 in order, and the gradient lands on those rows."""
    r = Run(5, 4, widths, filters, 3, seed=5, zero_E=True, zero_bias_below_last=zero_bias)
    out, sel = r.forward()
    want = torch.cat([torch.arange(k).view(1, 1, k, 1).expand(r.B, c, k, r.D).reshape(r.B, -1)
                      for c, k in zip(filters, r.ks)], dim=1).to(torch.uint8)
    assert torch.equal(sel, want)
    gE, gP = r.backward(sel)
    check_against_float64(r, want, out, gE, gP)          # routed by rows 0..k-1, not by what the kernel reported


def test_empty_batch_and_unsupported_shapes():
    from deepctr_torch._hip import lib as L
    lib = L.lib()
    st = L.stream_handle(torch.device(DEV))
    w, c, k = _i32([3, 2]), _i32([2, 1]), _i32([1, 1])
    assert lib.dctr_ccpm_fwd(None, 0, 0, 2, 4, 2, w, c, k, None, None, 0, None, st) == 0
    assert lib.dctr_ccpm_bwd(None, 0, 0, 2, 4, 2, w, c, k, None, None, None, 0, None, 0, None, None, st) == 0
    assert lib.dctr_ccpm_bwd_workspace_floats(0, 17) == 0
    B, D = 2, 4
    E = torch.zeros((B, 65 * D), device=DEV)
    P = torch.zeros((64,), device=DEV)
    out = torch.zeros((B, 64), device=DEV)
    assert lib.dctr_ccpm_fwd(_ptr(E), 65 * D, B, 65, D, 2, w, c, _i32([32, 3]), _ptr(P), _ptr(out), 64, None, st) == ENOSUP
    w5, c5, k5 = _i32([2] * 5), _i32([1] * 5), _i32([5, 4, 3, 3, 3])
    assert lib.dctr_ccpm_fwd(_ptr(E), 65 * D, B, 6, D, 5, w5, c5, k5, _ptr(P), _ptr(out), 64, None, st) == ENOSUP
    sel = torch.zeros((B, 64), dtype=torch.uint8, device=DEV)
    ws = torch.zeros((256,), device=DEV)
    for args in ((65, 2, w, c, _i32([32, 3])), (6, 5, w5, c5, k5)):
        assert lib.dctr_ccpm_bwd(_ptr(E), 65 * D, B, args[0], D, args[1], args[2], args[3], args[4], _ptr(P), _ptr(sel),
                                 _ptr(out), 64, _ptr(E), 65 * D, _ptr(P), _ptr(ws), st) == ENOSUP
    torch.cuda.synchronize()
