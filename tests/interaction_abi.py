"""Driver for the older interaction kernels THROUGH THE C ABI (include/dctr.h: dctr_fm_*, dctr_bi_pooling_*,
dctr_inner_product_*, dctr_senet_*, dctr_afm_*, dctr_interacting_*, dctr_crossnet_vec_*), shared by
tests/test_interaction_abi_host.py (over the stand-in library, on the CPU) and tests/test_gpu_interaction_abi.py (on the
device).  Not a test file.

A ``Case`` takes the library object and a device.  Every row buffer has ``pad`` extra floats behind each row (the leading
dimension the entry point is given is ``columns + pad``); every buffer an entry point writes is filled with a sentinel
first, the workspace too; flat parameter gradients get ``GUARD`` sentinel floats behind them.  ``check()`` asserts

  (a) values within ``OUT_TOL x max(1, max|ref|)``, gradients within ``GRAD_TOL x`` the same (CrossNet ``g_kernels``:
      ``GK_TOL``) -- the bounds of tests/test_gpu_pairwise.py -- against float64 on the CPU: oracle/np_oracle.py where it has
      the op (fm_*, inner_product_* with the sum, crossnet_*, senet_*, interacting_*), else torch.float64 autograd over the
      formula include/dctr.h states (BiInteraction, the un-reduced products, AFM);
  (b) every float outside the documented columns still holds the sentinel, and so do the padded floats of the inputs;
  (c) a second backward gives identical bits (whole buffers);
  (d) ``dctr_fm_bwd`` with ``accumulate = 1`` adds to a pre-filled ``gE``.

``case.nB`` is the batch the entry points are TOLD (default: the rows the buffers have): ``nB = 0`` is the empty-batch call
on valid one-row buffers.  ``case.tol[name]`` overrides a bound for one tensor; ``WORST`` collects the largest
``max|d| / max(1, max|ref|)`` per (op, tensor).

The CIN layer, its pooling glue, the two row products and the matrix CrossNet (dctr_cin_layer_*, dctr_cin_pool_*,
dctr_rows_dot, dctr_rows_tdot, dctr_crossnet_mat_*: ``NEW_OPS``) run under the same rules with these differences:

  scale       the deviation is divided by ``max|ref|`` of the tensor, NOT ``max(1, max|ref|)`` (a CIN output is of order
              0.1); the bounds stay OUT_TOL / GRAD_TOL / GK_TOL (the matrix CrossNet's gW).  A tensor whose reference is
              identically zero must come back exactly zero.
  relu mask   dctr_cin_layer_bwd / dctr_cin_pool_bwd are handed the float64 forward rounded to float32 as the saved
              activation, and the reference gradient uses that same mask (A32 > 0): no float32-versus-float64 disagreement
              about the sign of a pre-activation near zero.  The forward's own relu output is compared directly.
  workspace   exactly ``*_workspace_floats`` floats with GUARD sentinel floats behind them, which must survive; the
              workspace is pre-filled with 777 for one run and with NaN for the next, and both runs (forwards too) must give
              identical bits.
  symmetric   a CIN layer given the same pointer and leading dimension for H and X0 (h == M): gH and gX0 are compared with
              the split include/dctr.h documents, and gH + gX0 with the total gradient on X0.
  accumulate  ``accumulate_x0 = 1``: gX0 is pre-filled with random values; the reference is pre-fill + gradient in float64."""
import ctypes
import itertools

import numpy as np
import torch

import np_oracle
import np_oracle as O

SENT = 777.0
GUARD = 4
OUT_TOL, GRAD_TOL, GK_TOL = 1e-5, 2e-5, 5e-5
ENOSUP = -2
WORST = {}


class Buf(object):
    """float32 [rows, ld] on the device; ``cols`` (bool [ld]) marks the columns the header documents.  Everything else
    holds the sentinel."""

    def __init__(self, dev, rows, cols, values=None):
        self.cols = np.asarray(cols, bool)
        host = np.full((rows, self.cols.size), SENT, np.float32)
        if values is not None:
            host[:, self.cols] = np.asarray(values, np.float32).reshape(rows, int(self.cols.sum()))
        self.t = torch.from_numpy(host).to(dev)

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * self.lead)

    lead = 0          # floats in front of the address the entry point is given (a deliberately misaligned base)

    @property
    def ld(self):
        return int(self.cols.size)

    def get(self):
        return self.t.cpu().numpy()[:, self.cols].astype(np.float64)

    def untouched(self):
        return bool(np.all(self.t.cpu().numpy()[:, ~self.cols] == np.float32(SENT)))


def _mask(n, pad):
    return np.arange(n + pad) < n


def pairs_of(F):
    p = list(itertools.combinations(range(F), 2))
    return [i for i, _ in p], [j for _, j in p]


class Case(object):
    op = "?"
    relative = False          # True: deviations are divided by max|ref|, and a zero reference must come back exactly zero
    repeat_forward = False    # True: a second forward (over a NaN-filled workspace) must give identical bits

    def __init__(self, lib, dev, B, pad=0, seed=0):
        from deepctr_torch._hip import lib as L
        self.lib, self.dev = lib, torch.device(dev)
        self.B = self.nB = B
        self.pad = pad
        self.rng = np.random.RandomState(seed)
        self.stream = L.stream_handle(self.dev)
        self.tol = {}
        self.inputs, self.fwd_out, self.bwd_out = {}, {}, {}

    # ---- buffers -----------------------------------------------------------------------------------------------------
    def rows_in(self, name, values, pad=None):
        values = np.asarray(values)
        b = Buf(self.dev, values.shape[0], _mask(values.shape[1], self.pad if pad is None else pad), values)
        self.inputs[name] = b
        return b

    def flat_in(self, name, values):
        values = np.asarray(values).reshape(1, -1)
        return self.rows_in(name, values, pad=GUARD)

    def rows_out(self, n, rows=None, pad=None):
        return Buf(self.dev, self.B if rows is None else rows, _mask(n, self.pad if pad is None else pad))

    def flat_out(self, n):
        return Buf(self.dev, 1, _mask(n, GUARD))

    def normal(self, scale, *shape):
        return self.rng.normal(0, scale, shape).astype(np.float32)

    def sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)

    # ---- the check ---------------------------------------------------------------------------------------------------
    def default_tol(self, name, fwd):
        return OUT_TOL if fwd else (GK_TOL if name == "g_kernels" else GRAD_TOL)

    def compare(self, bufs, ref, fwd):
        for name, buf in bufs.items():
            got = buf.get()
            r = np.asarray(ref[name], np.float64).reshape(got.shape)
            scale = max(1.0, float(np.abs(r).max())) if r.size else 1.0
            err = float(np.abs(got - r).max()) if r.size else 0.0
            if self.relative and r.size:
                scale = float(np.abs(r).max())
                if scale == 0.0:
                    assert np.all(got == 0.0), "%s %s: max|d|=%.3e where the reference is identically zero" % (
                        self.op, name, err)
                    scale = 1.0
            tol = self.tol.get(name, self.default_tol(name, fwd))
            key = (self.op, name)
            WORST[key] = max(WORST.get(key, 0.0), err / scale)
            print("%s %s: max|d| %.3e  scale %.3g  ratio %.3e (bound %.1e)" % (self.op, name, err, scale, err / scale, tol))
            assert np.all(np.isfinite(got)), "%s %s: not finite" % (self.op, name)
            assert err <= tol * scale, "%s %s: max|d|=%.3e (scale %.3g, bound %.1e)" % (self.op, name, err, scale, tol)
            assert buf.untouched(), "%s %s: a float outside the documented columns was written" % (self.op, name)

    def check(self, grad=True):
        rc = self.forward()
        assert rc == 0, "%s forward: code %d" % (self.op, rc)
        ref = self.reference(grad)
        self.compare(self.fwd_out, ref, True)
        if self.repeat_forward:
            first = dict((k, b.t.clone()) for k, b in self.fwd_out.items())
            assert self.forward() == 0
            for k, b in self.fwd_out.items():
                assert torch.equal(first[k], b.t), "%s %s: two forward runs differ" % (self.op, k)
        if grad:
            rc = self.backward()
            assert rc == 0, "%s backward: code %d" % (self.op, rc)
            first = dict((k, b.t.clone()) for k, b in self.bwd_out.items())
            self.compare(self.bwd_out, ref, False)
            assert self.backward() == 0
            for k, b in self.bwd_out.items():
                assert torch.equal(first[k], b.t), "%s %s: two backward runs differ" % (self.op, k)
        for name, b in self.inputs.items():
            assert b.untouched(), "%s: the padding of input %s was written" % (self.op, name)
        return ref

    def sentinel_everywhere(self, bufs):
        return all(float(b.t.min()) == SENT and float(b.t.max()) == SENT for b in bufs.values())


# ---- FM on an explicit tensor ------------------------------------------------------------------------------------------
class FMCase(Case):
    op = "fm"

    def __init__(self, lib, dev, B, F, D, pad=0, accumulate=False, seed=0):
        Case.__init__(self, lib, dev, B, pad, seed)
        self.F, self.D, self.accumulate = F, D, accumulate
        self.E = self.rows_in("E", self.normal(0.7, B, F * D))
        self.gy = self.flat_in("gy", self.normal(1.0, B))
        self.pre = self.normal(1.0, B, F * D)

    def forward(self):
        self.fwd_out = {"y": self.flat_out(self.B)}
        rc = self.lib.dctr_fm_fwd(self.E.ptr(), self.E.ld, self.nB, self.F, self.D, self.fwd_out["y"].ptr(), self.stream)
        self.sync()
        return rc

    def backward(self):
        g = Buf(self.dev, self.B, _mask(self.F * self.D, self.pad), self.pre if self.accumulate else None)
        self.bwd_out = {"gE": g}
        rc = self.lib.dctr_fm_bwd(self.E.ptr(), self.E.ld, self.nB, self.F, self.D, self.gy.ptr(), g.ptr(), g.ld,
                                  int(self.accumulate), self.stream)
        self.sync()
        return rc

    def reference(self, grad=True):
        E = self.E.get().reshape(self.B, self.F, self.D)
        ref = {"y": O.fm_forward(E)[:, 0]}
        if grad:
            ref["gE"] = O.fm_backward(E, self.gy.get().reshape(self.B, 1)).reshape(self.B, -1)
            if self.accumulate:
                ref["gE"] = ref["gE"] + self.pre.astype(np.float64)
        return ref


# ---- BiInteractionPooling + NFM's DNN input ----------------------------------------------------------------------------
class BiPoolingCase(Case):
    """G row = [ F*D field floats | 2 floats of something else | n_dense dense floats | pad ]: dense_off lies past F*D"""
    op = "bi_pooling"

    def __init__(self, lib, dev, B, F, D, n_dense=0, pad=0, seed=0):
        Case.__init__(self, lib, dev, B, pad, seed)
        self.F, self.D, self.n_dense = F, D, n_dense
        self.dense_off = F * D + 2 if n_dense else -1
        width = F * D + (2 + n_dense if n_dense else 0) + pad
        self.gcols = np.zeros(width, bool)
        self.gcols[:F * D] = True
        if n_dense:
            self.gcols[self.dense_off:self.dense_off + n_dense] = True
        self.G = Buf(self.dev, B, self.gcols, self.normal(0.7, B, F * D + n_dense))
        self.inputs["G"] = self.G
        self.gout = self.rows_in("gout", self.normal(1.0, B, D + n_dense))

    def _head(self):
        return (self.G.ptr(), self.G.ld, self.nB, self.F, self.D, self.dense_off, self.n_dense)

    def forward(self):
        o = self.rows_out(self.D + self.n_dense)
        self.fwd_out = {"out": o}
        rc = self.lib.dctr_bi_pooling_fwd(*(self._head() + (o.ptr(), o.ld, self.stream)))
        self.sync()
        return rc

    def backward(self):
        g = Buf(self.dev, self.B, self.gcols)
        self.bwd_out = {"gG": g}
        rc = self.lib.dctr_bi_pooling_bwd(*(self._head() + (self.gout.ptr(), self.gout.ld, g.ptr(), g.ld, self.stream)))
        self.sync()
        return rc

    def reference(self, grad=True):
        FD = self.F * self.D
        G = torch.from_numpy(self.G.get()).requires_grad_(grad)
        E = G[:, :FD].reshape(self.B, self.F, self.D)
        out = torch.cat([0.5 * (E.sum(1).pow(2) - E.pow(2).sum(1)), G[:, FD:]], 1)
        ref = {"out": out.detach().numpy()}
        if grad:
            ref["gG"] = torch.autograd.grad(out, G, torch.from_numpy(self.gout.get()))[0].numpy()
        return ref


# ---- InnerProduct ------------------------------------------------------------------------------------------------------
class InnerProductCase(Case):
    op = "inner_product"

    def __init__(self, lib, dev, B, F, D, reduce, pad=0, seed=0):
        Case.__init__(self, lib, dev, B, pad, seed)
        self.F, self.D, self.reduce = F, D, int(reduce)
        self.P = F * (F - 1) // 2
        self.n_out = self.P * (1 if reduce else D)
        self.E = self.rows_in("E", self.normal(0.7, B, F * D))
        self.gp = self.rows_in("gp", self.normal(1.0, B, self.n_out))

    def forward(self):
        o = self.rows_out(self.n_out)
        self.fwd_out = {"out": o}
        rc = self.lib.dctr_inner_product_fwd(self.E.ptr(), self.E.ld, self.nB, self.F, self.D, self.reduce, o.ptr(), o.ld,
                                             self.stream)
        self.sync()
        return rc

    def backward(self):
        g = self.rows_out(self.F * self.D)
        self.bwd_out = {"gE": g}
        rc = self.lib.dctr_inner_product_bwd(self.E.ptr(), self.E.ld, self.nB, self.F, self.D, self.reduce, self.gp.ptr(),
                                             self.gp.ld, g.ptr(), g.ld, self.stream)
        self.sync()
        return rc

    def reference(self, grad=True):
        E = self.E.get().reshape(self.B, self.F, self.D)
        if self.reduce:
            out, pairs = O.inner_product_forward(E)
            ref = {"out": out}
            if grad:
                ref["gE"] = O.inner_product_backward(E, pairs, self.gp.get())
            return ref
        Et = torch.from_numpy(E).requires_grad_(grad)
        i, j = pairs_of(self.F)
        out = (Et[:, i] * Et[:, j]).reshape(self.B, -1)
        ref = {"out": out.detach().numpy()}
        if grad:
            ref["gE"] = torch.autograd.grad(out, Et, torch.from_numpy(self.gp.get()))[0].numpy()
        return ref


# ---- SENET (V, a, a1, gV, gE are contiguous by the header: a flat buffer with a guard behind it) ---------------------------
class SenetCase(Case):
    op = "senet"

    def __init__(self, lib, dev, B, F, D, R, pad=0, seed=0):
        Case.__init__(self, lib, dev, B, pad, seed)
        self.F, self.D, self.R = F, D, R
        self.E = self.rows_in("E", self.normal(0.7, B, F * D))
        self.W1 = self.flat_in("W1", self.normal(0.5, R * F))
        self.W2 = self.flat_in("W2", self.normal(0.5, F * R))
        self.gV = self.flat_in("gV", self.normal(1.0, B * F * D))

    def forward(self):
        B, F, D, R = self.B, self.F, self.D, self.R
        self.fwd_out = {"V": self.flat_out(B * F * D), "a": self.flat_out(B * F), "a1": self.flat_out(B * R)}
        o = self.fwd_out
        rc = self.lib.dctr_senet_fwd(self.E.ptr(), self.E.ld, self.nB, F, D, self.W1.ptr(), self.W2.ptr(), R, o["V"].ptr(),
                                     o["a"].ptr(), o["a1"].ptr(), self.stream)
        self.sync()
        return rc

    def backward(self):
        B, F, D, R = self.B, self.F, self.D, self.R
        self.bwd_out = {"gE": self.flat_out(B * F * D), "gW1": self.flat_out(R * F), "gW2": self.flat_out(F * R)}
        o, f = self.bwd_out, self.fwd_out
        self.ws = self.flat_out(max(1, int(self.lib.dctr_senet_bwd_workspace_floats(max(B, 1), F, R))))
        rc = self.lib.dctr_senet_bwd(self.gV.ptr(), self.E.ptr(), self.E.ld, self.nB, F, D, self.W1.ptr(), self.W2.ptr(), R,
                                     f["a"].ptr(), f["a1"].ptr(), o["gE"].ptr(), o["gW1"].ptr(), o["gW2"].ptr(),
                                     self.ws.ptr(), self.stream)
        self.sync()
        return rc

    def reference(self, grad=True):
        B, F, D, R = self.B, self.F, self.D, self.R
        E = self.E.get().reshape(B, F, D)
        W1, W2 = self.W1.get().reshape(R, F), self.W2.get().reshape(F, R)
        V, cache = O.senet_forward(E, W1, W2)
        ref = {"V": V, "a": cache[2], "a1": cache[1]}
        if grad:
            ref["gE"], ref["gW1"], ref["gW2"] = O.senet_backward(self.gV.get().reshape(B, F, D), E, cache, W1, W2)
        return ref


# ---- AFM ---------------------------------------------------------------------------------------------------------------
def afm_torch(E, W, bias, h, p):
    """include/dctr.h: bi_k = e_i (.) e_j; t_k = relu(bi_k W + bias); s_k = t_k . h; a = softmax_k(s); y = (sum_k a_k bi_k) . p
    -> (y [B], s [B, P])"""
    i, j = pairs_of(E.shape[1])
    bi = E[:, i] * E[:, j]
    s = torch.relu(bi @ W + bias) @ h
    return ((torch.softmax(s, dim=1)[:, :, None] * bi).sum(1) * p).sum(1), s


class AFMCase(Case):
    op = "afm"

    def __init__(self, lib, dev, B, F, D, A, pad=0, seed=0, e_scale=0.7, w_scale=None):
        Case.__init__(self, lib, dev, B, pad, seed)
        self.F, self.D, self.A = F, D, A
        self.E = self.rows_in("E", self.normal(e_scale, B, F * D))
        self.W = self.flat_in("W", self.normal(w_scale or (2.0 / (D + A)) ** 0.5, D * A))
        self.bias = self.flat_in("bias", self.normal(0.3, A))
        self.h = self.flat_in("h", self.normal(w_scale or (2.0 / (A + 1)) ** 0.5, A))
        self.p = self.flat_in("p", self.normal((2.0 / (D + 1)) ** 0.5, D))
        self.gy = self.flat_in("gy", self.normal(1.0, B))

    def _head(self):
        return (self.E.ptr(), self.E.ld, self.nB, self.F, self.D, self.A, self.W.ptr(), self.bias.ptr(), self.h.ptr(),
                self.p.ptr())

    def forward(self):
        self.fwd_out = {"y": self.flat_out(self.B)}
        rc = self.lib.dctr_afm_fwd(*(self._head() + (self.fwd_out["y"].ptr(), self.stream)))
        self.sync()
        return rc

    def backward(self):
        D, A = self.D, self.A
        self.bwd_out = {"gE": self.rows_out(self.F * D), "gW": self.flat_out(D * A), "gbias": self.flat_out(A),
                        "gh": self.flat_out(A), "gp": self.flat_out(D)}
        o = self.bwd_out
        self.ws = self.flat_out(max(1, int(self.lib.dctr_afm_bwd_workspace_floats(max(self.B, 1), D, A))))
        rc = self.lib.dctr_afm_bwd(*(self._head() + (self.gy.ptr(), o["gE"].ptr(), o["gE"].ld, o["gW"].ptr(),
                                                     o["gbias"].ptr(), o["gh"].ptr(), o["gp"].ptr(), self.ws.ptr(),
                                                     self.stream)))
        self.sync()
        return rc

    def tensors(self, dtype=torch.float64, dev="cpu"):
        B, F, D, A = self.B, self.F, self.D, self.A
        shapes = (("E", (B, F, D)), ("W", (D, A)), ("bias", (A,)), ("h", (A,)), ("p", (D,)))
        return [torch.from_numpy(self.inputs[n].get().reshape(s)).to(device=dev, dtype=dtype) for n, s in shapes]

    def evaluate(self, dtype, dev, grad=True):
        """the formula with plain torch ops in ``dtype`` on ``dev`` -> dict like ``reference``"""
        ins = [t.requires_grad_(grad) for t in self.tensors(dtype, dev)]
        y, s = afm_torch(*ins)
        ref = {"y": y.detach().double().cpu().numpy()}
        self.scores = s.detach().double().cpu().numpy()
        if grad:
            gy = torch.from_numpy(self.gy.get().reshape(-1)).to(device=dev, dtype=dtype)
            gs = torch.autograd.grad(y, ins, gy)
            for n, g in zip(("gE", "gW", "gbias", "gh", "gp"), gs):
                ref[n] = g.double().cpu().numpy()
        return ref

    def reference(self, grad=True):
        return self.evaluate(torch.float64, "cpu", grad)


# ---- InteractingLayer --------------------------------------------------------------------------------------------------
def interacting_torch(E, H, scaling, Wq, Wk, Wv, Wr):
    B, F, D = E.shape
    A = D // H

    def heads(x):
        return x.reshape(B, F, H, A).permute(0, 2, 1, 3)
    q, k, v = heads(E @ Wq), heads(E @ Wk), heads(E @ Wv)
    s = q @ k.transpose(-1, -2)
    if scaling:
        s = s / (A ** 0.5)
    o = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, F, D)
    if Wr is not None:
        o = o + E @ Wr
    return torch.relu(o).reshape(B, -1)


class InteractingCase(Case):
    op = "interacting"
    NAMES = ("W_Query", "W_key", "W_Value", "W_Res")

    def __init__(self, lib, dev, B, F, D, H, res=True, scaling=False, pad=0, seed=0, e_scale=0.7, w_scale=0.3):
        Case.__init__(self, lib, dev, B, pad, seed)
        self.F, self.D, self.H, self.res, self.scaling = F, D, H, res, int(scaling)
        self.E = self.rows_in("E", self.normal(e_scale, B, F * D))
        self.Ws = [self.flat_in(n, self.normal(w_scale, D * D)) for n in self.NAMES[:4 if res else 3]]
        self.gout = self.rows_in("gout", self.normal(1.0, B, F * D))

    def _head(self):
        w = [b.ptr() for b in self.Ws] + ([] if self.res else [None])
        return (self.E.ptr(), self.E.ld, self.nB, self.F, self.D, self.H, self.scaling) + tuple(w)

    def forward(self):
        o = self.rows_out(self.F * self.D)
        self.fwd_out = {"out": o}
        rc = self.lib.dctr_interacting_fwd(*(self._head() + (o.ptr(), o.ld, self.stream)))
        self.sync()
        return rc

    def backward(self):
        D = self.D
        self.bwd_out = {"gE": self.rows_out(self.F * D)}
        for n in self.NAMES[:len(self.Ws)]:
            self.bwd_out["g" + n] = self.flat_out(D * D)
        o = self.bwd_out
        self.ws = self.flat_out(max(1, int(self.lib.dctr_interacting_bwd_workspace_floats(max(self.B, 1), D))))
        gw = [o["g" + n].ptr() for n in self.NAMES[:len(self.Ws)]] + ([] if self.res else [None])
        rc = self.lib.dctr_interacting_bwd(*(self._head() + (self.gout.ptr(), self.gout.ld, o["gE"].ptr(), o["gE"].ld) +
                                             tuple(gw) + (self.ws.ptr(), self.stream)))
        self.sync()
        return rc

    def reference(self, grad=True):
        B, F, D, H = self.B, self.F, self.D, self.H
        E = self.E.get().reshape(B, F, D)
        P = dict((n, b.get().reshape(D, D)) for n, b in zip(self.NAMES, self.Ws))
        out, cache = O.interacting_forward(E, P, "", H, use_res=self.res, scaling=bool(self.scaling))
        _, qh, kh = cache[0], cache[1], cache[2]
        inner = qh @ kh.transpose(0, 1, 3, 2)
        self.scores = (inner / (D // H) ** 0.5 if self.scaling else inner).reshape(-1, F)       # one softmax row each
        ref = {"out": out.reshape(B, -1)}
        if grad:
            grads = {}
            ref["gE"] = O.interacting_backward(self.gout.get().reshape(B, F, D), cache, P, "", H, grads, use_res=self.res,
                                               scaling=bool(self.scaling))
            for n in self.NAMES[:len(self.Ws)]:
                ref["g" + n] = grads[n]
        return ref

    def evaluate(self, dtype, dev):
        """the formula with plain torch ops in ``dtype`` on ``dev`` -> dict like ``reference``"""
        B, F, D = self.B, self.F, self.D
        E = torch.from_numpy(self.E.get().reshape(B, F, D)).to(device=dev, dtype=dtype).requires_grad_(True)
        Ws = [torch.from_numpy(b.get().reshape(D, D)).to(device=dev, dtype=dtype).requires_grad_(True) for b in self.Ws]
        out = interacting_torch(E, self.H, self.scaling, *(Ws + ([] if self.res else [None])))
        g = torch.from_numpy(self.gout.get()).to(device=dev, dtype=dtype)
        gs = torch.autograd.grad(out, [E] + Ws, g)
        ref = {"out": out.detach().double().cpu().numpy(), "gE": gs[0].double().cpu().numpy()}
        for n, gw in zip(self.NAMES, gs[1:]):
            ref["g" + n] = gw.double().cpu().numpy()
        return ref


# ---- CrossNet, vector parameterisation ---------------------------------------------------------------------------------
class CrossNetCase(Case):
    op = "crossnet_vec"

    def __init__(self, lib, dev, B, W, L, pad=0, seed=0):
        Case.__init__(self, lib, dev, B, pad, seed)
        self.W, self.Lyr = W, L
        self.X = self.rows_in("X", self.normal(0.5, B, W))
        self.kernels = self.flat_in("kernels", self.normal(0.5 * (2.0 / (W + 1)) ** 0.5, L * W))
        self.bias = self.flat_in("bias", self.normal(0.1, L * W))
        self.gY = self.rows_in("gY", self.normal(1.0, B, W))

    def _head(self):
        return (self.X.ptr(), self.X.ld, self.nB, self.W, self.Lyr, self.kernels.ptr(), self.bias.ptr())

    def forward(self):
        o = self.rows_out(self.W)
        self.fwd_out = {"Y": o}
        rc = self.lib.dctr_crossnet_vec_fwd(*(self._head() + (o.ptr(), o.ld, self.stream)))
        self.sync()
        return rc

    def backward(self):
        n = self.Lyr * self.W
        self.bwd_out = {"gX": self.rows_out(self.W), "g_kernels": self.flat_out(n), "g_bias": self.flat_out(n)}
        o = self.bwd_out
        self.ws = self.flat_out(max(1, int(self.lib.dctr_crossnet_vec_bwd_workspace_floats(max(self.B, 1), self.W, self.Lyr))))
        rc = self.lib.dctr_crossnet_vec_bwd(*(self._head() + (self.gY.ptr(), self.gY.ld, o["gX"].ptr(), o["gX"].ld,
                                                              o["g_kernels"].ptr(), o["g_bias"].ptr(), self.ws.ptr(),
                                                              self.stream)))
        self.sync()
        return rc

    def reference(self, grad=True):
        L, W = self.Lyr, self.W
        K, Bs = self.kernels.get().reshape(L, W, 1), self.bias.get().reshape(L, W, 1)
        Y, xs = O.crossnet_forward(self.X.get(), K, Bs, "vector")
        ref = {"Y": Y}
        if grad:
            ref["gX"], ref["g_kernels"], ref["g_bias"] = O.crossnet_backward(self.gY.get(), xs, K, Bs, "vector")
        return ref


# ---- the CIN layer, its glue and the matrix CrossNet: rules of the module docstring's second part --------------------------
EINVAL, EALIGN = -1, -3


class NewCase(Case):
    relative = True
    repeat_forward = True

    def __init__(self, lib, dev, B, pad=0, seed=0):
        Case.__init__(self, lib, dev, B, pad, seed)
        self.runs = {"fwd": 0, "bwd": 0}

    def workspace(self, n, which):
        """exactly ``n`` floats, filled with 777 on the first run of ``which`` and with NaN on the next, GUARD sentinel
        floats behind them"""
        ws = Buf(self.dev, 1, _mask(int(n), GUARD))
        if n:
            ws.t[0, :int(n)] = SENT if self.runs[which] % 2 == 0 else float("nan")
        self.runs[which] += 1
        return ws

    def guard_intact(self, ws, what="workspace"):
        self.sync()
        assert ws.untouched(), "%s %s: a float behind the advertised size was written" % (self.op, what)

    def flat_lead(self, name, values, lead):
        """a flat input whose base lies ``lead`` floats into its buffer (lead = 1: not 16-byte aligned)"""
        values = np.asarray(values).reshape(1, -1)
        cols = np.zeros(lead + values.shape[1] + GUARD, bool)
        cols[lead:lead + values.shape[1]] = True
        b = Buf(self.dev, 1, cols, values)
        b.lead = lead
        self.inputs[name] = b
        return b


_CIN_REF = {}


def _ratio(d, ref):
    """max|d| / max|ref|; where the reference is identically zero any deviation at all counts as infinite"""
    scale = float(np.abs(ref).max())
    return d / scale if scale else (0.0 if d == 0.0 else float("inf"))


def cin_sym_split(X0, W, gY):
    """what gH and gX0 each receive from the symmetric kernels (include/dctr.h, dctr_cin_layer_bwd): every unordered field
    pair a <= b once, with the folded weight; pairs with a < Hh = (M + 1) / 2 give field a's share to gH and field b's to
    gX0, pairs with a >= Hh the other way round"""
    B, M, D = X0.shape
    Hh = (M + 1) // 2
    Wm = W.reshape(-1, M, M)
    Wf = np.triu(Wm + Wm.transpose(0, 2, 1), 1)
    i = np.arange(M)
    Wf[:, i, i] = Wm[:, i, i]
    t = np.einsum("oab,nod->nabd", Wf, gY)
    gH, gX = np.zeros_like(X0), np.zeros_like(X0)
    gH[:, :Hh] += np.einsum("nabd,nbd->nad", t[:, :Hh], X0)
    gX += np.einsum("nabd,nad->nbd", t[:, :Hh], X0[:, :Hh])
    gH += np.einsum("nabd,nad->nbd", t[:, Hh:], X0[:, Hh:])
    gX[:, Hh:] += np.einsum("nabd,nbd->nad", t[:, Hh:], X0)
    return gH, gX


class CinLayerCase(NewCase):
    """dctr_cin_layer_fwd / _bwd.  ``sym``: H IS X0 (one buffer, h == M); ``same``: H holds X0's values in a buffer of its
    own (the general kernels on the symmetric layer's inputs: shares the symmetric case's float64 reference); ``pads``:
    extra floats behind the rows of h / x0 / a / gh / gx (default ``pad`` each); ``force_ld``: a leading dimension the
    entry point is TOLD in place of the buffer's (refusal cases)."""
    op = "cin_layer"

    def __init__(self, lib, dev, B, h, M, D, O, relu=1, bias=True, gbias=True, sym=False, same=False, accumulate=False,
                 pad=0, pads=None, seed=None):
        seed = (B * 7 + h * 11 + M * 13 + D * 17 + O * 19) if seed is None else seed
        NewCase.__init__(self, lib, dev, B, pad, seed)
        assert not (sym or same) or h == M
        self.h, self.M, self.D, self.O, self.relu = h, M, D, O, int(relu)
        self.sym, self.same, self.accumulate, self.has_gbias = sym, sym or same, accumulate, gbias
        self.pads = dict((k, pad) for k in ("h", "x0", "a", "gh", "gx"))
        self.pads.update(pads or {})
        self.force_ld = {}
        self.key = (B, h, M, D, O, self.relu, bool(bias), seed, self.same, accumulate)
        x0, hh, w = self.normal(0.5, B, M * D), self.normal(0.5, B, h * D), self.normal(0.1, O * h * M)
        bs, ga, self.pre = self.normal(0.1, O), self.normal(1.0, B, O * D), self.normal(1.0, B, M * D)
        self.X0 = self.rows_in("X0", x0, pad=self.pads["x0"])
        self.H = self.X0 if sym else self.rows_in("H", x0 if same else hh, pad=self.pads["h"])
        self.W = self.flat_in("W", w)
        self.bias = self.flat_in("bias", bs) if bias else None
        self.gA = self.rows_in("gA", ga, pad=self.pads["a"])
        self.A_saved = None

    def ld(self, name, buf):
        return self.force_ld.get(name, buf.ld)

    def forward(self):
        h, M, D, O = self.h, self.M, self.D, self.O
        a = self.rows_out(O * D, pad=self.pads["a"])
        self.fwd_out = {"A": a}
        ws = self.workspace(self.lib.dctr_cin_workspace_floats(h, M, O), "fwd")
        rc = self.lib.dctr_cin_layer_fwd(self.H.ptr(), self.ld("h", self.H), self.X0.ptr(), self.ld("x0", self.X0),
                                         self.W.ptr(), self.bias.ptr() if self.bias else None, self.nB, h, M, D, O,
                                         self.relu, a.ptr(), self.ld("a", a), ws.ptr(), self.stream)
        self.guard_intact(ws, "forward workspace")
        return rc

    def backward(self):
        h, M, D, O = self.h, self.M, self.D, self.O
        if self.A_saved is None:          # the float64 forward rounded to float32: the saved activation of this backward
            self.A_saved = self.rows_in("A_saved", self.reference()["A"].astype(np.float32), pad=self.pads["a"])
        gx = Buf(self.dev, self.B, _mask(M * D, self.pads["gx"]), self.pre if self.accumulate else None)
        self.bwd_out = {"gH": self.rows_out(h * D, pad=self.pads["gh"]), "gX0": gx, "gW": self.flat_out(O * h * M)}
        if self.has_gbias:
            self.bwd_out["gbias"] = self.flat_out(O)
        o = self.bwd_out
        ws = self.workspace(self.lib.dctr_cin_bwd_workspace_floats(max(self.B, 1), h, M, D, O), "bwd")
        rc = self.lib.dctr_cin_layer_bwd(self.gA.ptr(), self.A_saved.ptr() if self.relu else None, self.ld("a", self.gA),
                                         self.relu, self.H.ptr(),
                                         self.ld("h", self.H), self.X0.ptr(), self.ld("x0", self.X0), self.W.ptr(), self.nB,
                                         h, M, D, O, o["gH"].ptr(), self.ld("gh", o["gH"]), gx.ptr(), self.ld("gx", gx),
                                         int(self.accumulate), o["gW"].ptr(),
                                         o["gbias"].ptr() if self.has_gbias else None, ws.ptr(), self.stream)
        self.guard_intact(ws, "backward workspace")
        return rc

    def arrays(self):
        B, h, M, D, O = self.B, self.h, self.M, self.D, self.O
        return (self.H.get().reshape(B, h, D), self.X0.get().reshape(B, M, D), self.W.get().reshape(O, h * M),
                self.bias.get().reshape(O) if self.bias else None, self.gA.get().reshape(B, O, D))

    def reference(self, grad=True):
        """float64, shared by the cases with the same inputs: A; gH / gX0 of the general kernels (``g_gH`` / ``g_gX0``),
        their symmetric split (``s_gH`` / ``s_gX0``) and ``total`` = d loss / d X0 of a symmetric layer; gW; gbias"""
        ref = _CIN_REF.get(self.key)
        if ref is None:
            B, h, M, D, O = self.B, self.h, self.M, self.D, self.O
            H, X0, W, bias, gA = self.arrays()
            A, (Z, Y) = np_oracle.cin_layer_forward(H, X0, W, bias, bool(self.relu))
            mask_src = A.astype(np.float32).astype(np.float64) if self.relu else Y
            gH, gX0, gW, gb = np_oracle.cin_layer_backward(gA, H, X0, W, (Z, mask_src), bool(self.relu))
            pre = self.pre.astype(np.float64).reshape(B, M, D) if self.accumulate else 0.0
            ref = {"A": A.reshape(B, -1), "g_gH": gH.reshape(B, -1), "g_gX0": (gX0 + pre).reshape(B, -1), "gW": gW,
                   "gbias": gb}
            if self.same:
                sH, sX = cin_sym_split(X0, W, gA * (mask_src > 0) if self.relu else gA)
                ref.update({"s_gH": sH.reshape(B, -1), "s_gX0": (sX + pre).reshape(B, -1),
                            "total": (gH + gX0 + pre).reshape(B, -1)})
            if len(_CIN_REF) > 64:
                _CIN_REF.clear()
            _CIN_REF[self.key] = ref
        ref = dict(ref)
        pick = "s_" if self.sym else "g_"
        ref["gH"], ref["gX0"] = ref[pick + "gH"], ref[pick + "gX0"]
        return ref

    def compare(self, bufs, ref, fwd):
        Case.compare(self, bufs, ref, fwd)
        if self.sym and not fwd:          # what the callers rely on: the two buffers add up to the gradient on X0
            got = bufs["gH"].get() + bufs["gX0"].get()
            scale = float(np.abs(ref["total"]).max())
            err = float(np.abs(got - ref["total"]).max())
            WORST[(self.op, "gH+gX0")] = max(WORST.get((self.op, "gH+gX0"), 0.0), err / scale)
            print("%s gH+gX0: max|d| %.3e  scale %.3g  ratio %.3e (bound %.1e)" % (self.op, err, scale, err / scale, GRAD_TOL))
            assert err <= GRAD_TOL * scale, "%s gH+gX0: max|d|=%.3e (scale %.3g, bound %.1e)" % (self.op, err, scale,
                                                                                                 GRAD_TOL)

    def float32_ratios(self):
        """the op in plain torch float32 on the CPU -> {tensor: (max|d| / max|ref|, bound)} against ``reference()``; a
        symmetric layer's inputs also give the split and gH + gX0"""
        B, h, M, D, O = self.B, self.h, self.M, self.D, self.O
        ref = self.reference()
        H, X0, W, bias, gA = [None if a is None else torch.from_numpy(a).float() for a in self.arrays()]
        for t in (H, X0, W):
            t.requires_grad_(True)
        Z = (H[:, :, None, :] * X0[:, None, :, :]).reshape(B, h * M, D)
        Y = torch.einsum("ok,bkd->bod", W, Z)
        if bias is not None:
            Y = Y + bias[None, :, None]
        gY = gA * torch.from_numpy(ref["A"].reshape(B, O, D).astype(np.float32) > 0).float() if self.relu else gA
        gH, gX0, gW = torch.autograd.grad(Y, [H, X0, W], gY)
        if self.accumulate:
            gX0 = gX0 + torch.from_numpy(self.pre).reshape(B, M, D)
        got = {"A": (torch.relu(Y) if self.relu else Y).detach(), "gW": gW, "gbias": gY.sum((0, 2))}
        got["g_gH"], got["g_gX0"] = gH, gX0
        if self.same:          # the split in float32 as well, from the same float32 gradient rows
            sH, sX = cin_sym_split(X0.detach().numpy(), W.detach().numpy(), gY.numpy())
            pre = self.pre.reshape(B, M, D) if self.accumulate else np.float32(0)
            got["total"], got["s_gH"], got["s_gX0"] = gH + gX0, torch.from_numpy(sH), torch.from_numpy(sX + pre)
        out = {}
        for name, g in got.items():
            r = ref[name]
            d = float(np.abs(g.double().numpy().reshape(r.shape) - r).max())
            out[name] = (_ratio(d, r), OUT_TOL if name == "A" else GRAD_TOL)
        return out


class CinPoolCase(NewCase):
    """dctr_cin_pool_fwd / _bwd of one layer: ``n_hidden`` rows go on to the next layer, the rows from ``pool_from`` are
    summed over d.  ``w_head``: g_pooled is one float per sample, times w_head[j]; ``relu``: the mask of A is applied;
    ``pooled_grad = False``: g_pooled NULL; ``lead = 1``: g_hidden starts one float into its buffer."""
    op = "cin_pool"

    def __init__(self, lib, dev, B, O, D, n_hidden, pool_from, w_head=False, relu=True, pooled_grad=True, lead=0, pad=0,
                 seed=None):
        NewCase.__init__(self, lib, dev, B, pad, (B * 7 + O * 11 + D * 13 + n_hidden) if seed is None else seed)
        self.O, self.D, self.n_hidden, self.pool_from, self.relu = O, D, n_hidden, pool_from, relu
        nd = O - pool_from
        self.A = self.flat_in("A", self.normal(1.0, B * O * D))
        self.g_hidden = self.flat_lead("g_hidden", self.normal(1.0, B * n_hidden * D), lead) if n_hidden else None
        self.g_pooled = self.rows_in("g_pooled", self.normal(1.0, B, 1 if w_head else nd)) if pooled_grad else None
        self.w_head = self.flat_in("w_head", self.normal(0.5, nd)) if w_head else None
        assert not (w_head and not pooled_grad)

    def forward(self):
        o = self.rows_out(self.O - self.pool_from)
        self.fwd_out = {"pooled": o}
        rc = self.lib.dctr_cin_pool_fwd(self.A.ptr(), self.nB, self.O, self.D, self.pool_from, o.ptr(), o.ld, self.stream)
        self.sync()
        return rc

    def backward(self):
        g = self.flat_out(self.B * self.O * self.D)
        self.bwd_out = {"gA": g}
        gp = self.g_pooled
        rc = self.lib.dctr_cin_pool_bwd(self.g_hidden.ptr() if self.g_hidden else None, gp.ptr() if gp else None,
                                        gp.ld if gp else 0, self.w_head.ptr() if self.w_head else None,
                                        self.A.ptr() if self.relu else None, self.nB, self.O, self.D, self.n_hidden,
                                        self.pool_from, g.ptr(), self.stream)
        self.sync()
        return rc

    def reference(self, grad=True):
        B, O, D, nh, pf = self.B, self.O, self.D, self.n_hidden, self.pool_from
        A = torch.from_numpy(self.A.get().reshape(B, O, D))
        ref = {"pooled": A[:, pf:].sum(-1).numpy()}
        if grad:
            g = torch.zeros(B, O, D, dtype=torch.float64)
            if self.g_hidden:
                g[:, :nh] += torch.from_numpy(self.g_hidden.get().reshape(B, nh, D))
            if self.g_pooled:
                gp = torch.from_numpy(self.g_pooled.get())
                if self.w_head:
                    gp = gp * torch.from_numpy(self.w_head.get().reshape(1, -1))
                g[:, pf:] += gp[:, :, None]
            if self.relu:
                g = g * (A > 0)
            ref["gA"] = g.reshape(1, -1).numpy()
        return ref


class RowsDotCase(NewCase):
    op = "rows_dot"

    def check(self, grad=False):          # (no backward of its own: dctr_rows_tdot IS dctr_rows_dot's weight gradient)
        return Case.check(self, False)

    def __init__(self, lib, dev, B, N, pad=0, seed=None):
        NewCase.__init__(self, lib, dev, B, pad, (B * 7 + N * 11) if seed is None else seed)
        self.N = N
        self.x = self.rows_in("x", self.normal(1.0, B, N))
        self.w = self.flat_in("w", self.normal(0.5, N))

    def forward(self):
        o = self.flat_out(self.B)
        self.fwd_out = {"out": o}
        rc = self.lib.dctr_rows_dot(self.x.ptr(), self.x.ld, self.w.ptr(), self.nB, self.N, o.ptr(), self.stream)
        self.sync()
        return rc

    def reference(self, grad=True):
        return {"out": (torch.from_numpy(self.x.get()) @ torch.from_numpy(self.w.get().reshape(-1))).numpy()}


class RowsTdotCase(NewCase):
    op = "rows_tdot"

    def check(self, grad=False):          # (no backward of its own: dctr_rows_tdot IS dctr_rows_dot's weight gradient)
        return Case.check(self, False)

    def __init__(self, lib, dev, B, N, pad=0, seed=None):
        NewCase.__init__(self, lib, dev, B, pad, (B * 7 + N * 11 + 1) if seed is None else seed)
        self.N = N
        self.x = self.rows_in("x", self.normal(1.0, B, N))
        self.w = self.flat_in("w", self.normal(0.5, B))

    def forward(self):
        o = self.flat_out(self.N)
        self.fwd_out = {"out": o}
        ws = self.workspace(self.lib.dctr_relu_bwd_bias_workspace_floats(self.B, self.N), "fwd")
        rc = self.lib.dctr_rows_tdot(self.x.ptr(), self.x.ld, self.w.ptr(), self.nB, self.N, o.ptr(), ws.ptr(), self.stream)
        self.guard_intact(ws)
        return rc

    def reference(self, grad=True):
        return {"out": (torch.from_numpy(self.w.get().reshape(-1)) @ torch.from_numpy(self.x.get())).numpy()}


class CrossNetMatCase(NewCase):
    """dctr_crossnet_mat_fwd / _bwd on a dctr_mlp_t of L layers W x W.  Every leading dimension is W + pad with
    pad = 4 - W % 4 (+ ``extra``, a multiple of 4): a multiple of 4 and greater than W.  Checked: the last layer's h
    (``Y``), gx and every layer's gW over their W documented columns -- their padding columns must be zero, as the header
    says -- and gbias.  The
    other layers' h and every dh are scratch: only the guards behind them are looked at."""
    op = "crossnet_mat"

    def __init__(self, lib, dev, B, W, L, extra=0, seed=None):
        assert extra % 4 == 0
        NewCase.__init__(self, lib, dev, B, 4 - W % 4 + extra, (B * 7 + W * 11 + L * 13) if seed is None else seed)
        self.W, self.Lyr = W, L
        self.ldw = W + self.pad
        self.force_ld = {}
        self.w_out = None
        self.X = self.rows_in("X", self.normal(0.5, B, W))
        self.Ws = [self.rows_in("W%d" % l, self.normal(0.5 / W ** 0.5, W, W)) for l in range(L)]
        self.bs = [self.flat_in("bias%d" % l, self.normal(0.1, W)) for l in range(L)]
        self.gY = self.rows_in("gY", self.normal(1.0, B, W))

    def default_tol(self, name, fwd):
        return OUT_TOL if fwd else (GK_TOL if name.startswith("gW") else GRAD_TOL)

    def _mlp(self):
        from deepctr_torch._hip import lib as L
        B, W, n = self.B, self.W, self.Lyr
        if not hasattr(self, "hs"):
            self.hs = [Buf(self.dev, 1, _mask(B * self.ldw, GUARD)) for _ in range(n - 1)] + [self.rows_out(W)]
            self.dhs = [Buf(self.dev, 1, _mask(B * self.ldw, GUARD)) for _ in range(n)]
        self.gWs = [Buf(self.dev, 1, _mask(W * self.ldw, GUARD)) for _ in range(n)]
        self.gbs = [self.flat_out(W) for _ in range(n)]
        m = L.Mlp()
        m.n_layers = n
        for l in range(n):
            e = m.layer[l]
            e.W, e.bias, e.h, e.dh = self.Ws[l].ptr(), self.bs[l].ptr(), self.hs[l].ptr(), self.dhs[l].ptr()
            e.gW, e.gbias = self.gWs[l].ptr(), self.gbs[l].ptr()
            e.K = e.N = W
            e.ld_w = self.force_ld.get("w", self.ldw)
            e.ld_h = self.force_ld.get("h", self.ldw)
            e.relu = 0
        m.w_out = self.w_out.ptr() if self.w_out else None
        return m

    def forward(self):
        self.m = self._mlp()
        self.hs[-1].t.fill_(SENT)          # (a repeated forward that wrote nothing must not pass for identical bits)
        self.fwd_out = {"Y": self.hs[-1]}
        rc = self.lib.dctr_crossnet_mat_fwd(ctypes.byref(self.m), self.X.ptr(), self.force_ld.get("x", self.X.ld), self.nB,
                                            self.stream)
        self.sync()
        return rc

    def backward(self):
        if self.runs["bwd"]:          # the backward turned the u_l parked in dh into gradients: park them again
            assert self.forward() == 0
        self.m = self._mlp()
        gx = Buf(self.dev, self.B, np.ones(self.ldw, bool))          # include/dctr.h: the padding columns of gx receive 0
        self.bwd_out = {"gx": gx}
        for l in range(self.Lyr):
            self.bwd_out["gbias%d" % l] = self.gbs[l]
        for l in range(self.Lyr):
            self.bwd_out["gW%d" % l] = self.gWs[l]
        ws = self.workspace(self.lib.dctr_crossnet_mat_bwd_workspace_floats(ctypes.byref(self.m), max(self.B, 1)), "bwd")
        rc = self.lib.dctr_crossnet_mat_bwd(ctypes.byref(self.m), self.X.ptr(), self.force_ld.get("x", self.X.ld), self.nB,
                                            self.gY.ptr(), self.force_ld.get("g", self.gY.ld), gx.ptr(),
                                            self.force_ld.get("gx", gx.ld),
                                            ws.ptr(),
                                            self.stream)
        self.guard_intact(ws)
        for b in self.hs[:-1] + self.dhs:
            assert b.untouched(), "%s: a float behind a layer's h / dh was written" % self.op
        return rc

    def arrays(self):
        L, W = self.Lyr, self.W
        return (self.X.get(), np.stack([b.get() for b in self.Ws]), np.stack([b.get().reshape(W, 1) for b in self.bs]),
                self.gY.get())

    def reference(self, grad=True):
        X, K, Bs, gY = self.arrays()
        Y, xs = np_oracle.crossnet_forward(X, K, Bs, "matrix")
        ref = {"Y": Y}
        if grad:
            gx, gk, gb = np_oracle.crossnet_backward(gY, xs, K, Bs, "matrix")
            ref["gx"] = np.zeros((self.B, self.ldw))
            ref["gx"][:, :self.W] = gx
            for l in range(self.Lyr):
                full = np.zeros((self.W, self.ldw))          # include/dctr.h: the padding columns of gW receive 0
                full[:, :self.W] = gk[l]
                ref["gW%d" % l], ref["gbias%d" % l] = full.reshape(1, -1), gb[l].reshape(1, -1)
        return ref

    def compare(self, bufs, ref, fwd):
        if not fwd:
            for l in range(self.Lyr):
                padding = bufs["gW%d" % l].get().reshape(self.W, self.ldw)[:, self.W:]
                assert np.all(padding == 0.0), "%s gW%d: a padding column is not zero" % (self.op, l)
            assert np.all(bufs["gx"].get()[:, self.W:] == 0.0), "%s gx: a padding column is not zero" % self.op
        Case.compare(self, bufs, ref, fwd)

    def float32_ratios(self):
        """the op in plain torch float32 on the CPU -> {tensor: (max|d| / max|ref|, bound)} against ``reference()``"""
        ref = self.reference()
        X, K, Bs, gY = [torch.from_numpy(a).float() for a in self.arrays()]
        for t in (X, K, Bs):
            t.requires_grad_(True)
        xl = X
        for l in range(self.Lyr):
            xl = X * (xl @ K[l].t() + Bs[l][:, 0]) + xl
        gx, gk, gb = torch.autograd.grad(xl, [X, K, Bs], gY)
        full = torch.zeros(self.B, self.ldw)
        full[:, :self.W] = gx
        got = {"Y": xl.detach(), "gx": full}
        for l in range(self.Lyr):
            full = torch.zeros(self.W, self.ldw)
            full[:, :self.W] = gk[l]
            got["gW%d" % l], got["gbias%d" % l] = full, gb[l]
        out = {}
        for name, g in got.items():
            r = ref[name]
            d = float(np.abs(g.double().numpy().reshape(r.shape) - r).max())
            out[name] = (_ratio(d, r), self.default_tol(name, name == "Y"))
        return out


NEW_OPS = ("cin_layer", "cin_pool", "rows_dot", "rows_tdot", "crossnet_mat")


def _smallest_new(lib, dev, op, D):
    for B in (1, 5):
        for pad in (0, 5):
            if op == "cin_layer":
                yield CinLayerCase(lib, dev, B, 1, 2, D, 1, relu=int(pad == 0), pad=pad)
                yield CinLayerCase(lib, dev, B, 2, 2, D, 3, sym=True, accumulate=B == 5, pad=pad)
            elif op == "cin_pool":
                yield CinPoolCase(lib, dev, B, 2, D, 1, 1, w_head=pad == 0, pad=pad)
                yield CinPoolCase(lib, dev, B, 2, D, 0, 0, relu=False, pad=pad)
            elif op == "rows_dot":
                yield RowsDotCase(lib, dev, B, D, pad=pad)
            elif op == "rows_tdot":
                yield RowsTdotCase(lib, dev, B, D, pad=pad)
            else:
                yield CrossNetMatCase(lib, dev, B, D, 2, extra=4 if pad else 0)


def _cin_layer_cases():
    """(id, CinLayerCase keywords) of every device case of tests/test_gpu_cin_abi.py that runs the full check; the id says
    which branch of csrc/cin.hip's launchers the case is there for.  tests/test_interaction_abi_host.py evaluates each in
    plain float32 on the CPU."""
    c = [("minimal", dict(B=1, h=1, M=1, D=1, O=1))]
    # sizes of O: every OT instantiation both ways, the separately launched last chunk, gH / gX0 accumulated over chunks of 128
    c += [("O=%d" % o, dict(B=5, h=3, M=5, D=4, O=o, pad=3 if o % 2 else 0))
          for o in (31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 224, 256, 257)]
    # columns B * D around the 256-column tile; at D = 3 / 5 / 17 a sample straddles the tile edge
    c += [("cols=%dx%d" % (b, d), dict(B=b, h=2, M=3, D=d, O=5, pad=b % 2))
          for b, d in ((255, 1), (256, 1), (257, 1), (85, 3), (86, 3), (51, 5), (52, 5), (16, 16), (17, 16), (15, 17),
                       (16, 17))]
    # sizes of M: an odd M pads to M_pad
    c += [("M=%d" % m, dict(B=3, h=2, M=m, D=4, O=5, pad=m % 2)) for m in (1, 2, 31, 32)]
    # weight gradient: column groups of 256 (h*M = 255, 256, 258 -> 1, 1, 2; 64 x 26 -> 7), hspan at M = 26, partial sets
    c += [("wgrad-hM=%dx%d" % (h, m), dict(B=3, h=h, M=m, D=4, O=5))
          for h, m in ((51, 5), (8, 32), (43, 6), (64, 26), (10, 26), (11, 26), (12, 26))]
    c += [("wgrad-sets-BD=%dx%d" % (b, d), dict(B=b, h=3, M=5, D=d, O=5, pad=1))
          for b, d in ((16, 4), (64, 1), (65, 1), (13, 5))]
    c += [("wgrad-512-sets", dict(B=2100, h=4, M=5, D=16, O=8))]
    # k_cin_wgrad's opt-in to more than 64 KB of LDS: ph = min(h, 255 / M + 2) | 1 > 94
    c += [("wgrad-lds-hM=%dx%d" % (h, m), dict(B=9, h=h, M=m, D=4, O=33)) for h, m in ((93, 2), (94, 2), (130, 1))]
    # k_cin_bwd_data_flat (M = 26, H != X0, three or four row tiles): not taken at O = 64; O = 129 a flat chunk then a regular
    # one; O = 224 two flat chunks, the second accumulating
    c += [("flat-h=3-O=%d" % o, dict(B=5, h=3, M=26, D=4, O=o, pad=o % 2)) for o in (64, 65, 96, 128, 129, 224)]
    c += [("flat-h=%d-O=%d" % (h, o), dict(B=5, h=h, M=26, D=4, O=o)) for h in (1, 17) for o in (96, 129)]
    # the symmetric kernels (one buffer for H and X0), and the same inputs in two buffers: the general kernels
    for m, o, b in [(m, o, 3) for m in (1, 2, 5, 26, 31, 32) for o in (8, 33, 129)] + [(5, 8, 64)]:
        c += [("sym-M=%d-O=%d-B=%d" % (m, o, b), dict(B=b, h=m, M=m, D=4, O=o, sym=True)),
              ("two-buffers-M=%d-O=%d-B=%d" % (m, o, b), dict(B=b, h=m, M=m, D=4, O=o, same=True))]
    # options
    c += [("relu=%d-bias=%d-gbias=%d" % (r, bi, gb), dict(B=5, h=3, M=5, D=4, O=33, relu=r, bias=bool(bi), gbias=bool(gb)))
          for r in (0, 1) for bi in (0, 1) for gb in (0, 1)]
    c += [("accumulate-general-O=130", dict(B=5, h=3, M=5, D=4, O=130, accumulate=True, pad=1)),
          ("accumulate-sym-O=130", dict(B=5, h=5, M=5, D=4, O=130, sym=True, accumulate=True)),
          ("accumulate-sym-M=26", dict(B=5, h=26, M=26, D=4, O=33, sym=True, accumulate=True, pad=1)),
          ("accumulate-flat-O=96", dict(B=5, h=3, M=26, D=4, O=96, accumulate=True)),
          ("every-ld-padded", dict(B=5, h=3, M=5, D=4, O=33, pads=dict(h=3, x0=5, a=2, gh=7, gx=1))),
          ("every-ld-padded-sym", dict(B=5, h=5, M=5, D=4, O=33, sym=True, pads=dict(x0=5, a=2, gh=7, gx=1))),
          ("H-is-the-first-half-of-a-wider-map", dict(B=5, h=3, M=5, D=4, O=33, pads=dict(h=12)))]
    return c


CIN_LAYER_CASES = _cin_layer_cases()
# (B, W, L): sizes of B at W = 5; of W at B = 17 (the backward opts in to > 64 KB of LDS from W = 193, the forward from
# W = 321; 512 is the envelope); many layers; the batches at which the weight gradient's batch slices change (B / 64)
CROSSNET_MAT_CASES = ([(b, 5, 2) for b in (1, 15, 16, 17, 33)] +
                      [(17, w, 1) for w in (1, 3, 4, 16, 17, 63, 64, 65, 192, 193, 320, 321, 512)] +
                      [(17, 17, 2), (17, 17, 12)] + [(b, 40, 2) for b in (63, 64, 65, 129, 1025)])


def report():
    for (op, name), r in sorted(WORST.items()):
        scale = "max|ref|        " if op in NEW_OPS else "max(1, max|ref|)"
        print("worst max|d| / %s  %-14s %-10s %.3e" % (scale, op, name, r))


# ---- the case lists both test files share ----------------------------------------------------------------------------------
OPS = ("fm", "bi_pooling", "inner_product", "senet", "afm", "interacting", "crossnet_vec")
SMALL_D = (1, 3, 16)


def smallest(lib, dev, op, D):
    """the smallest shapes of ``op`` at width D: B = 1 and 5, F = 2 (1 for fm, bi_pooling and senet, beside 2), rows padded
    by 0 and 5 floats"""
    if op in NEW_OPS:
        for case in _smallest_new(lib, dev, op, D):
            yield case
        return
    for B in (1, 5):
        for pad in (0, 5):
            seed = 100 * B + 10 * pad + D
            if op == "fm":
                yield FMCase(lib, dev, B, 1, D, pad=pad, seed=seed)
                yield FMCase(lib, dev, B, 2, D, pad=pad, accumulate=True, seed=seed)
            elif op == "bi_pooling":
                yield BiPoolingCase(lib, dev, B, 1, D, n_dense=0, pad=pad, seed=seed)
                yield BiPoolingCase(lib, dev, B, 2, D, n_dense=3, pad=pad, seed=seed)
            elif op == "inner_product":
                yield InnerProductCase(lib, dev, B, 2, D, True, pad=pad, seed=seed)
                yield InnerProductCase(lib, dev, B, 2, D, False, pad=pad, seed=seed)
            elif op == "senet":
                yield SenetCase(lib, dev, B, 1, D, 1, pad=pad, seed=seed)
                yield SenetCase(lib, dev, B, 2, D, 3, pad=pad, seed=seed)
            elif op == "afm":
                yield AFMCase(lib, dev, B, 2, D, 3, pad=pad, seed=seed)
            elif op == "interacting":
                yield InteractingCase(lib, dev, B, 2, D, 2 if D % 2 == 0 else 1, res=pad == 0, scaling=B == 1, pad=pad,
                                      seed=seed)
            else:
                yield CrossNetCase(lib, dev, B, D, 2, pad=pad, seed=seed)


def afm_overflow(lib, dev):
    return AFMCase(lib, dev, 5, 3, 4, 3, pad=5, seed=11, e_scale=5.0, w_scale=1.5)


def interacting_overflow(lib, dev, res=True):
    return InteractingCase(lib, dev, 5, 3, 4, 2, res=res, scaling=False, pad=5, seed=12, e_scale=4.0, w_scale=1.0)


def assert_overflows(case):
    """after ``case.reference()``: a kernel that skipped the row maximum would overflow expf (> 88.7) and the scores of one
    softmax are spread far beyond what fp32 exp can hold side by side"""
    s = case.scores
    spread = float((s.max(axis=1) - s.min(axis=1)).max())
    print("%s: largest score %.1f, largest |score| %.1f, largest spread inside one softmax %.1f" %
          (case.op, float(s.max()), float(np.abs(s).max()), spread))
    assert float(s.max()) > 90.0 and spread > 100.0
