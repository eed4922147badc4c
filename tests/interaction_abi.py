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
``max|d| / max(1, max|ref|)`` per (op, tensor)."""
import ctypes
import itertools

import numpy as np
import torch

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
        return ctypes.c_void_p(self.t.data_ptr())

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


def report():
    for (op, name), r in sorted(WORST.items()):
        print("worst max|d| / max(1, max|ref|)  %-14s %-10s %.3e" % (op, name, r))


# ---- the case lists both test files share ----------------------------------------------------------------------------------
OPS = ("fm", "bi_pooling", "inner_product", "senet", "afm", "interacting", "crossnet_vec")
SMALL_D = (1, 3, 16)


def smallest(lib, dev, op, D):
    """the smallest shapes of ``op`` at width D: B = 1 and 5, F = 2 (1 for fm, bi_pooling and senet, beside 2), rows padded
    by 0 and 5 floats"""
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
