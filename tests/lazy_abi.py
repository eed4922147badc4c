"""Driver for the lazy table-update entry points THROUGH THE C ABI (include/dctr.h: dctr_lazy_catchup, dctr_lazy_apply,
dctr_lazy_flush, dctr_lazy_sweep, dctr_lazy_step_inc, dctr_dense_opt_reg), shared by tests/test_lazy_abi_host.py (over the
stand-in library, on the CPU) and tests/test_gpu_lazy_abi.py (on the device).  Not a test file.

A ``LazyCase`` owns, for a list of units ``(vocab, dim, has_deep, has_wide, l2_deep, l2_wide)``:

  one float32 arena   every table, state slab and gradient slab of every unit, and Adam's three tables, each with ``GUARD``
                      sentinel floats in front of and behind it (the sentinel of tests/interaction_abi.py).  Interleaved:
                      a table and its first state slab are strided views of one slab ``[vocab, 2*dim + pad]`` (the wide side
                      ``[vocab, 2 + pad]``), the pad columns hold the sentinel.  Adam's tables sit at the very END of their
                      allocation: the float behind ``adam_ss[n_ss - 1]`` is a sentinel, so a clamp that is one off computes
                      with 777 instead of a stray zero.
  one int32 arena     the stamps of every unit and the step counter, with sentinel bands.
  the structs         ``L.LazyUnit[]`` (copied to the device) and ``L.LazyOpt`` as ``LazyState._ensure`` builds them; the
                      tables are ``LazyState.adam_tables(lr, beta1, beta2)`` -- what the product ships.
  two models          the contract of include/dctr.h in float64 (``ref``) and the same statement in plain float32 numpy
                      (``ref32``): per row (w, s1, s2, stamp) and the gradient slabs.  A replayed step uses
                      g = 2 lambda w, an applied one g = G + 2 lambda w and zeroes G; the target is t (t + 1 for apply);
                      ids outside [0, vocab) mean row 0; the sweep's window is (t mod K) of width ceil(vocab / K).  The step
                      scalars come from the formulas (lr / (1 - beta1^T), sqrt(1 - beta2^T), in double), never from the
                      tables: from the optimizer's doubles when the struct carries tables (that is what the header defines
                      them to hold), from the struct's floats when it carries none (they are all the kernel has).
                      Written from the header and torch.optim -- tests/mock_lib.py's ``_lazy_pass`` is a second,
                      independent statement, and tests/test_lazy_abi_host.py holds the two against each other.

Every call (``catchup / apply / flush / sweep / step_inc``) runs the entry point, then both models, then ``_verify``:

  (a) the int arena equals the model's stamps and step counter exactly (sentinel bands included);
  (b) every float of the arena outside the rows the model touched IN THIS CALL keeps its bits: untouched rows of the table,
      s1, s2, every gradient slab outside an apply's rows, pad columns, guard bands, Adam's tables -- "sentinels intact";
  (c) weights within ``wtol x max(1, max|ref|)``, tests/test_gpu_lazy.py's bars: 1e-4 (RMSprop 3e-4) in the cases whose
      rows replay 300 steps (ids-*, long-gaps-*), 2e-5 in every other case -- no row of those takes more than 43 steps;
  (d) state tensors relative to ``max|ref|`` of the tensor (moments are of order 1e-6) within
      ``max(4 x |ref32 - ref|, 4 float32 ulps)``: what plain float32 loses at this very case, times four for the replay
      loop's 1.5-ulp reciprocal / root against IEEE's 0.5 ulp, three of them per step;
  (e) gradient slabs equal the model's exactly (zero for exactly the applied rows);
  (f) the float64 model's weights stay away from zero (min|w| > 0.05): the normalised steps of Adam / RMSprop make the sign
      of a near-zero weight decide a whole lr, and no comparison with float64 means anything there.

``WORST`` collects the largest ratio per (kind, tensor) and the float32 model's beside it; each check prints its own."""
import ctypes

import numpy as np
import torch

from interaction_abi import GUARD, SENT

ISENT = -777777
EINVAL, ENOSUP = -1, -2
SGD, ADAGRAD, ADAM, RMSPROP = 0, 1, 2, 3
KINDS = ("sgd", "adagrad", "adam", "rmsprop")
KIND_CODE = {"sgd": SGD, "adagrad": ADAGRAD, "adam": ADAM, "rmsprop": RMSPROP}
# (lr, eps, beta1, beta2) as the optimizer holds them, in double; RMSprop: beta2 = alpha, beta1 = 1 - alpha
HYPER = {"sgd": (0.01, 0.0, 0.0, 0.0), "adagrad": (0.01, 1e-10, 0.0, 0.0), "adam": (1e-3, 1e-8, 0.9, 0.999),
         "rmsprop": (1e-3, 1e-8, 1.0 - 0.99, 0.99)}
LAM = 1e-3
SGD_BIG_LAM = 0.1
WTOL_SHORT, WTOL_LONG, WTOL_LONG_RMSPROP = 2e-5, 1e-4, 3e-4
ULP = 2.0 ** -23
WORST = {}          # (kind, tensor) -> [kernel ratio, float32 ratio]
F32 = np.float32


def wtol_long(kind):
    """the bar of the cases whose rows replay 300 steps (ids-*, long-gaps-*); every other case -- at most 43 steps on any row
    -- is held to WTOL_SHORT: plain float32 stays within 1e-5 of float64 even at 300 steps, so no case in between needs more"""
    return WTOL_LONG_RMSPROP if kind == "rmsprop" else WTOL_LONG


def n_states(kind):
    return {"sgd": 0, "adagrad": 1, "rmsprop": 1, "adam": 2}[kind]


# ---- the contract, in one dtype ------------------------------------------------------------------------------------------
class Model(object):
    """include/dctr.h's lazy update on numpy arrays of ``dt``.  The recurrence runs on the floats the structs carry (lr, eps,
    beta1, beta2, lambda); Adam's step scalars are computed from ``hyper``, the optimizer's doubles, as torch does on the
    host (``clock``: from the struct's floats -- the case without tables)."""

    def __init__(self, dt, kind, hyper, tables, t, clock=False):
        self.dt, self.kind, self.t = dt, kind, int(t)
        # Adam's step scalars: from the optimizer's doubles (what the header defines the tables to hold) -- or, when the
        # struct carries no tables and the kernel computes them itself, from the floats of the struct, which are all it has
        # (float(0.999) is 1.3e-8 off: 6e-6 of sqrt(1 - beta2^T) at T = 1)
        self.hyper = tuple(float(F32(h)) for h in hyper) if clock else hyper
        self.lr, self.eps, self.b1, self.b2 = [dt(F32(h)) for h in hyper]
        self.units = []
        for tb in tables:
            u = {"stamp": tb["stamp"].astype(np.int64).copy(), "vocab": tb["vocab"]}
            for side in ("deep", "wide"):
                u[side] = None if tb[side] is None else dict(
                    (k, v.astype(dt).copy()) for k, v in tb[side].items() if k != "lam")
                if tb[side] is not None:
                    u[side]["lam2"] = dt(2) * dt(F32(tb[side]["lam"]))
            self.units.append(u)

    def scalars(self, T):
        lr, _, b1, b2 = self.hyper
        return self.dt(lr / (1.0 - b1 ** T)), self.dt(np.sqrt(1.0 - b2 ** T))

    def step(self, T, g, w, a, b):
        """one optimizer step, number T, on arrays (returns the new w, a, b)"""
        dt = self.dt
        if self.kind == "sgd":
            return w - self.lr * g, a, b
        if self.kind == "adagrad":
            a = a + g * g
            return w - self.lr * (g / (np.sqrt(a) + self.eps)), a, b
        if self.kind == "rmsprop":
            a = a * self.b2 + self.b1 * g * g
            return w - self.lr * (g / (np.sqrt(a) + self.eps)), a, b
        ss, bc = self.scalars(T)
        a = a + (g - a) * (dt(1) - self.b1)
        b = b * self.b2 + (dt(1) - self.b2) * g * g
        return w - ss * (a / (np.sqrt(b) / bc + self.eps)), a, b

    def _advance(self, u, rows, apply):
        """bring ``rows`` of unit u to t (and one applied step further): returns the rows that moved"""
        un = self.units[u]
        target = self.t + 1 if apply else self.t
        rows = np.unique(np.asarray(rows, np.int64))
        rows = rows[un["stamp"][rows] < target]
        if not rows.size:
            return rows
        prev = un["stamp"][rows].copy()
        for side in ("deep", "wide"):
            s = un[side]
            if s is None:
                continue
            w, a, b = s["w"][rows], s["s1"][rows], s["s2"][rows]
            for T in range(int(prev.min()) + 1, self.t + 1):
                on = (prev < T)[:, None]
                w1, a1, b1 = self.step(T, s["lam2"] * w, w, a, b)
                w, a, b = np.where(on, w1, w), np.where(on, a1, a), np.where(on, b1, b)
            if apply:
                w, a, b = self.step(self.t + 1, s["g"][rows] + s["lam2"] * w, w, a, b)
                s["g"][rows] = 0
            s["w"][rows], s["s1"][rows], s["s2"][rows] = w, a, b
        un["stamp"][rows] = target
        return rows

    def rows_of(self, u, ids):
        ids = np.asarray(ids, np.int64)
        return np.where((ids < 0) | (ids >= self.units[u]["vocab"]), 0, ids)

    def catchup(self, ids_t):
        return [self._advance(u, self.rows_of(u, ids_t[u]), False) for u in range(len(self.units))]

    def apply(self, ids_t):
        return [self._advance(u, self.rows_of(u, ids_t[u]), True) for u in range(len(self.units))]

    def flush(self):
        return [self._advance(u, np.arange(un["vocab"]), False) for u, un in enumerate(self.units)]

    def window(self, u, K):
        vocab = self.units[u]["vocab"]
        wlen = -(-vocab // K)
        lo = (self.t % K) * wlen
        return np.arange(min(lo, vocab), min(lo + wlen, vocab))

    def sweep(self, K):
        return [self._advance(u, self.window(u, K), False) for u in range(len(self.units))]

    def step_inc(self):
        self.t += 1
        return [np.zeros(0, np.int64) for _ in self.units]


# ---- the arenas ----------------------------------------------------------------------------------------------------------
class _Arena(object):
    def __init__(self, dtype, sent):
        self.dtype, self.sent = dtype, sent
        self.parts, self.n = [np.full(GUARD, sent, dtype)], GUARD

    def alloc(self, rows, cols, ld=None, col0=0):
        """[rows, cols] with rows ``ld`` apart starting ``col0`` floats into a fresh slab; returns the index array"""
        ld = cols if ld is None else ld
        size = -(-(rows * ld) // 4) * 4          # (keeps every base 16-byte aligned)
        base = self.n
        self.parts.append(np.full(size + GUARD, self.sent, self.dtype))
        self.n += size + GUARD
        return base, base + col0 + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]

    def alloc_at_end(self, values):
        """``values`` flush against the sentinel band behind them"""
        n = len(values)
        lead = (-n) % 4
        base = self.n + lead
        part = np.full(lead + n + GUARD, self.sent, self.dtype)
        part[lead:lead + n] = values
        self.parts.append(part)
        self.n += lead + n + GUARD
        return base

    def build(self):
        return np.concatenate(self.parts)


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


class LazyCase(object):
    """see the module docstring.  ``gaps``: row r of every unit starts ``gaps[r % len(gaps)]`` steps behind ``t`` (an int:
    every row).  ``tables``: Adam only -- "all" (ss, bc, rbc), "norbc" (adam_rbc = NULL), "none" (the in-kernel clock)."""

    def __init__(self, lib, dev, kind, units, t=0, gaps=0, vec=None, interleaved=False, pad=4, betas=None, tables="all",
                 wtol=WTOL_SHORT, seed=0, any_l2=None):
        from deepctr_torch._hip import lib as L
        from deepctr_torch._hip.plan import LazyState
        self.L, self.lib, self.dev, self.kind = L, lib, torch.device(dev), kind
        self.units_spec = [tuple(u) for u in units]
        self.t0, self.wtol = int(t), wtol
        self.stream = L.stream_handle(self.dev)
        rng = self.rng = np.random.RandomState(seed)
        hyper = list(HYPER[kind])
        if betas is not None:
            hyper[2], hyper[3] = betas
        self.hyper = tuple(hyper)
        dims = [d if hd else 1 for (_, d, hd, _, _, _) in self.units_spec]
        self.max_dim = max(dims)
        self.vec = vec if vec is not None else (4 if all(d % 4 == 0 for (_, d, hd, _, _, _) in self.units_spec if hd) else 1)
        self.max_vocab = max(v for (v, _, _, _, _, _) in self.units_spec)
        ns = n_states(kind)
        gaps = np.atleast_1d(np.asarray(gaps, np.int64))
        assert gaps.max() <= self.t0

        fa, ia = _Arena(np.float32, F32(SENT)), _Arena(np.int32, ISENT)
        self.idx, tables_init, host_vals = [], [], []
        gsign = self.gsign = {}
        for (vocab, dim, has_deep, has_wide, l2d, l2w) in self.units_spec:
            stamp = self.t0 - gaps[np.arange(vocab) % len(gaps)]
            entry, tb = {}, {"vocab": vocab, "stamp": stamp, "deep": None, "wide": None}
            for side, on, d, lam in (("deep", has_deep, dim, l2d), ("wide", has_wide, 1, l2w)):
                if not on:
                    continue
                if interleaved:
                    _, iw = fa.alloc(vocab, d, 2 * d + pad)
                    i1 = iw + d
                    ld = 2 * d + pad
                else:
                    _, iw = fa.alloc(vocab, d)
                    _, i1 = fa.alloc(vocab, d)
                    ld = d
                _, i2 = fa.alloc(vocab, d)
                _, ig = fa.alloc(vocab, d)
                entry[side] = {"w": iw, "s1": i1 if ns >= 1 else None, "s2": i2 if ns >= 2 else None, "g": ig, "ld": ld}
                w = (rng.uniform(0.5, 1.5, (vocab, d)) * rng.choice([-1.0, 1.0], (vocab, d))).astype(F32)
                g0 = F32(2) * F32(lam) * w
                old = (stamp > 0)[:, None]
                if kind == "adam":
                    s1, s2 = np.where(old, g0, 0).astype(F32), np.where(old, g0 * g0, 0).astype(F32)
                elif kind == "adagrad":
                    s1, s2 = (stamp[:, None].astype(F32) * g0 * g0).astype(F32), np.zeros_like(w)
                elif kind == "rmsprop":
                    s1, s2 = np.where(old, g0 * g0, 0).astype(F32), np.zeros_like(w)
                else:
                    s1, s2 = np.zeros_like(w), np.zeros_like(w)
                tb[side] = {"w": w, "s1": s1, "s2": s2, "g": np.zeros_like(w), "lam": lam}
                gsign.setdefault(len(self.idx), {})[side] = rng.choice([-1.0, 1.0], (vocab, d))
                host_vals.append((iw, w))
                if ns >= 1:
                    host_vals.append((i1, s1))
                if ns >= 2:
                    host_vals.append((i2, s2))
                host_vals.append((ig, np.zeros_like(w)))
            _, istamp = ia.alloc(vocab, 1)
            entry["stamp"] = istamp[:, 0]
            self.idx.append(entry)
            tables_init.append(tb)
        self.istep = ia.alloc(1, 1)[1][0, 0]
        self.tab = None
        if kind == "adam" and tables != "none":
            ss, bc, rbc = LazyState.adam_tables(*[self.hyper[i] for i in (0, 2, 3)])
            self.tab = (fa.alloc_at_end(ss), len(ss), fa.alloc_at_end(bc), len(bc),
                        fa.alloc_at_end(rbc) if tables == "all" else None)
        host = fa.build()
        for ix, v in host_vals:
            host[ix] = v
        ihost = ia.build()
        for e, tb in zip(self.idx, tables_init):
            ihost[e["stamp"]] = tb["stamp"]
        ihost[self.istep] = self.t0
        self.fa = torch.from_numpy(host).to(self.dev)
        self.ia = torch.from_numpy(ihost).to(self.dev)
        self.ref = Model(np.float64, kind, self.hyper, tables_init, self.t0, clock=self.tab is None)
        self.ref32 = Model(np.float32, kind, self.hyper, tables_init, self.t0, clock=self.tab is None)

        fptr = lambda off: self.fa.data_ptr() + 4 * int(off)          # noqa: E731
        arr = (L.LazyUnit * len(self.units_spec))()
        for u, ((vocab, dim, has_deep, has_wide, l2d, l2w), e) in enumerate(zip(self.units_spec, self.idx)):
            un = arr[u]
            if has_deep:
                d = e["deep"]
                un.deep, un.deep_g = fptr(d["w"][0, 0]), fptr(d["g"][0, 0])
                un.deep_s1 = fptr(d["s1"][0, 0]) if d["s1"] is not None else None
                un.deep_s2 = fptr(d["s2"][0, 0]) if d["s2"] is not None else None
                un.l2_deep = l2d
                un.ld_deep = d["ld"]
                un.ld_deep_s1 = d["ld"] if d["s1"] is not None else 0
            if has_wide:
                d = e["wide"]
                un.wide, un.wide_g = fptr(d["w"][0, 0]), fptr(d["g"][0, 0])
                un.wide_s1 = fptr(d["s1"][0, 0]) if d["s1"] is not None else None
                un.wide_s2 = fptr(d["s2"][0, 0]) if d["s2"] is not None else None
                un.l2_wide = l2w
                un.ld_wide = d["ld"]
                un.ld_wide_s1 = d["ld"] if d["s1"] is not None else 0
            un.stamp = self.ia.data_ptr() + 4 * int(e["stamp"][0])
            un.vocab = vocab
            un.dim = dim if has_deep else 1
            un.col = u
        self.units_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.dev)
        opt = self.opt = L.LazyOpt()
        opt.kind = KIND_CODE[kind]
        opt.lr, opt.eps, opt.beta1, opt.beta2 = self.hyper
        l2_any = any((hd and l2d > 0) or (hw and l2w > 0) for (_, _, hd, hw, l2d, l2w) in self.units_spec)
        opt.any_l2 = int(l2_any if any_l2 is None else any_l2)
        if self.tab is not None:
            o_ss, n_ss, o_bc, n_bc, o_rbc = self.tab
            opt.adam_ss, opt.n_ss, opt.adam_bc, opt.n_bc = fptr(o_ss), n_ss, fptr(o_bc), n_bc
            opt.adam_rbc = fptr(o_rbc) if o_rbc is not None else None
        self.order = None
        self.sync()

    # ---- plumbing ------------------------------------------------------------------------------------------------------
    @property
    def n_units(self):
        return len(self.units_spec)

    def sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)

    def units_ptr(self):
        return ctypes.c_void_p(self.units_dev.data_ptr())

    def step_ptr(self):
        return ctypes.c_void_p(self.ia.data_ptr() + 4 * int(self.istep))

    def snapshot(self):
        self.sync()
        return self.fa.cpu().numpy().copy(), self.ia.cpu().numpy().copy()

    def ids_tensor(self, ids_t):
        ids_t = np.ascontiguousarray(np.asarray(ids_t, np.int32).reshape(self.n_units, -1))
        return ids_t, torch.from_numpy(ids_t.copy()).to(self.dev)

    def order_tensor(self, B):
        """n_units * B ints of scratch between two sentinel bands"""
        self.order = torch.full((self.n_units * B + 2 * GUARD,), ISENT, dtype=torch.int32).to(self.dev)
        return ctypes.c_void_p(self.order.data_ptr() + 4 * GUARD)

    def put_grads(self, ids_t):
        """data gradients |G| in [0.05, 0.5] on the batch's rows (device slabs and both models).  The sign is random per
        element and the same at every step: a row applied at every step with alternating signs makes Adam's exp_avg a
        cancelling sum (0.002 out of terms of 0.05), whose error in ulps of the RESULT is unbounded in any float32
        arithmetic -- a one-row table then fails the state bound by the luck of the draw, not by a fault."""
        ids_t, _ = self.ids_tensor(ids_t)
        pos, val = [], []
        for u, e in enumerate(self.idx):
            rows = np.unique(self.ref.rows_of(u, ids_t[u]))
            for side in ("deep", "wide"):
                if side not in e:
                    continue
                d = e[side]["g"].shape[1]
                G = (self.rng.uniform(0.05, 0.5, (len(rows), d)) * self.gsign[u][side][rows]).astype(F32)
                for m in (self.ref, self.ref32):
                    m.units[u][side]["g"][rows] = G
                pos.append(e[side]["g"][rows].ravel())
                val.append(G.ravel())
        if pos:
            self.fa[torch.from_numpy(np.concatenate(pos)).to(self.dev)] = torch.from_numpy(np.concatenate(val)).to(self.dev)
        self.sync()

    # ---- the entry points ------------------------------------------------------------------------------------------------
    def raw(self, name, ids=None, B=None, K=None, order=None, **over):
        """one entry point with this case's arguments, each replaceable: returns the code (no model, no check)"""
        a = dict(units=self.units_ptr(), n_units=self.n_units, step=self.step_ptr(), opt=ctypes.byref(self.opt),
                 vec=self.vec, max_dim=self.max_dim, max_vocab=self.max_vocab)
        a.update(over)
        lib = self.lib
        if name in ("catchup", "apply"):
            self._ids_dev = ids          # (kept alive over the launch)
            p = ctypes.c_void_p(ids.data_ptr()) if ids is not None else None
            if name == "catchup":
                rc = lib.dctr_lazy_catchup(a["units"], a["n_units"], p, B, a["step"], a["opt"], a["vec"], a["max_dim"], order,
                                           self.stream)
            else:
                rc = lib.dctr_lazy_apply(a["units"], a["n_units"], p, B, a["step"], a["opt"], a["vec"], a["max_dim"],
                                         self.stream)
        elif name == "flush":
            rc = lib.dctr_lazy_flush(a["units"], a["n_units"], a["max_vocab"], a["step"], a["opt"], a["vec"], a["max_dim"],
                                     self.stream)
        elif name == "sweep":
            rc = lib.dctr_lazy_sweep(a["units"], a["n_units"], a["max_vocab"], K, a["step"], a["opt"], a["vec"], a["max_dim"],
                                     self.stream)
        else:
            rc = lib.dctr_lazy_step_inc(a["step"], self.stream)
        self.sync()
        return rc

    def _run(self, name, model_call, verify=True, **kw):
        before = self.snapshot() if verify else None
        rc = self.raw(name, **kw)
        assert rc == 0, "%s %s: code %d" % (self.kind, name, rc)
        touched = model_call(self.ref)
        model_call(self.ref32)
        if verify:
            self._verify(name, before, touched)
        return touched

    def catchup(self, ids_t, order=False, verify=True):
        ids_t, dev = self.ids_tensor(ids_t)
        B = ids_t.shape[1]
        ows = self.order_tensor(B) if order else None
        t_before = self.ref.t
        gaps_before = [un["stamp"].copy() for un in self.ref.units]
        touched = self._run("catchup", lambda m: m.catchup(ids_t), verify, ids=dev, B=B, order=ows)
        if order:
            self._check_order(ids_t, B, t_before, gaps_before)
        return touched

    def apply(self, ids_t, verify=True):
        ids_t, dev = self.ids_tensor(ids_t)
        return self._run("apply", lambda m: m.apply(ids_t), verify, ids=dev, B=ids_t.shape[1])

    def flush(self, verify=True):
        return self._run("flush", lambda m: m.flush(), verify)

    def sweep(self, K, verify=True):
        return self._run("sweep", lambda m: m.sweep(K), verify, K=K)

    def step_inc(self, verify=True):
        return self._run("step_inc", lambda m: m.step_inc(), verify)

    def replays(self):
        return self.kind in ("adam", "rmsprop") or bool(self.opt.any_l2)

    def _check_order(self, ids_t, B, t, stamps):
        """include/dctr.h: with order_ws the catch-up deals every unit's entries by gap -- B >= 64 and a kind that replays
        (SGD / Adagrad only with any_l2): a permutation of 0 .. B-1 per unit, longest gap first; otherwise left alone."""
        self.sync()
        o = self.order.cpu().numpy()
        assert np.all(o[:GUARD] == ISENT) and np.all(o[-GUARD:] == ISENT), "%s: order_ws guard band written" % self.kind
        body = o[GUARD:-GUARD].reshape(self.n_units, B)
        if B >= 64 and self.replays():
            for u in range(self.n_units):
                assert np.array_equal(np.sort(body[u]), np.arange(B)), \
                    "%s: order_ws of unit %d is not a permutation of 0..%d" % (self.kind, u, B - 1)
        else:
            assert np.all(body == ISENT), "%s: order_ws written at B = %d" % (self.kind, B)

    # ---- the check -------------------------------------------------------------------------------------------------------
    def tensors(self, fa=None):
        """(unit, side, name) -> float32 array read from the (snapshot of the) arena through the unit's own strides"""
        fa = self.fa.cpu().numpy() if fa is None else fa
        out = {}
        for u, e in enumerate(self.idx):
            for side in ("deep", "wide"):
                if side in e:
                    for k in ("w", "s1", "s2", "g"):
                        if e[side][k] is not None:
                            out[(u, side, k)] = fa[e[side][k]]
        return out

    def stamps(self, ia=None):
        ia = self.ia.cpu().numpy() if ia is None else ia
        return [ia[e["stamp"]].copy() for e in self.idx]

    def _verify(self, name, before, touched):
        fb, ib = before
        fa, ia = self.snapshot()
        tag = "%s %s" % (self.kind, name)
        # (a) stamps, step counter and their sentinel bands
        want = ib.copy()
        for e, un in zip(self.idx, self.ref.units):
            want[e["stamp"]] = un["stamp"]
        want[self.istep] = self.ref.t
        if not np.array_equal(ia, want):
            bad = np.flatnonzero(ia != want)
            for u, e in enumerate(self.idx):
                rows = np.flatnonzero(ia[e["stamp"]] != want[e["stamp"]])
                assert not rows.size, "%s: stamp of unit %d row %d is %d, the contract says %d" % (
                    tag, u, rows[0], ia[e["stamp"]][rows[0]], want[e["stamp"]][rows[0]])
            assert False, "%s: int arena differs at %s (step counter or a sentinel band)" % (tag, bad[:4])
        # (b) whatever the model did not touch in this call keeps its bits
        may = np.zeros(fa.size, bool)
        for u, e in enumerate(self.idx):
            rows = touched[u]
            for side in ("deep", "wide"):
                if side in e and rows.size:
                    for k in ("w", "s1", "s2") + (("g",) if name == "apply" else ()):
                        if e[side][k] is not None:
                            may[e[side][k][rows].ravel()] = True
        changed = np.flatnonzero((_bits(fa) != _bits(fb)) & ~may)
        assert not changed.size, "%s: %d floats outside the call's rows changed (first at arena offset %d: %r -> %r): " \
            "an untouched row, a pad column, a guard band or a table was written" % (
                tag, changed.size, changed[0], fb[changed[0]], fa[changed[0]])
        # (c) (d) (e) values
        got = self.tensors(fa)
        worst = {}
        for (u, side, k), x in sorted(got.items()):
            r = self.ref.units[u][side][k]
            r32 = self.ref32.units[u][side][k].astype(np.float64)
            assert np.all(np.isfinite(x)), "%s unit %d %s %s: not finite" % (tag, u, side, k)
            err, err32 = float(np.abs(x - r).max()), float(np.abs(r32 - r).max())
            top = float(np.abs(r).max())
            if k == "g":
                assert np.array_equal(x.astype(np.float64), r), "%s unit %d %s gradient slab differs from the contract's" % (
                    tag, u, side)
                continue
            if k == "w":
                scale, bound = max(1.0, top), self.wtol
            else:
                if top == 0.0:
                    assert np.all(x == 0), "%s unit %d %s %s: nonzero where the reference is identically zero" % (
                        tag, u, side, k)
                    continue
                scale = top
                bound = max(4.0 * err32 / scale, 4.0 * ULP)
            key = (self.kind, k)
            w0 = WORST.setdefault(key, [0.0, 0.0])
            w0[0], w0[1] = max(w0[0], err / scale), max(w0[1], err32 / scale)
            cur = worst.setdefault(k, [0.0, 0.0, bound])
            cur[0], cur[1], cur[2] = max(cur[0], err / scale), max(cur[1], err32 / scale), min(cur[2], bound)
            assert err <= bound * scale, "%s unit %d %s %s: max|d| %.3e (scale %.3g) ratio %.3e, bound %.3e " \
                "(plain float32: %.3e)" % (tag, u, side, k, err, scale, err / scale, bound, err32 / scale)
        print("%s t=%d: %s" % (tag, self.ref.t, "  ".join(
            "%s ratio %.2e (float32 %.2e, bound %.2e)" % (k, v[0], v[1], v[2]) for k, v in sorted(worst.items()))))
        # (f)
        lo = min(float(np.abs(un[side]["w"]).min()) for un in self.ref.units for side in ("deep", "wide") if un[side])
        assert lo > 0.05, "%s: a float64 weight came within %.3g of zero: the case is not comparable" % (tag, lo)

    def check(self):
        """the whole state against the models, outside any call"""
        self._verify("state", self.snapshot(), [np.zeros(0, np.int64) for _ in self.idx])

    def bits(self):
        """{(unit, side, tensor): int32 bit patterns} + stamps: what two routes must agree on"""
        out = dict((k, _bits(v.copy())) for k, v in self.tensors().items() if k[2] != "g")
        for u, s in enumerate(self.stamps()):
            out[(u, "stamp")] = s
        return out


def same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        diff = np.flatnonzero(a[k].ravel() != b[k].ravel())
        assert not diff.size, "%s: %s differs in %d of %d elements (first at %d)" % (what, k, diff.size, a[k].size, diff[0])


def batch_ids(rng, vocabs, B, hot=True):
    """[n_units, B]: random rows; with ``hot`` one id five times and the ids -1, vocab, 2^31 - 1 (all row 0)"""
    ids = np.stack([rng.randint(0, v, B) for v in vocabs]).astype(np.int64)
    if hot:
        for u, v in enumerate(vocabs):
            special = [v // 2] * 5 + [-1, v, 2 ** 31 - 1]
            pos = rng.permutation(B)[:len(special)]
            ids[u, pos] = special[:len(pos)]
    return ids.astype(np.int32)


# ---- the case list: (id, fn(lib, dev)) -- both test files run exactly these ------------------------------------------------
def _unit(vocab, dim, deep=True, wide=True, lam=LAM):
    return (vocab, dim, deep, wide, lam, lam)


def geometry(lib, dev, kind, units, vec, interleaved, seed=0):
    """catch-up of rows with gaps 0..8, apply, step_inc, flush.  Row r starts r mod 9 steps behind and the batch is rows
    0..8 (the last row, repeated, of a smaller vocabulary): every gap 0..8 goes through the catch-up, none is left to the
    flush."""
    c = LazyCase(lib, dev, kind, units, t=11, gaps=np.arange(9), vec=vec, interleaved=interleaved, seed=seed)
    ids = np.stack([np.minimum(np.arange(9), u[0] - 1) for u in units]).astype(np.int32)
    c.catchup(ids)
    c.put_grads(ids)
    c.apply(ids)
    c.step_inc()
    c.flush()
    return c


GEOMETRY = [("vec1-dim%d" % d, [_unit(11, d)], 1) for d in (1, 3, 5, 64)] + \
           [("vec4-dim%d" % d, [_unit(11, d)], 4) for d in (4, 8, 20, 64, 256)] + \
           [("vec4-mixed", [_unit(50, 16), _unit(3, 4), _unit(300, 1, deep=False), _unit(1, 16, wide=False)], 4),
            ("vec1-mixed", [_unit(50, 6), _unit(300, 3), _unit(1, 1), _unit(3, 1, deep=False), _unit(7, 6, wide=False)], 1)]


def refusals(lib, dev):
    """nothing is written by a refused or an empty call"""
    for vec, dim in ((1, 5), (4, 8)):
        c = LazyCase(lib, dev, "adam", [_unit(7, dim)], t=5, gaps=np.arange(4), vec=vec)
        before = c.snapshot()
        ids, dids = c.ids_tensor(batch_ids(c.rng, [7], 5, hot=False))
        ows = c.order_tensor(5)
        bad_opt = c.L.LazyOpt()
        bad_opt.kind = 4
        calls = []
        for name, kw in (("catchup", dict(ids=dids, B=5, order=ows)), ("apply", dict(ids=dids, B=5)), ("flush", {}),
                         ("sweep", dict(K=3))):
            calls += [(ENOSUP, name, dict(kw, max_dim=64 * vec + 1)), (EINVAL, name, dict(kw, vec=2)),
                      (EINVAL, name, dict(kw, opt=ctypes.byref(bad_opt))), (EINVAL, name, dict(kw, units=None)),
                      (EINVAL, name, dict(kw, step=None)), (EINVAL, name, dict(kw, opt=None))]
        calls += [(EINVAL, "sweep", dict(K=0)), (EINVAL, "catchup", dict(ids=dids, B=-1, order=ows)),
                  (EINVAL, "apply", dict(ids=dids, B=-1)), (EINVAL, "step_inc", dict(step=None)),
                  (0, "catchup", dict(ids=dids, B=0, order=ows)), (0, "apply", dict(ids=dids, B=0)),
                  (0, "flush", dict(max_vocab=0)), (0, "sweep", dict(K=3, max_vocab=0))]
        for want, name, kw in calls:
            rc = c.raw(name, **kw)
            assert rc == want, "%s(%s): code %d, expected %d" % (name, sorted(kw), rc, want)
            fa, ia = c.snapshot()
            assert np.array_equal(_bits(fa), _bits(before[0])) and np.array_equal(ia, before[1]), \
                "%s(%s) wrote something" % (name, sorted(kw))
            assert bool((c.order == ISENT).all()), "%s(%s) wrote order_ws" % (name, sorted(kw))


def ids_case(lib, dev, kind, B, any_l2=True, seed=3, lam=LAM):
    """duplicates, out-of-range ids, gaps 0..300; with and without order_ws: identical bits"""
    res = []
    lam = lam if any_l2 else 0.0
    for order in (False, True):
        c = LazyCase(lib, dev, kind, [_unit(300, 8, lam=lam), _unit(300, 4, lam=lam)], t=340,
                     gaps=np.r_[0:300:7, 300, 0, 1, 2], wtol=wtol_long(kind), seed=seed)
        ids = batch_ids(c.rng, [300, 300], B, hot=B >= 17)
        if B == 1:
            ids[:, 0] = [-1, 300]
        c.catchup(ids, order=order)
        c.put_grads(ids)
        c.apply(ids)
        c.step_inc()
        c.flush()
        res.append(c.bits())
    same_bits(res[0], res[1], "%s B=%d: order_ws NULL against order_ws given" % (kind, B))


def sweep_case(lib, dev, kind, K, units, t0, seed=5):
    """K consecutive {catchup, sweep, apply, step_inc} from a step that is no multiple of K"""
    c = LazyCase(lib, dev, kind, units, t=t0, gaps=np.r_[0:min(t0, 9)], seed=seed)
    vocabs = [u[0] for u in units]
    for _ in range(K):
        ids = batch_ids(c.rng, vocabs, 5, hot=False)
        c.catchup(ids)
        t = c.ref.t
        before = c.stamps()
        touched = c.sweep(K)
        after = c.stamps()
        for u in range(c.n_units):
            win = c.ref.window(u, K)
            moved = np.flatnonzero(after[u] != before[u])
            assert np.array_equal(moved, win[before[u][win] < t]), "sweep K=%d t=%d unit %d: rows %s moved, window %s" % (
                K, t, u, moved, win)
            assert np.array_equal(touched[u], moved)
            assert np.all(after[u][win] == t)
        c.put_grads(ids)
        c.apply(ids)
        c.step_inc()
    for u, s in enumerate(c.stamps()):
        assert c.ref.t - s.min() <= K, "after K = %d steps a stamp of unit %d is %d behind" % (K, u, c.ref.t - s.min())
    c.flush()
    for s in c.stamps():
        assert np.all(s == c.ref.t)


SWEEP = [("K7", 7, [_unit(50, 8), _unit(3, 4), _unit(1, 4)], 10), ("K1", 1, [_unit(5, 4)], 3),
         ("K64-wlen1", 64, [_unit(50, 4)], 70), ("K7-vec1", 7, [_unit(50, 3), _unit(3, 1, deep=False)], 12)]


def adam_scalars_case(lib, dev, betas, start, tables, route, vec=4):
    """gaps of 12 steps across the end of a table (or far past both): catch-up / flush / apply"""
    c = LazyCase(lib, dev, "adam", [_unit(6, 8 if vec == 4 else 3)], t=start + 12, gaps=[12, 12, 5, 0, 12, 1], vec=vec,
                 betas=betas, tables=tables, seed=7)
    ids = np.array([[0, 1, 2, 3, 0]], np.int32)
    if route == "flush":
        c.flush()
    else:
        c.catchup(ids)
        if route == "apply":
            c.put_grads(ids)
            c.apply(ids)
            c.step_inc()
            c.catchup(ids)          # a second applied step: T = t + 1 one further past the table's end
            c.put_grads(ids)
            c.apply(ids)
            c.step_inc()
        c.flush()


def adam_starts(betas):
    from deepctr_torch._hip.plan import LazyState
    ss, bc, _ = LazyState.adam_tables(HYPER["adam"][0], *betas)
    out = [("n_ss-6", len(ss) - 6), ("n_bc-6", len(bc) - 6)]
    return out + ([("1e6", 1000000)] if betas == (0.5, 0.9) else [])


ADAM_SCALARS = [("%s-%s-%s-%s" % ("fast" if betas == (0.5, 0.9) else "default", sname, tables, route), betas, start, tables, route)
                for betas in ((0.5, 0.9), (0.9, 0.999)) for sname, start in adam_starts(betas)
                for tables in ("all", "norbc", "none") for route in ("catchup", "flush", "apply")]


def long_gaps(lib, dev, kind, start, tables="all", lam=LAM):
    """gap 300 on every row, then one wavefront's 16 rows with 16 different gaps, through catch-up and through flush"""
    units = [_unit(16, 4, lam=lam), _unit(16, 8, lam=lam)]
    c = LazyCase(lib, dev, kind, units, t=start + 300, gaps=300, tables=tables, wtol=wtol_long(kind), seed=start)
    ids = np.stack([np.arange(16), np.arange(16)[::-1]]).astype(np.int32)
    c.catchup(ids)
    c.flush()
    stairs = np.r_[1, 20:301:20]
    assert len(stairs) == 16
    for route in ("catchup", "flush"):
        c = LazyCase(lib, dev, kind, units, t=start + 300, gaps=stairs, tables=tables, wtol=wtol_long(kind),
                     seed=start + 1)
        if route == "catchup":
            c.catchup(ids)
        c.flush()


def routes(lib, dev, kind, tables="all", dims=(8, 4), vec=None, seed=11):
    """one initial state, no data gradients, 40 steps: who replays a (row, step) never changes its bits.
    A: 40 step_inc, one flush.  B: every step catch-up of 17 random ids and sweep(7).  C: as B without the sweep and with
    order_ws given -- at B = 17 the ordering pass stays off (``_check_order`` holds the scratch to its sentinel), so C is the
    catch-up alone.  D: every fifth step a catch-up of 70 random ids with order_ws: ``k_lazy_order`` runs, over gaps 0..8."""
    units = [_unit(40, dims[0]), _unit(9, dims[1])]
    vocabs = [40, 9]

    def run(route, vec):
        c = LazyCase(lib, dev, kind, units, t=3, gaps=[0, 1, 2, 3], vec=vec, tables=tables, seed=seed)
        rng = np.random.RandomState(seed + 1)
        for i in range(40):
            if route == "D":
                if i % 5 == 4:
                    c.catchup(batch_ids(rng, vocabs, 70, hot=False), order=True, verify=False)
            elif route != "A":
                ids = batch_ids(rng, vocabs, 17, hot=False)
                c.catchup(ids, order=route == "C", verify=False)
                if route == "B":
                    c.sweep(7, verify=False)
            c.step_inc(verify=False)
        c.flush()
        return c.bits()
    a = run("A", vec)
    b = run("B", vec)
    same_bits(a, b, "%s: 40 step_inc + flush against catch-up + sweep + flush" % kind)
    same_bits(a, run("C", vec), "%s: 40 step_inc + flush against catch-up with order_ws + flush" % kind)
    same_bits(a, run("D", vec), "%s: 40 step_inc + flush against ordered catch-ups of 70 + flush" % kind)
    same_bits(b, run("B", vec), "%s: two runs of catch-up + sweep + flush" % kind)
    if vec is None and all(d % 4 == 0 for d in dims):
        same_bits(a, run("A", 1), "%s: vec = 4 against vec = 1 (flush)" % kind)
        same_bits(b, run("B", 1), "%s: vec = 4 against vec = 1 (catch-up + sweep)" % kind)


# ---- dctr_dense_opt_reg ----------------------------------------------------------------------------------------------------
class DenseCase(object):
    """p, g, s1, s2, lam of n floats each between sentinel bands; three successive steps against both models"""

    def __init__(self, lib, dev, kind, n, lam=True, t=0, tables="all", betas=None, states=None, seed=0):
        from deepctr_torch._hip import lib as L
        from deepctr_torch._hip.plan import LazyState
        self.L, self.lib, self.dev, self.kind, self.n = L, lib, torch.device(dev), kind, n
        self.stream = L.stream_handle(self.dev)
        rng = self.rng = np.random.RandomState(seed)
        hyper = list(HYPER[kind])
        if betas is not None:
            hyper[2], hyper[3] = betas
        self.hyper = tuple(hyper)
        ns = n_states(kind) if states is None else states
        fa = _Arena(np.float32, F32(SENT))
        self.ix = dict((k, fa.alloc(1, n)[1][0]) for k in ("p", "g", "s1", "s2", "lam"))
        self.has = {"p": True, "g": True, "s1": ns >= 1, "s2": ns >= 2, "lam": bool(lam)}
        tab = None
        if kind == "adam" and tables != "none":
            ss, bc, rbc = LazyState.adam_tables(*[self.hyper[i] for i in (0, 2, 3)])
            tab = (fa.alloc_at_end(ss), len(ss), fa.alloc_at_end(bc), len(bc), fa.alloc_at_end(rbc))
        host = fa.build()
        w = (rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
        lamv = rng.uniform(0.0, 2e-3, n).astype(F32)
        g0 = F32(2) * lamv * w
        s1 = {"adam": g0, "adagrad": F32(t) * g0 * g0, "rmsprop": g0 * g0, "sgd": 0 * g0}[kind] if t > 0 else 0 * g0
        s2 = g0 * g0 if (kind == "adam" and t > 0) else 0 * g0
        host[self.ix["p"]] = w
        if self.has["s1"]:
            host[self.ix["s1"]] = s1
        if self.has["s2"]:
            host[self.ix["s2"]] = s2
        if lam:
            host[self.ix["lam"]] = lamv
        self.fa = torch.from_numpy(host).to(self.dev)
        self.step = torch.tensor([ISENT, t, ISENT], dtype=torch.int32).to(self.dev)
        opt = self.opt = L.LazyOpt()
        opt.kind = KIND_CODE[kind]
        opt.lr, opt.eps, opt.beta1, opt.beta2 = self.hyper
        opt.any_l2 = int(bool(lam))
        if tab is not None:
            opt.adam_ss, opt.n_ss, opt.adam_bc, opt.n_bc = self.ptr(tab[0]), tab[1], self.ptr(tab[2]), tab[3]
            opt.adam_rbc = self.ptr(tab[4])
        self.models = []
        for dt in (np.float64, np.float32):
            m = Model(dt, kind, self.hyper, [], t, clock=tab is None)
            m.p, m.s1, m.s2 = w.astype(dt), s1.astype(dt), s2.astype(dt)
            m.lam2 = dt(2) * lamv.astype(dt) if lam else dt(0) * lamv.astype(dt)
            self.models.append(m)

    def ptr(self, off):
        return self.fa.data_ptr() + 4 * int(off)

    def arg(self, k):
        return ctypes.c_void_p(self.ptr(self.ix[k][0])) if self.has[k] else None

    def sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)

    def call(self, **over):
        a = dict(p=self.arg("p"), g=self.arg("g"), s1=self.arg("s1"), s2=self.arg("s2"), lam=self.arg("lam"), n=self.n,
                 opt=ctypes.byref(self.opt), step=ctypes.c_void_p(self.step.data_ptr() + 4))
        a.update(over)
        rc = self.lib.dctr_dense_opt_reg(a["p"], a["g"], a["s1"], a["s2"], a["lam"], a["n"], a["opt"], a["step"], self.stream)
        self.sync()
        return rc

    def run(self, steps=3):
        tag = "dense_opt_reg %s n=%d" % (self.kind, self.n)
        for _ in range(steps):
            G = (self.rng.uniform(0.05, 0.5, self.n) * self.rng.choice([-1.0, 1.0], self.n)).astype(F32)
            self.fa[torch.from_numpy(self.ix["g"]).to(self.dev)] = torch.from_numpy(G).to(self.dev)
            self.sync()
            before = self.fa.cpu().numpy().copy()
            assert self.call() == 0
            after = self.fa.cpu().numpy()
            may = np.zeros(after.size, bool)
            for k in ("p", "s1", "s2"):
                if self.has[k]:
                    may[self.ix[k]] = True
            assert np.array_equal(_bits(after)[~may], _bits(before)[~may]), "%s: a float outside p / s1 / s2 was written" % tag
            for m in self.models:
                m.p, m.s1, m.s2 = m.step(m.t + 1, G.astype(m.dt) + m.lam2 * m.p, m.p, m.s1, m.s2)
            r, r32 = self.models
            for k, wtol in (("p", WTOL_SHORT), ("s1", None), ("s2", None)):
                if not self.has[k]:
                    continue
                x, ref, ref32 = after[self.ix[k]], getattr(r, k), getattr(r32, k).astype(np.float64)
                err, err32, top = float(np.abs(x - ref).max()), float(np.abs(ref32 - ref).max()), float(np.abs(ref).max())
                scale = max(1.0, top) if k == "p" else top
                bound = wtol if k == "p" else max(4.0 * err32 / scale, 4.0 * ULP)
                w0 = WORST.setdefault(("dense " + self.kind, k), [0.0, 0.0])
                w0[0], w0[1] = max(w0[0], err / scale), max(w0[1], err32 / scale)
                print("%s T=%d %s: ratio %.2e (float32 %.2e, bound %.2e)" % (tag, r.t + 1, k, err / scale, err32 / scale, bound))
                assert np.all(np.isfinite(x)) and err <= bound * scale, "%s T=%d %s: max|d| %.3e (scale %.3g), bound %.3e" % (
                    tag, r.t + 1, k, err, scale, bound)
            assert self.lib.dctr_lazy_step_inc(ctypes.c_void_p(self.step.data_ptr() + 4), self.stream) == 0
            self.sync()
            for m in self.models:
                m.t += 1
            assert self.step.cpu().tolist() == [ISENT, r.t, ISENT], "%s: the step counter or its neighbours" % tag

    def refused(self, **over):
        before = self.fa.cpu().numpy().copy()
        rc = self.call(**over)
        assert rc == EINVAL, "dense_opt_reg %s (%s): code %d" % (self.kind, sorted(over), rc)
        assert np.array_equal(_bits(self.fa.cpu().numpy()), _bits(before)), "a refused dctr_dense_opt_reg wrote something"


def dense_case(lib, dev, kind, n, lam):
    from deepctr_torch._hip.plan import LazyState
    DenseCase(lib, dev, kind, n, lam=lam, t=0, seed=n).run()
    if kind == "adam":
        ss, bc, _ = LazyState.adam_tables(*[HYPER["adam"][i] for i in (0, 2, 3)])
        for t in (len(ss) - 1, len(bc) - 1):
            DenseCase(lib, dev, kind, n, lam=lam, t=t, seed=n + 1).run()
        DenseCase(lib, dev, kind, n, lam=lam, t=len(ss) - 1, tables="none", seed=n + 2).run()
    if kind == "sgd":
        DenseCase(lib, dev, kind, n, lam=lam, t=5, seed=n + 3).run()          # (s1 = s2 = NULL by construction)


def dense_refusals(lib, dev):
    for kind, missing in (("adagrad", "s1"), ("rmsprop", "s1"), ("adam", "s2"), ("adam", "s1")):
        DenseCase(lib, dev, kind, 257, seed=1).refused(**{missing: None})
    c = DenseCase(lib, dev, "sgd", 257, seed=2)
    c.refused(p=None)
    c.refused(g=None)
    c.refused(opt=None)
    c.refused(step=None)
    c.refused(n=-1)
    before = c.fa.cpu().numpy().copy()
    assert c.call(n=0) == 0
    assert np.array_equal(_bits(c.fa.cpu().numpy()), _bits(before))


DENSE_N = (1, 255, 256, 257, 1000)
ID_B = (1, 17, 63, 64, 65, 300)


def case_list():
    """[(id, fn(lib, dev))]: every case of tests/test_gpu_lazy_abi.py; tests/test_lazy_abi_host.py runs the same list"""
    out = []
    for kind in KINDS:
        for name, units, vec in GEOMETRY:
            for inter in (False, True):
                out.append(("geometry-%s-%s-%s" % (kind, name, "interleaved" if inter else "contiguous"),
                            lambda lib, dev, k=kind, u=units, v=vec, i=inter: geometry(lib, dev, k, u, v, i)))
    # SGD keeps no state, and at lambda = 1e-3 one replayed step moves a weight by lr * 2 lambda |w| <= 3e-5 -- the size of the
    # short bar itself: a lost or doubled step would pass.  At lambda = 0.1 it is 2e-3 |w| >= 5e-4 (|w| >= 0.27 after 300
    # steps of decay), 3 times the widest bar used, through every kernel that counts steps
    big = SGD_BIG_LAM
    out.append(("geometry-sgd-lam0.1-vec4-dim8", lambda lib, dev: geometry(lib, dev, "sgd", [_unit(11, 8, lam=big)], 4, False)))
    out.append(("geometry-sgd-lam0.1-vec1-dim5", lambda lib, dev: geometry(lib, dev, "sgd", [_unit(11, 5, lam=big)], 1, True)))
    out.append(("ids-sgd-lam0.1-B17", lambda lib, dev: ids_case(lib, dev, "sgd", 17, lam=big)))
    out.append(("ids-sgd-lam0.1-B65", lambda lib, dev: ids_case(lib, dev, "sgd", 65, lam=big)))
    out.append(("sweep-sgd-lam0.1-K7", lambda lib, dev: sweep_case(
        lib, dev, "sgd", 7, [_unit(50, 8, lam=big), _unit(3, 4, lam=big), _unit(1, 4, lam=big)], 10)))
    out.append(("long-gaps-sgd-lam0.1-from40", lambda lib, dev: long_gaps(lib, dev, "sgd", 40, lam=big)))
    out.append(("refusals", refusals))
    for kind in KINDS:
        for B in ID_B:
            out.append(("ids-%s-B%d" % (kind, B), lambda lib, dev, k=kind, B=B: ids_case(lib, dev, k, B)))
    for kind in ("sgd", "adagrad"):
        out.append(("ids-%s-no-l2-B65" % kind, lambda lib, dev, k=kind: ids_case(lib, dev, k, 65, any_l2=False)))
    for kind in KINDS:
        for name, K, units, t0 in SWEEP:
            out.append(("sweep-%s-%s" % (kind, name),
                        lambda lib, dev, k=kind, K=K, u=units, t0=t0: sweep_case(lib, dev, k, K, u, t0)))
    for name, betas, start, tables, route in ADAM_SCALARS:
        out.append(("adam-scalars-" + name,
                    lambda lib, dev, b=betas, s=start, t=tables, r=route: adam_scalars_case(lib, dev, b, s, t, r)))
    out.append(("adam-scalars-fast-n_ss-6-all-catchup-vec1",
                lambda lib, dev: adam_scalars_case(lib, dev, (0.5, 0.9), adam_starts((0.5, 0.9))[0][1], "all", "catchup", 1)))
    for kind in KINDS:
        for start in (0, 40):
            out.append(("long-gaps-%s-from%d" % (kind, start), lambda lib, dev, k=kind, s=start: long_gaps(lib, dev, k, s)))
    out.append(("long-gaps-adam-clock-from0", lambda lib, dev: long_gaps(lib, dev, "adam", 0, tables="none")))
    for kind in KINDS:
        out.append(("routes-%s" % kind, lambda lib, dev, k=kind: routes(lib, dev, k)))
        out.append(("routes-%s-vec1-odd-dims" % kind, lambda lib, dev, k=kind: routes(lib, dev, k, dims=(5, 3))))
    out.append(("routes-adam-clock", lambda lib, dev: routes(lib, dev, "adam", tables="none")))
    out.append(("routes-adam-norbc", lambda lib, dev: routes(lib, dev, "adam", tables="norbc")))
    for kind in KINDS:
        for lam in (True, False):
            for n in DENSE_N:
                out.append(("dense-%s-n%d-%s" % (kind, n, "lam" if lam else "nolam"),
                            lambda lib, dev, k=kind, n=n, l=lam: dense_case(lib, dev, k, n, l)))
    out.append(("dense-refusals", dense_refusals))
    return out
