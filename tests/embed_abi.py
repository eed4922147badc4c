"""Driver for the fused lookup and the deterministic sorted update THROUGH THE C ABI (include/dctr.h: dctr_embed_fwd,
dctr_embed_ids, dctr_embed_segments, dctr_embed_update, dctr_embed_bwd, dctr_embed_apply; csrc/embed.hip, csrc/update.hip),
shared by tests/test_embed_abi_host.py (over the stand-in library, on the CPU) and tests/test_gpu_embed_abi.py (on the
device).  Not a test file.

An ``EmbedCase`` owns a plan of SIMPLE units ``(vocab, dim | 0, has_wide)`` -- unit u reads X column u and feeds a deep table
of ``dim`` floats per row and / or a wide table of one -- built by hand with ctypes (``L.Field``, ``L.Plan``, the ``units``
``[n][4]`` array), so that every byte a kernel can reach belongs to the test:

  one float32 arena   every table, Adagrad state slab and gacc slab, X, out, g_out, fm_s, fm, wide, g_wide, g_fm, g_wdense,
                      Linear.weight and its state, each with ``GUARD`` sentinel floats (tests/interaction_abi.py's 777) in
                      front of and behind it.  Contiguous tables (``ld = 0``) or interleaved: table and state are strided
                      views of one slab ``[vocab, 2*dim + pad]`` (wide: ``[vocab, 2 + pad]``), the pad columns hold the
                      sentinel.  X is ``[B, n_xcols + xpad]``; out / g_out / fm_s / wide / g_wide have padded leading
                      dimensions; every pad column holds the sentinel.
  one int32 arena     units, dense_cols, wdense_cols, ids_t / parts_t of the forward and of dctr_embed_ids, err, and the
                      bucket workspace: exactly dctr_embed_update_workspace_ints ints, zero inside, a sentinel band behind.
  two models          the header's contract in float64 (``ref``) and the same statement in plain float32 numpy (``ref32``),
                      which sums a row's duplicates once in sample order and once in reverse: the kernel's segment sum runs
                      backwards and the hot-id path uses a tree, so no single order is "the" float32 answer.  Ids truncate
                      toward zero like Tensor.long(); an id outside [0, vocab) means row 0 (and bit 0 of err in the forward);
                      FM's backward is g_fm * (S - e) with e the row before the step and S the fm_s the caller passes;
                      SGD p -= lr G; Adagrad s += G*G, p -= lr G / (sqrt(s) + eps); ACCUM gacc += G.  Both models start from
                      the arena as it stood before the call.  Written from include/dctr.h and torch.optim, not from
                      tests/mock_lib.py -- tests/test_embed_abi_host.py holds the two against each other.

Hyper-parameters make the step as large as the table: SGD lr = 1, Adagrad lr = 0.5 with every state element preset in
[0.05, 0.5], tables N(0, 0.5), gradients N(0, 1): the table after the step shows the summed gradient G at full scale.

Every call verifies
  (a) integer outputs exactly: ids_t, parts_t (= clamp(id) mod dctr_embed_update_partitions, and dctr_embed_ids' equal to the
      forward's), err; after dctr_embed_update the workspace's counters are zero again and the band behind it is intact;
  (b) the forward's copies bit for bit: out's field slices are the table rows, the dense block is X;
  (c) every float outside what the header says is written keeps its bits: pad columns, guard bands, every input buffer, and
      every table / state / gacc row whose id is not in the batch, in all three modes;
  (d) floating-point results against ``ref`` per tensor over max|ref| of the tensor (no floor of 1; a reference that is
      identically zero must come back exactly zero) within ``TOL[tensor]``;
  (e) the sorted update twice from the same arena gives the same bits, and so does every route through it;
  (f) a second ACCUM launch onto a non-zero gacc gives 2 G.
``WORST`` records the kernel's and ``ref32``'s largest ratio per (entry point, tensor)."""
import ctypes

import numpy as np
import torch

from interaction_abi import GRAD_TOL, GUARD, OUT_TOL, SENT
from lazy_abi import ISENT, _Arena, _bits

EINVAL, ENOSUP, EALIGN = -1, -2, -3
SGD, ADAGRAD, ACCUM, LAZY = 0, 1, 2, 3
OPT_NAME = {SGD: "sgd", ADAGRAD: "adagrad", ACCUM: "accum"}
LR = {SGD: 1.0, ADAGRAD: 0.5, ACCUM: 0.0}
EPS = 1e-10
F32 = np.float32
KBUCKET = 512          # keys per (unit, partition) bucket: include/dctr.h's workspace is n_units * P * (1 + 512) ints at least
# (d): the starting bounds of tests/interaction_abi.py; tests/test_embed_abi_host.py asserts that plain float32, in both
# orders, stays within a quarter of each at every case of the list
TOL = {"wide": OUT_TOL, "fm": OUT_TOL, "fm_s": OUT_TOL, "table": GRAD_TOL, "state": GRAD_TOL, "gacc": GRAD_TOL,
       "g_wdense": GRAD_TOL, "wdense_w": GRAD_TOL, "wdense_s": GRAD_TOL}
# ... and where it does not, four times the largest deviation of plain float32 over the list (never anything a kernel
# returned): dctr_embed_update's table 1.763e-5, state 9.170e-6, gacc 5.145e-6 -- all three from update-routes-*-B16384 and
# update-skew-*, where one row takes 520 to 655 entries and float32 adds them one at a time
# update-general-dim*-hot (about 2000 entries of a pooled history on one row): table 8.251e-6, state 5.564e-6.  (Measured
# over the stand-in, where tests/test_embed_abi_host.py asserts the rule; on a device the float32 model starts from the
# device forward's out / fm_s, other last bits, and its own deviation moves -- it is printed there, not asserted.)
WIDENED = {("update", "table"): 7.06e-5, ("update", "state"): 3.67e-5, ("update", "gacc"): 2.06e-5,
           ("update-general", "table"): 3.305e-5, ("update-general", "state"): 2.23e-5}
WORST = {}          # (entry point, tensor) -> [kernel ratio, float32 ratio]


def tol(entry, tensor):
    return WIDENED.get((entry, tensor), TOL[tensor])


def _round_up(x, m):
    return -(-x // m) * m


def seg_sum(rows, G, reverse):
    """rows [n], G [n, d] -> (uniq rows, their sums): every row's duplicates added one at a time in sample order (or in
    reverse), in G's dtype"""
    order = np.argsort(rows, kind="stable")
    r, Gs = rows[order], G[order]
    uniq, start, cnt = np.unique(r, return_index=True, return_counts=True)
    acc = np.zeros((len(uniq), G.shape[1]), G.dtype)
    for k in range(int(cnt.max()) if len(cnt) else 0):
        on = cnt > k
        acc[on] += Gs[start[on] + ((cnt[on] - 1 - k) if reverse else k)]
    return uniq, acc


class EmbedCase(object):
    """see the module docstring.  ``units``: [(vocab, dim | 0, has_wide)]; ``ids``: None (random rows) or {unit: float values
    of the first samples' X entries}."""

    def __init__(self, lib, dev, units, B, vec=None, interleaved=False, pad=4, xpad=3, n_dense=0, dense_off=True, n_wdense=0,
                 wdense_w=True, wpf=False, ld_wide=3, wide_in_out=False, ld_gw=1, ids=None, flags=None, seed=0):
        from deepctr_torch._hip import lib as L
        self.L, self.lib, self.dev, self.B = L, lib, torch.device(dev), int(B)
        self.units_spec = [tuple(u) for u in units]
        self.stream = L.stream_handle(self.dev)
        rng = self.rng = np.random.RandomState(seed)
        nu = self.n_units = len(self.units_spec)
        dims = [d for (_, d, _) in self.units_spec if d]
        self.n_deep, self.n_wide = len(dims), sum(1 for u in self.units_spec if u[2])
        self.emb_dim = dims[0] if dims and all(d == dims[0] for d in dims) else 0
        self.max_dim = max(dims) if dims else 0
        if vec is None:
            vec = 1 if not dims else (4 if all(d % 4 == 0 for d in dims) else (2 if all(d % 2 == 0 for d in dims) else 1))
        self.vec, self.wpf = vec, bool(wpf)
        self.n_dense, self.n_wdense = n_dense, n_wdense
        self.n_emb = sum(dims)
        self.dense_off = self.n_emb if (dense_off and n_dense) else -1
        self.n_xcols = nu + n_dense + n_wdense
        self.ldx = self.n_xcols + xpad
        self.ld_out = _round_up(self.n_emb + n_dense + 1, 4) + 4
        self.ld_s = _round_up(max(self.emb_dim, 1), 4) + 4
        self.ld_gw = (self.n_wide + 1 + (ld_gw - 1)) if wpf else ld_gw
        self.wide_in_out = wide_in_out
        self.wide_col = self.n_emb + n_dense          # (wide as a column of out: the first column behind the dense block)
        self.ld_wide = self.ld_out if wide_in_out else ((self.n_wide + 1 + (ld_wide - 1)) if wpf else ld_wide)
        self.max_vocab = max(v for (v, _, _) in self.units_spec)

        # ---- the plan's scalars first: the library sizes the workspace from them -------------------------------------
        plan = self.plan = L.Plan()
        plan.n_deep = plan.n_deep_fixed = self.n_deep
        plan.n_wide = plan.n_wide_fixed = self.n_wide
        plan.n_dense, plan.n_wdense, plan.dense_off = n_dense, n_wdense, self.dense_off
        plan.emb_dim, plan.n_xcols, plan.max_dim, plan.vec = self.emb_dim, self.n_xcols, self.max_dim, vec
        plan.flags = (L.PLAN_HAS_GACC | L.PLAN_HAS_STATE if flags is None else flags) | (L.PLAN_WIDE_PER_FIELD if wpf else 0)
        self.P = int(lib.dctr_embed_update_partitions(ctypes.byref(plan), B)) if B > 0 else 1
        self.ws_ints = int(lib.dctr_embed_update_workspace_ints(ctypes.byref(plan), nu, B)) if B > 0 else 0
        assert self.ws_ints >= nu * self.P * (1 + KBUCKET) or B <= 0, "workspace of %d ints for %d buckets" % (
            self.ws_ints, nu * self.P)

        # ---- arenas ---------------------------------------------------------------------------------------------------
        fa, ia = _Arena(np.float32, F32(SENT)), _Arena(np.int32, ISENT)
        self.reg, self.ireg, init = {}, {}, []
        self.fields = {"deep": [], "wide": []}          # per field: dict(unit, vocab, dim, off, w, s, g, ld)
        unit_rows, off = [], 0
        for u, (vocab, dim, has_wide) in enumerate(self.units_spec):
            row = [-1, -1, u, 0]
            for side, d in (("deep", dim), ("wide", 1 if has_wide else 0)):
                if not d:
                    continue
                if interleaved:
                    ld = 2 * d + pad
                    _, iw = fa.alloc(vocab, d, ld)
                    i_s = iw + d
                else:
                    ld = 0
                    _, iw = fa.alloc(vocab, d)
                    _, i_s = fa.alloc(vocab, d)
                _, ig = fa.alloc(vocab, d)
                f = dict(unit=u, vocab=vocab, dim=d, off=off if side == "deep" else 0, w=iw, s=i_s, g=ig, ld=ld)
                row[0 if side == "deep" else 1] = len(self.fields[side])
                self.fields[side].append(f)
                init += [(iw, rng.normal(0, 0.5, (vocab, d))), (i_s, rng.uniform(0.05, 0.5, (vocab, d))), (ig, np.zeros((vocab, d)))]
                if side == "deep":
                    off += d
            unit_rows.append(row)
        R = self.reg
        Bn = max(self.B, 1)
        _, R["X"] = fa.alloc(Bn, self.n_xcols, self.ldx)
        _, R["out"] = fa.alloc(Bn, self.ld_out, self.ld_out)          # (the whole padded row: slices are views of it)
        _, R["g_out"] = fa.alloc(Bn, max(self.n_emb + n_dense, 1), self.ld_out)
        _, R["fm_s"] = fa.alloc(Bn, max(self.emb_dim, 1), self.ld_s)
        _, R["fm"] = fa.alloc(1, Bn)
        _, R["g_fm"] = fa.alloc(1, Bn)
        if wide_in_out:
            R["wide"] = R["out"][:, self.wide_col:self.wide_col + 1]
        else:
            _, R["wide"] = fa.alloc(Bn, (self.n_wide + 1) if wpf else 1, self.ld_wide)
        _, R["g_wide"] = fa.alloc(Bn, (self.n_wide + 1) if wpf else 1, self.ld_gw)
        nwd = max(n_wdense, 1)
        for k in ("g_wdense", "wdense_w", "wdense_s"):
            _, R[k] = fa.alloc(1, nwd)
        IR = self.ireg
        _, IR["units"] = ia.alloc(nu, 4)
        _, IR["dense_cols"] = ia.alloc(1, max(n_dense, 1))
        _, IR["wdense_cols"] = ia.alloc(1, nwd)
        for k in ("ids_t", "ids2"):
            _, IR[k] = ia.alloc(nu, Bn)
        for k in ("parts_t", "parts2"):          # uint16 [n_units, B] in int32 words
            _, IR[k] = ia.alloc(1, (nu * Bn + 1) // 2)
        _, IR["err"] = ia.alloc(1, 1)
        _, IR["ws"] = ia.alloc(1, max(self.ws_ints, 1))
        host, ihost = fa.build(), ia.build()
        for ix, v in init:
            host[ix] = v.astype(F32)

        # ---- inputs -----------------------------------------------------------------------------------------------------
        X = np.zeros((Bn, self.n_xcols), F32)
        for u, (vocab, _, _) in enumerate(self.units_spec):
            X[:, u] = rng.randint(0, vocab, Bn)
            if ids is not None and u in ids:
                vals = np.asarray(ids[u], F32)
                X[:len(vals), u] = vals[:Bn]
        X[:, nu:] = rng.normal(0, 1, (Bn, n_dense + n_wdense))
        host[R["X"]] = X
        host[R["g_out"]] = rng.normal(0, 1, R["g_out"].shape)
        host[R["g_fm"]] = rng.normal(0, 1, R["g_fm"].shape)
        host[R["g_wide"]] = rng.normal(0, 1, R["g_wide"].shape)
        host[R["wdense_w"]] = rng.normal(0, 0.5, (1, nwd))
        host[R["wdense_s"]] = rng.uniform(0.05, 0.5, (1, nwd))
        ihost[IR["units"]] = np.asarray(unit_rows, np.int32)
        ihost[IR["dense_cols"]] = 0
        ihost[IR["wdense_cols"]] = 0
        ihost[IR["dense_cols"][0, :n_dense]] = nu + np.arange(n_dense)
        ihost[IR["wdense_cols"][0, :n_wdense]] = nu + n_dense + np.arange(n_wdense)
        ihost[IR["err"]] = 0
        ihost[IR["ws"]] = 0
        self.fa = torch.from_numpy(host).to(self.dev)
        self.ia = torch.from_numpy(ihost).to(self.dev)
        self.f0, self.i0 = self.fa.clone(), self.ia.clone()

        # ---- descriptors ------------------------------------------------------------------------------------------------
        self._desc = {}
        for side in ("deep", "wide"):
            n = len(self.fields[side])
            arr = (L.Field * max(n, 1))()
            for i, f in enumerate(self.fields[side]):
                a = arr[i]
                a.table, a.gacc, a.state = self.fptr(f["w"][0, 0]), self.fptr(f["g"][0, 0]), self.fptr(f["s"][0, 0])
                a.vocab, a.dim, a.col, a.len, a.pool, a.len_col = f["vocab"], f["dim"], f["unit"], 1, 0, -1
                a.out_off, a.ld, a.ld_state = f["off"], f["ld"], f["ld"]
            self._desc[side] = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.dev)
        plan.deep = self._desc["deep"].data_ptr() if self.n_deep else None
        plan.wide = self._desc["wide"].data_ptr() if self.n_wide else None
        plan.dense_cols = self.iptr("dense_cols") if n_dense else None
        plan.wdense_cols = self.iptr("wdense_cols") if n_wdense else None
        plan.wdense_w = self.fptr(R["wdense_w"][0, 0]) if (n_wdense and wdense_w) else None
        self.has_wdense_w = bool(n_wdense and wdense_w)
        self.sync()

    # ---- plumbing ----------------------------------------------------------------------------------------------------------
    def fptr(self, off):
        return self.fa.data_ptr() + 4 * int(off)

    def rptr(self, name):
        return ctypes.c_void_p(self.fptr(self.reg[name].ravel()[0]))

    def _ptr_or(self, on, name):
        """a flag -> the case's own buffer or NULL; a pointer (a refusal case's) -> itself"""
        if isinstance(on, ctypes.c_void_p):
            return on
        return self.rptr(name) if on else None

    def iptr(self, name):
        return self.ia.data_ptr() + 4 * int(self.ireg[name].ravel()[0])

    def ip(self, name):
        return ctypes.c_void_p(self.iptr(name))

    def sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)

    def snapshot(self):
        self.sync()
        return self.fa.cpu().numpy().copy(), self.ia.cpu().numpy().copy()

    def save(self):
        """what ``restore`` returns to: the arena with the forward's outputs in it"""
        self.sync()
        self.f0, self.i0 = self.fa.clone(), self.ia.clone()

    def restore(self):
        self.fa.copy_(self.f0)
        self.ia.copy_(self.i0)
        self.sync()

    def unit_vocab(self, u):
        return self.units_spec[u][0]

    def ids_of(self, X):
        """[n_units, B] int64: Tensor.long() of the id columns -- truncation toward zero"""
        return np.trunc(X[:, :self.n_units].astype(np.float64)).astype(np.int64).T

    def rows_of(self, ids):
        vocab = np.asarray([v for (v, _, _) in self.units_spec], np.int64)[:, None]
        bad = (ids < 0) | (ids >= vocab)
        return np.where(bad, 0, ids), bad

    def _record(self, entry, tensor, x, r, r32s, tag):
        """(d): x (float32 result), r (float64), r32s (float32 models) -> asserts, WORST"""
        assert np.all(np.isfinite(x)), "%s %s: not finite" % (tag, tensor)
        top = float(np.abs(r).max()) if r.size else 0.0
        if top == 0.0:
            assert np.all(x == 0), "%s %s: nonzero where the reference is identically zero" % (tag, tensor)
            return
        err = float(np.abs(x.astype(np.float64) - r).max()) / top
        err32 = max(float(np.abs(q.astype(np.float64) - r).max()) for q in r32s) / top
        w = WORST.setdefault((entry, tensor), [0.0, 0.0])
        w[0], w[1] = max(w[0], err), max(w[1], err32)
        assert err <= tol(entry, tensor), "%s %s: max|d| / max|ref| %.3e (max|ref| %.3g), bound %.2e (plain float32: %.3e)" % (
            tag, tensor, err, top, tol(entry, tensor), err32)

    def _unchanged(self, tag, fb, fa, may, ib, ia, want_i, imay=None):
        changed = np.flatnonzero((_bits(fa) != _bits(fb)) & ~may)
        assert not changed.size, "%s: %d floats outside what the call writes changed (first at arena offset %d: %r -> %r): " \
            "an untouched row, a pad column, a guard band or an input buffer was written" % (
                tag, changed.size, changed[0], fb[changed[0]], fa[changed[0]])
        diff = ia != want_i
        if imay is not None:
            diff &= ~imay
        bad = np.flatnonzero(diff)
        if bad.size:
            for k, ix in sorted(self.ireg.items()):
                hit = np.intersect1d(bad, ix.ravel())
                assert not hit.size, "%s: int buffer %s differs from the contract at arena offset %d (%d, expected %d)" % (
                    tag, k, hit[0], ia[hit[0]], want_i[hit[0]])
            assert False, "%s: an int sentinel band was written at %s" % (tag, bad[:4])

    # ---- dctr_embed_fwd / dctr_embed_ids -------------------------------------------------------------------------------
    def fwd_args(self, out=True, wide=True, fm=True, fm_s=True, side=True, parts=True, err=True, **over):
        p = self._ptr_or
        a = dict(plan=ctypes.byref(self.plan), X=self.rptr("X"), ldx=self.ldx, B=self.B, out=p(out, "out"), ld_out=self.ld_out,
                 wide=p(wide, "wide"), ld_wide=self.ld_wide, fm=p(fm, "fm"), err=self.ip("err") if err else None,
                 units=self.ip("units") if side else None, n_units=self.n_units if side else 0,
                 ids_t=self.ip("ids_t") if side else None, parts_t=self.ip("parts_t") if (side and parts) else None,
                 fm_s=p(fm_s, "fm_s"), ld_s=self.ld_s)
        a.update(over)
        return a

    def raw_fwd(self, **kw):
        a = self.fwd_args(**kw)
        rc = self.lib.dctr_embed_fwd(a["plan"], a["X"], a["ldx"], a["B"], a["out"], a["ld_out"], a["wide"], a["ld_wide"],
                                     a["fm"], a["err"], a["units"], a["n_units"], a["ids_t"], a["parts_t"], a["fm_s"],
                                     a["ld_s"], self.stream)
        self.sync()
        return rc

    def raw_ids(self, plan=True, parts=True, **over):
        a = dict(plan=ctypes.byref(self.plan) if plan else None, units=self.ip("units"), n_units=self.n_units,
                 X=self.rptr("X"), ldx=self.ldx, B=self.B, ids_t=self.ip("ids2"), parts_t=self.ip("parts2") if parts else None)
        a.update(over)
        rc = self.lib.dctr_embed_ids(a["plan"], a["units"], a["n_units"], a["X"], a["ldx"], a["B"], a["ids_t"], a["parts_t"],
                                     self.stream)
        self.sync()
        return rc

    def forward_models(self, fb):
        """{tensor: (float64, [float32 in field order, float32 in reverse field order])} and the rows / bad flag"""
        R = self.reg
        X = fb[R["X"]]
        rows, bad = self.rows_of(self.ids_of(X))
        res = {}
        for dt, key in ((np.float64, 0), (np.float32, 1), (np.float32, 2)):
            order = (lambda l: l[::-1]) if key == 2 else (lambda l: l)
            S = np.zeros((self.B, max(self.emb_dim, 1)), dt)
            Q = np.zeros_like(S)
            if self.emb_dim:
                for f in order(self.fields["deep"]):
                    e = fb[f["w"]][rows[f["unit"]]].astype(dt)
                    S += e
                    Q += e * e
            nw = self.n_wide
            W = np.zeros((self.B, nw + 1 if self.wpf else 1), dt)
            for i, f in order(list(enumerate(self.fields["wide"]))):
                W[:, i if self.wpf else 0] += fb[f["w"]][rows[f["unit"]], 0].astype(dt)
            if self.has_wdense_w:
                ww = fb[R["wdense_w"]][0].astype(dt)
                for j in order(list(range(self.n_wdense))):
                    W[:, nw if self.wpf else 0] += X[:, self.n_units + self.n_dense + j].astype(dt) * ww[j]
            fm = dt(0.5) * (S * S - Q).sum(axis=1)
            for name, v in (("wide", W), ("fm", fm[None, :]), ("fm_s", S)):
                if key == 0:
                    res[name] = (v, [])
                else:
                    res[name][1].append(v)
        return res, rows, bad

    def fwd(self, **kw):
        """dctr_embed_fwd (+ dctr_embed_ids into the second pair of buffers when the side outputs are on), checked"""
        opt = dict(out=True, wide=True, fm=True, fm_s=True, side=True, parts=True, err=True)
        opt.update(kw)
        if not self.emb_dim or not opt["out"]:
            opt["fm"] = opt["fm_s"] = False
        tag = "embed_fwd B=%d %s" % (self.B, ",".join(k for k in sorted(opt) if opt[k]))
        fb, ib = self.snapshot()
        rc = self.raw_fwd(**opt)
        assert rc == 0, "%s: code %d" % (tag, rc)
        if opt["side"]:
            rc = self.raw_ids(parts=opt["parts"])
            assert rc == 0, "dctr_embed_ids: code %d" % rc
        fa, ia = self.snapshot()
        R, IR = self.reg, self.ireg
        res, rows, bad = self.forward_models(fb)
        X = fb[R["X"]]
        may = np.zeros(fa.size, bool)
        # (b) copies
        if opt["out"]:
            O = fa[R["out"]]
            for f in self.fields["deep"]:
                sl = slice(f["off"], f["off"] + f["dim"])
                may[R["out"][:, sl].ravel()] = True
                assert np.array_equal(_bits(O[:, sl]), _bits(fb[f["w"]][rows[f["unit"]]])), \
                    "%s: out's slice of deep field %d is not the table row, bit for bit" % (tag, f["unit"])
            if self.dense_off >= 0:
                sl = slice(self.dense_off, self.dense_off + self.n_dense)
                may[R["out"][:, sl].ravel()] = True
                assert np.array_equal(_bits(O[:, sl]), _bits(X[:, self.n_units:self.n_units + self.n_dense])), \
                    "%s: the dense block of out is not X's columns" % tag
        # (d) floats
        for name in ("wide", "fm", "fm_s"):
            if not opt[name]:
                continue
            ix = R[name] if name != "fm_s" else R["fm_s"][:, :max(self.emb_dim, 1)]
            if name == "wide" and self.wpf:
                ix = R["wide"][:, :self.n_wide + 1]
            may[ix.ravel()] = True
            r, r32s = res[name]
            self._record("fwd", name, fa[ix].reshape(r.shape), r, r32s, tag)
        # (a) ints
        want = ib.copy()
        if opt["err"]:          # (an id is range-checked where its table is read: deep tables with out, wide ones with wide)
            seen = [f["unit"] for f in self.fields["deep"]] * bool(opt["out"]) + \
                   [f["unit"] for f in self.fields["wide"]] * bool(opt["wide"])
            want[IR["err"]] = 1 if bad[seen].any() else 0
        if opt["side"]:
            ids32 = self.ids_of(X).astype(np.int32)
            want[IR["ids_t"]] = ids32
            want[IR["ids2"]] = ids32
            tags = (rows % self.P).astype(np.uint16)
            for k in (("parts_t", "parts2") if opt["parts"] else ()):
                w16 = want[IR[k][0]].view(np.uint16).copy()
                w16[:tags.size] = tags.ravel()
                want[IR[k][0]] = w16.view(np.int32)
        self._unchanged(tag, fb, fa, may, ib, ia, want)
        return res

    # ---- dctr_embed_update / dctr_embed_segments -----------------------------------------------------------------------
    def dense_step(self, kind):
        if kind is None:
            return None
        s = self._wd_step = self.L.DenseStep()
        s.kind, s.lr, s.eps = kind, LR[kind], EPS
        s.grad_base = self.fptr(self.reg["g_wdense"][0, 0])
        s.param_base = self.fptr(self.reg["wdense_w"][0, 0])
        s.state_base = self.fptr(self.reg["wdense_s"][0, 0]) if kind == ADAGRAD else None
        return ctypes.byref(s)

    def upd_args(self, opt=SGD, g_out=True, g_fm=True, g_wide=True, parts=True, ws=None, g_wdense=False, wd_step=None, **over):
        p = self._ptr_or
        a = dict(plan=ctypes.byref(self.plan), units=self.ip("units"), n_units=self.n_units, max_vocab=self.max_vocab,
                 ids_t=self.ip("ids_t"), parts_t=self.ip("parts_t") if parts else None, B=self.B, g_out=p(g_out, "g_out"),
                 ld_g=self.ld_out, out=self.rptr("out"), ld_out=self.ld_out, fm_s=p(g_fm, "fm_s"), ld_s=self.ld_s,
                 g_fm=p(g_fm, "g_fm"), g_wide=p(g_wide, "g_wide"), ld_gw=self.ld_gw, opt=opt, lr=LR.get(opt, 0.0), eps=EPS,
                 X=self.rptr("X"), ld_x=self.ldx, g_wdense=p(g_wdense, "g_wdense"), wdense_step=self.dense_step(wd_step),
                 workspace=self.ip("ws") if ws else None, workspace_ints=self.ws_ints if ws else 0,
                 presorted=1 if ws == "presorted" else 0)
        a.update(over)
        return a

    def raw_update(self, **kw):
        a = self.upd_args(**kw)
        rc = self.lib.dctr_embed_update(
            a["plan"], a["units"], a["n_units"], a["max_vocab"], a["ids_t"], a["parts_t"], a["B"], a["g_out"], a["ld_g"],
            a["out"], a["ld_out"], a["fm_s"], a["ld_s"], a["g_fm"], a["g_wide"], a["ld_gw"], a["opt"], a["lr"], a["eps"],
            a["X"], a["ld_x"], a["g_wdense"], a["wdense_step"], a["workspace"], a["workspace_ints"], a["presorted"],
            self.stream)
        self.sync()
        return rc

    def raw_segments(self, parts=True, **over):
        a = dict(plan=ctypes.byref(self.plan), units=self.ip("units"), n_units=self.n_units, max_vocab=self.max_vocab,
                 ids_t=self.ip("ids_t"), parts_t=self.ip("parts_t") if parts else None, B=self.B, workspace=self.ip("ws"),
                 workspace_ints=self.ws_ints)
        a.update(over)
        rc = self.lib.dctr_embed_segments(a["plan"], a["units"], a["n_units"], a["max_vocab"], a["ids_t"], a["parts_t"],
                                          a["B"], a["workspace"], a["workspace_ints"], self.stream)
        self.sync()
        return rc

    def entry_grads(self, fb, dt, g_out, g_fm, g_wide):
        """per field: (rows [B], G [B, dim]) -- what every sample contributes to its row, in ``dt``"""
        R = self.reg
        rows, _ = self.rows_of(fb_ids(self, fb))
        out = {"deep": [], "wide": []}
        gO = fb[R["g_out"]].astype(dt)
        gF = fb[R["g_fm"]][0].astype(dt)
        S = fb[R["fm_s"]].astype(dt)
        gW = fb[R["g_wide"]].astype(dt)
        for f in self.fields["deep"]:
            r = rows[f["unit"]]
            if not (g_out or g_fm):
                out["deep"].append(None)
                continue
            G = np.zeros((self.B, f["dim"]), dt)
            if g_out:
                G += gO[:, f["off"]:f["off"] + f["dim"]]
            if g_fm:
                G += gF[:, None] * (S[:, :f["dim"]] - fb[f["w"]][r].astype(dt))
            out["deep"].append((r, G))
        for i, f in enumerate(self.fields["wide"]):
            out["wide"].append((rows[f["unit"]], gW[:, (i if self.wpf else 0):(i if self.wpf else 0) + 1].copy()) if g_wide else None)
        return out

    def update_models(self, fb, opt, g_out, g_fm, g_wide, g_wdense, wd_step):
        """{(side, field, tensor) | name: (float64, [float32 forward order, float32 reverse order])}, touched rows"""
        R = self.reg
        res, touched = {}, {}
        for key, dt, rev in ((0, np.float64, False), (1, np.float32, False), (2, np.float32, True)):
            grads = self.entry_grads(fb, dt, g_out, g_fm, g_wide)
            lr, eps = dt(F32(LR[opt])), dt(F32(EPS))
            for side in ("deep", "wide"):
                for i, (f, eg) in enumerate(zip(self.fields[side], grads[side])):
                    if eg is None:
                        continue
                    uniq, G = seg_sum(eg[0], eg[1], rev)
                    touched[(side, i)] = uniq
                    w, s, g = fb[f["w"]].astype(dt), fb[f["s"]].astype(dt), fb[f["g"]].astype(dt)
                    if opt == SGD:
                        w[uniq] = w[uniq] - lr * G
                        new = {"table": w}
                    elif opt == ADAGRAD:
                        s[uniq] = s[uniq] + G * G
                        w[uniq] = w[uniq] - lr * (G / (np.sqrt(s[uniq]) + eps))
                        new = {"table": w, "state": s}
                    else:
                        g[uniq] = g[uniq] + G
                        new = {"gacc": g}
                    for k, v in new.items():
                        if key == 0:
                            res[(side, i, k)] = (v, [])
                        else:
                            res[(side, i, k)][1].append(v)
            if g_wdense:
                X = fb[R["X"]].astype(dt)
                gW = fb[R["g_wide"]][:, self.n_wide if self.wpf else 0].astype(dt)
                cols = self.n_units + self.n_dense + np.arange(self.n_wdense)
                idx = np.arange(self.B)[::-1] if rev else np.arange(self.B)
                gd = np.zeros(self.n_wdense, dt)
                for b in idx:
                    gd += gW[b] * X[b, cols]
                new = {"g_wdense": gd[None, :]}
                if wd_step is not None:
                    p = fb[R["wdense_w"]][0, :self.n_wdense].astype(dt)
                    s = fb[R["wdense_s"]][0, :self.n_wdense].astype(dt)
                    l2, e2 = dt(F32(LR[wd_step])), dt(F32(EPS))
                    if wd_step == ADAGRAD:
                        s = s + gd * gd
                        p = p - l2 * (gd / (np.sqrt(s) + e2))
                        new["wdense_s"] = s[None, :]
                    else:
                        p = p - l2 * gd
                    new["wdense_w"] = p[None, :]
                for k, v in new.items():
                    if key == 0:
                        res[k] = (v, [])
                    else:
                        res[k][1].append(v)
        return res, touched

    def update(self, opt=SGD, g_out=True, g_fm=True, g_wide=True, parts=True, ws=None, g_wdense=False, wd_step=None,
               segments_parts=True, reuse=False):
        """dctr_embed_update (behind dctr_embed_segments when ``ws == "presorted"``), checked; returns the models.
        ``reuse``: the arena and the arguments are those of the previous call (another route): its models stand."""
        g_fm = bool(g_fm and self.emb_dim)
        g_wide = bool(g_wide)
        tag = "embed_update %s B=%d%s%s%s ws=%s%s" % (OPT_NAME[opt], self.B, " g_out" if g_out else "", " g_fm" if g_fm else "",
                                                       " g_wide" if g_wide else "", ws, "" if parts else " parts_t=NULL")
        fb, ib = self.snapshot()
        if ws == "presorted":
            rc = self.raw_segments(parts=segments_parts)
            assert rc == 0, "dctr_embed_segments: code %d" % rc
        rc = self.raw_update(opt=opt, g_out=g_out, g_fm=g_fm, g_wide=g_wide, parts=parts, ws=ws, g_wdense=g_wdense,
                             wd_step=wd_step)
        assert rc == 0, "%s: code %d" % (tag, rc)
        fa, ia = self.snapshot()
        margs = (opt, g_out, g_fm, g_wide, g_wdense, wd_step)
        if reuse:
            assert self._last[0] == margs
        else:
            self._last = (margs,) + self.update_models(fb, *margs)
        res, touched = self._last[1:]
        may = np.zeros(fa.size, bool)
        for key, (r, r32s) in sorted(res.items(), key=str):
            if isinstance(key, tuple):
                side, i, k = key
                f = self.fields[side][i]
                ix = f[{"table": "w", "state": "s", "gacc": "g"}[k]]
                may[ix[touched[(side, i)]].ravel()] = True
                self._record("update", k, fa[ix], r, r32s, "%s %s field %d" % (tag, side, i))
            else:
                ix = self.reg[key][:, :self.n_wdense]
                may[ix.ravel()] = True
                self._record("update", key, fa[ix], r, r32s, tag)
        IR = self.ireg
        imay = np.zeros(ia.size, bool)
        if ws:          # counters zero again; the keys behind them are the library's to leave as it likes; band intact
            imay[IR["ws"][0, self.n_units * self.P:self.ws_ints]] = True
        self._unchanged(tag, fb, fa, may, ib, ia, ib, imay)
        return res

    def table_bits(self):
        """{(side, field, tensor): int32 bit patterns} of every table, state and gacc slab (+ the dense half)"""
        fa = self.snapshot()[0]
        out = {}
        for side in ("deep", "wide"):
            for i, f in enumerate(self.fields[side]):
                for k in ("w", "s", "g"):
                    out[(side, i, k)] = _bits(fa[f[k]].copy())
        for k in ("g_wdense", "wdense_w", "wdense_s"):
            out[k] = _bits(fa[self.reg[k]].copy())
        return out

    # ---- dctr_embed_bwd / dctr_embed_apply (float atomics: (d) only) -----------------------------------------------------
    def raw_bwd(self, mode=0, g_out=True, g_fm=True, g_wide=True, **over):
        p = self._ptr_or
        a = dict(plan=ctypes.byref(self.plan), X=self.rptr("X"), ldx=self.ldx, B=self.B, g_out=p(g_out, "g_out"),
                 ld_g=self.ld_out, out=self.rptr("out"), ld_out=self.ld_out, g_fm=p(g_fm, "g_fm"), g_wide=p(g_wide, "g_wide"),
                 mode=mode, lr=LR[SGD])
        a.update(over)
        rc = self.lib.dctr_embed_bwd(a["plan"], a["X"], a["ldx"], a["B"], a["g_out"], a["ld_g"], a["out"], a["ld_out"],
                                     a["g_fm"], a["g_wide"], a["mode"], a["lr"], self.stream)
        self.sync()
        return rc

    def raw_apply(self, opt=0, **over):
        a = dict(plan=ctypes.byref(self.plan), X=self.rptr("X"), ldx=self.ldx, B=self.B, opt=opt, lr=LR[opt], eps=EPS)
        a.update(over)
        rc = self.lib.dctr_embed_apply(a["plan"], a["X"], a["ldx"], a["B"], a["opt"], a["lr"], a["eps"], self.stream)
        self.sync()
        return rc

    def bwd(self, mode, g_fm=True):
        """dctr_embed_bwd: mode 0 adds into gacc, mode 1 steps the table (SGD); the model is the update's (S = out's field sum
        is what the forward left in fm_s -- the same floats in another association, inside the bound)"""
        assert self.ld_gw == 1 or self.wpf
        g_fm = bool(g_fm and self.emb_dim)
        tag = "embed_bwd mode=%d B=%d%s" % (mode, self.B, " g_fm" if g_fm else "")
        fb, ib = self.snapshot()
        rc = self.raw_bwd(mode=mode, g_fm=g_fm)
        assert rc == 0, "%s: code %d" % (tag, rc)
        fa, ia = self.snapshot()
        res, touched = self.update_models(fb, ACCUM if mode == 0 else SGD, True, g_fm, True, False, None)
        may = np.zeros(fa.size, bool)
        for (side, i, k), (r, r32s) in sorted(res.items(), key=str):
            f = self.fields[side][i]
            ix = f[{"table": "w", "gacc": "g"}[k]]
            may[ix[touched[(side, i)]].ravel()] = True
            self._record("bwd", k, fa[ix], r, r32s, "%s %s field %d" % (tag, side, i))
        self._unchanged(tag, fb, fa, may, ib, ia, ib)

    def apply(self, opt):
        """dctr_embed_apply: consumes the batch's gacc rows (exactly zero afterwards), steps table (and state)"""
        tag = "embed_apply %s B=%d" % (OPT_NAME[opt], self.B)
        fb, ib = self.snapshot()
        rc = self.raw_apply(opt=opt)
        assert rc == 0, "%s: code %d" % (tag, rc)
        fa, ia = self.snapshot()
        rows, _ = self.rows_of(fb_ids(self, fb))
        may = np.zeros(fa.size, bool)
        for side in ("deep", "wide"):
            for i, f in enumerate(self.fields[side]):
                uniq = np.unique(rows[f["unit"]])
                models = []
                for dt in (np.float64, np.float32):
                    lr, eps = dt(F32(LR[opt])), dt(F32(EPS))
                    w, s, G = fb[f["w"]].astype(dt), fb[f["s"]].astype(dt), fb[f["g"]][uniq].astype(dt)
                    if opt == ADAGRAD:
                        s[uniq] = s[uniq] + G * G
                        w[uniq] = w[uniq] - lr * (G / (np.sqrt(s[uniq]) + eps))
                    else:
                        w[uniq] = w[uniq] - lr * G
                    models.append((w, s))
                for k, j in (("w", 0),) + ((("s", 1),) if opt == ADAGRAD else ()):
                    may[f[k][uniq].ravel()] = True
                    self._record("apply", "table" if k == "w" else "state", fa[f[k]], models[0][j], [models[1][j]],
                                 "%s %s field %d" % (tag, side, i))
                may[f["g"][uniq].ravel()] = True
                assert np.all(fa[f["g"]] == 0), "%s %s field %d: gacc is not exactly zero after the apply" % (tag, side, i)
        self._unchanged(tag, fb, fa, may, ib, ia, ib)


def fb_ids(case, fb):
    """the batch's ids, from the snapshot's X"""
    return case.ids_of(fb[case.reg["X"]])


def same_bits(a, b, what):
    assert sorted(a, key=str) == sorted(b, key=str)
    for k in sorted(a, key=str):
        diff = np.flatnonzero(a[k].ravel() != b[k].ravel())
        assert not diff.size, "%s: %s differs in %d of %d elements (first at %d)" % (what, k, diff.size, a[k].size, diff[0])


# ---- lane geometry, as the header's callers see it ------------------------------------------------------------------------
def lookup_lpr(dim, vec):
    """lanes per sample of dctr_embed_fwd: the smallest power of two covering dim / vec (SPB = 64 / lpr samples a workgroup)"""
    lpr = 1
    while lpr * vec < dim:
        lpr *= 2
    return lpr


def update_tile(dim, vec, common=True):
    """entries per tile of the sorted update, G = 256 / lpr: vec 4 rows of a common dim % 8 == 0, <= 64 move as vec 8"""
    if vec == 4 and common and dim % 8 == 0 and dim <= 64:
        vec = 8
    return 256 // lookup_lpr(max(dim, 1), vec)


def vec_of(dim):
    return 4 if dim % 4 == 0 else (2 if dim % 2 == 0 else 1)


# ---- the cases ------------------------------------------------------------------------------------------------------------
LOOKUP_DIMS = (4, 8, 16, 20, 64, 128, 256, 2, 6, 30, 1, 3, 5, 33)
# (vec, lpr) of lane_layout(): (8,1) (8,2) (8,4) (8,8) | (4,1) (4,4) (4,8) (4,16) (4,32) (4,64) | (2,1) (2,4) (2,8) (2,16) (2,32)
# (2,64) | (1,1) (1,4) (1,8) (1,16) (1,32) (1,64); the three pairs no natural dim selects are in FORCED_PAIRS below
UPDATE_DIMS = (8, 16, 32, 64, 4, 12, 20, 36, 128, 256, 2, 6, 10, 30, 34, 66, 1, 3, 5, 9, 17, 33)
# (4,2): mixed dims 4 and 8 (emb_dim = 0 keeps vec 4); (2,2): dim 4 declared with vec 2; (1,2): dim 2 declared with vec 1
FORCED_PAIRS = [("vec4-lpr2", [(50, 4, True), (7, 8, False), (7, 0, True)], 8, 4, False),
                ("vec2-lpr2", [(50, 4, True), (7, 4, False), (7, 0, True)], 4, 2, True),
                ("vec1-lpr2", [(50, 2, True), (7, 2, False), (7, 0, True)], 2, 1, True)]
MIXED = [(50, 4, True), (7, 8, False), (9, 20, True), (7, 0, True)]


def geometry_units(dim):
    """one launch holds units of all three kinds: deep + wide, deep only, wide only"""
    return [(50, dim, True), (7, dim, False), (7, 0, True)]


def lookup_grid(lib, dev, dim, interleaved):
    """dctr_embed_fwd at B = 1, SPB - 1, SPB, SPB + 1 with every output on"""
    vec = vec_of(dim)
    spb = 64 // lookup_lpr(dim, vec)
    for B in sorted(set(b for b in (1, spb - 1, spb, spb + 1) if b >= 1)):
        EmbedCase(lib, dev, geometry_units(dim), B, interleaved=interleaved, n_dense=3, n_wdense=2, seed=dim + B).fwd()


def lookup_shape(lib, dev, units, **kw):
    for B in (3, 65):
        EmbedCase(lib, dev, units, B, seed=B, **kw).fwd()


def lookup_outputs(lib, dev):
    """the output combinations of dctr_embed_fwd on one plan (dim 8, LPR = 2)"""
    units = geometry_units(8)
    for B in (5, 65):
        mk = lambda **kw: EmbedCase(lib, dev, units, B, n_dense=3, n_wdense=2, seed=B, **kw)          # noqa: E731
        mk().fwd(wide=False, fm=False, fm_s=False, side=False)          # out only
        mk().fwd(out=False, side=False)                                 # wide only (out = NULL)
        mk().fwd(wide=False, fm_s=False, side=False)                    # fm without wide
        mk().fwd(fm=False, side=False)                                  # fm_s (padded ld_s) without fm
        mk(ld_wide=1).fwd()                                             # wide as a plain vector
        mk(wide_in_out=True).fwd()                                      # wide as a column of out
        mk(wpf=True).fwd()                                              # DCTR_PLAN_WIDE_PER_FIELD, ld_wide = n_wide + 1 + pad
        mk(wpf=True, ld_wide=1).fwd()                                   # ... and ld_wide = n_wide + 1
        mk().fwd(parts=False)                                           # ids_t without parts_t
        mk().fwd(err=False)
        mk(xpad=0).fwd()                                                # ldx == n_xcols: the contiguous tile copy


def lookup_ids(lib, dev, interleaved):
    """3.9 and -0.5 in X mean ids 3 and 0, no error; -1, vocab and 2^20 mean row 0 with err bit 0; vocab 1"""
    units = [(11, 8, True), (1, 8, True), (5, 0, True)]
    c = EmbedCase(lib, dev, units, 6, interleaved=interleaved, ids={0: [3.9, -0.5, 10.99, 0.0]}, seed=1)
    c.fwd()
    assert int(c.snapshot()[1][c.ireg["err"][0, 0]]) == 0, "a clean batch (3.9, -0.5, 10.99) set err"
    for k, bad in enumerate((-1.0, 11.0, float(2 ** 20))):
        for u in (0, 2):
            c = EmbedCase(lib, dev, units, 6, interleaved=interleaved, ids={u: [3.9, bad]}, seed=2 + k)
            c.fwd()
            assert int(c.snapshot()[1][c.ireg["err"][0, 0]]) == 1, "id %r in unit %d did not set err bit 0" % (bad, u)


def skew_ids(c, n_hot):
    """the first ``n_hot`` samples of unit 0 alternate between ids 1 and 1 + P (one partition, two segments)"""
    assert 1 + c.P < c.unit_vocab(0)
    return {0: [1 + c.P * (i % 2) for i in range(n_hot)]}


def update_sweep(c, e_check=True, modes=(SGD, ADAGRAD, ACCUM), combos=((True, True), (True, False), (False, True)),
                 routes=(None,)):
    """forward, then every mode x (g_out, g_fm) combination from the same arena; the first combination twice (e), ACCUM
    twice without a reset (f)"""
    c.fwd()
    c.save()
    for opt in modes:
        for n, (g_out, g_fm) in enumerate(combos):
            if g_fm and not c.emb_dim and not g_out:
                continue
            first = None
            for ws in routes:
                c.restore()
                c.update(opt=opt, g_out=g_out, g_fm=g_fm, ws=ws, reuse=first is not None)
                bits = c.table_bits()
                if first is None:
                    first = bits
                    if n == 0 and e_check:
                        c.restore()
                        c.raw_update(opt=opt, g_out=g_out, g_fm=bool(g_fm and c.emb_dim), ws=ws)
                        same_bits(first, c.table_bits(), "%s B=%d: two launches from the same arena" % (OPT_NAME[opt], c.B))
                else:
                    same_bits(first, bits, "%s B=%d: route ws=%s against the first" % (OPT_NAME[opt], c.B, ws))
            if opt == ACCUM and n == 0:
                # (f) a second launch onto the non-zero gacc: the float64 model from a zero slab, doubled
                c.restore()
                res = c.update(opt=ACCUM, g_out=g_out, g_fm=g_fm)
                c.update(opt=ACCUM, g_out=g_out, g_fm=g_fm)
                fa = c.snapshot()[0]
                for (side, i, k), (r, _) in res.items():
                    top = float(np.abs(r).max())
                    if top > 0:
                        err = float(np.abs(fa[c.fields[side][i]["g"]] - 2.0 * r).max()) / (2.0 * top)
                        assert err <= tol("update", "gacc"), "ACCUM twice, %s field %d: gacc is not 2 G (ratio %.3e)" % (side, i, err)


def update_geometry(lib, dev, units, dim, vec, interleaved, common=True):
    """B = 1, G - 1, G, G + 1 and one batch that puts 1.5 G + 1 entries of two ids into one partition (the carry between
    tiles), G = 256 / lpr; contiguous tables with ld_gw = 1, interleaved with ld_gw = 3"""
    G = update_tile(dim, vec, common)
    kw = dict(vec=vec, interleaved=interleaved, ld_gw=3 if interleaved else 1)
    for B in sorted(set(b for b in (1, G - 1, G, G + 1) if b >= 1)):
        update_sweep(EmbedCase(lib, dev, units, B, seed=B, **kw), e_check=(B == G + 1))
    B = 2 * G + 3
    probe = EmbedCase(lib, dev, units, B, seed=B, **kw)
    n_hot = min(G + G // 2 + 1, KBUCKET)
    c = EmbedCase(lib, dev, units, B, seed=B, ids=skew_ids(probe, n_hot), **kw)
    update_sweep(c, routes=(None, "bucket", "presorted"))


def p_change(lib, dev, dim):
    """the batch sizes on either side of a change of dctr_embed_update_partitions"""
    units = geometry_units(dim)
    probe = EmbedCase(lib, dev, units, 1)
    parts = lambda B: int(lib.dctr_embed_update_partitions(ctypes.byref(probe.plan), B))          # noqa: E731
    G = update_tile(dim, vec_of(dim))
    B = next(b for b in range(2 * G, 40 * G + 40) if parts(b) != parts(b + 1))
    for b in (B, B + 1):
        update_sweep(EmbedCase(lib, dev, units, b, seed=b), modes=(ADAGRAD,), combos=((True, True),),
                     routes=(None, "bucket", "presorted"))


def update_wpf(lib, dev):
    """DCTR_PLAN_WIDE_PER_FIELD: wide field f's gradient in column f of a g_wide row, the dense half's in column n_wide"""
    for ld_gw in (1, 3):
        c = EmbedCase(lib, dev, geometry_units(8), 70, wpf=True, ld_gw=ld_gw, n_wdense=2, seed=ld_gw)
        c.fwd()
        c.save()
        for opt in (SGD, ADAGRAD, ACCUM):
            c.restore()
            c.update(opt=opt, g_wdense=True)


def update_routes(lib, dev, dim, B):
    """every route through the update gives the bits of the first, and each matches ref"""
    units = [(max(B // 3, 40), dim, True), (25, dim, True)]          # (B = 16 384: 655 entries per id of the second unit)
    c = EmbedCase(lib, dev, units, B, interleaved=(dim == 5), seed=B + dim)
    c.fwd()
    c.save()
    for opt in (SGD, ADAGRAD, ACCUM):
        first = None
        for ws, parts, seg_parts in ((None, True, True), (None, False, True), ("bucket", True, True), ("bucket", False, True),
                                     ("presorted", True, True), ("presorted", False, True), ("presorted", True, False)):
            c.restore()
            c.update(opt=opt, ws=ws, parts=parts, segments_parts=seg_parts, reuse=first is not None)
            bits = c.table_bits()
            if first is None:
                first = bits
            same_bits(first, bits, "%s dim %d B=%d: ws=%s parts_t=%s (segments: %s) against no workspace" % (
                OPT_NAME[opt], dim, B, ws, parts, seg_parts))


def update_skew(lib, dev, dim, name):
    """partitions past kCap / kBucket = 512 entries: the split by id bits and the hot-id streaming path"""
    vocab = 700
    B = int(name) if name.isdigit() else 600
    units = [(1 if name == "hot" else vocab, dim, True)]
    P = EmbedCase(lib, dev, units, B).P
    assert 1 + 2 * P < vocab
    if name == "hot":          # (vocab 1)                    # one id: the streaming path, ragged last tile
        ids = None
    elif name == "split-split-hot":      # id / P = 0 (520 entries), 1 (40), 2 (40): split, split again, then streaming
        ids = {0: list(np.random.RandomState(5).permutation([1] * 520 + [1 + P] * 40 + [1 + 2 * P] * 40))}
    else:                                # two ids that differ in bit 0 of id / P, every entry of the batch
        ids = {0: [1 + P * (i % 2) for i in range(B)]}
    c = EmbedCase(lib, dev, units, B, ids=ids, seed=B + dim)
    assert c.P == P
    update_sweep(c, routes=(None, "presorted", "bucket"), combos=((True, True),))


def update_dense_half(lib, dev, n_wdense):
    """g_wdense alone, and with an SGD and an Adagrad wdense_step, through both kernels"""
    for B in (1, 300):
        c = EmbedCase(lib, dev, geometry_units(8), B, n_wdense=n_wdense, n_dense=2, ld_gw=3, seed=B + n_wdense)
        c.fwd()
        c.save()
        for wd in (None, SGD, ADAGRAD):
            first = None
            for ws in (None, "presorted"):
                c.restore()
                c.update(opt=ADAGRAD, g_wdense=True, wd_step=wd, ws=ws, reuse=first is not None)
                bits = c.table_bits()
                first = first or bits
                same_bits(first, bits, "dense half B=%d wd_step=%s: presorted against the scanning kernel" % (B, wd))


def atomic_fallback(lib, dev, dim):
    """dctr_embed_bwd (ACCUM, SGD) + dctr_embed_apply (SGD, Adagrad); after the apply gacc is exactly zero"""
    units = geometry_units(dim) if dim != "mixed" else MIXED
    for B in (1, 65, 300):
        c = EmbedCase(lib, dev, units, B, interleaved=(B == 65), seed=B)
        c.fwd()
        c.save()
        c.bwd(1)
        for opt in (SGD, ADAGRAD):
            c.restore()
            c.bwd(0)
            c.apply(opt)
        c.restore()
        c.bwd(0, g_fm=False)
        c.bwd(0, g_fm=False)          # adds onto a non-zero gacc


def refusals(lib, dev):
    """every argument check that returns before a launch: its documented code, and nothing written"""
    L = None
    for dim in (8, 5):
        c = EmbedCase(lib, dev, geometry_units(dim), 9, n_wdense=1, seed=dim)
        L = c.L
        c.fwd()
        c.save()
        before = c.snapshot()

        def expect(want, what, rc):
            assert rc == want, "%s: code %d, expected %d" % (what, rc, want)
            fa, ia = c.snapshot()
            assert np.array_equal(_bits(fa), _bits(before[0])) and np.array_equal(ia, before[1]), "%s wrote something" % what

        bad_plan = lambda **kw: _plan_with(c, **kw)          # noqa: E731
        no_gacc = bad_plan(flags=L.PLAN_HAS_STATE)
        no_state = bad_plan(flags=L.PLAN_HAS_GACC)
        too_wide = bad_plan(max_dim=64 * c.vec + 1)
        bad_vec = bad_plan(vec=3)
        # dctr_embed_update
        U = c.raw_update
        expect(EINVAL, "update opt = DCTR_UPD_LAZY", U(opt=LAZY))
        expect(EINVAL, "update opt = 7", U(opt=7))
        expect(EINVAL, "update presorted = 1, workspace one int short",
               U(ws="presorted", workspace_ints=c.n_units * c.P * (1 + KBUCKET) - 1))
        expect(EINVAL, "update presorted = 1 without a workspace", U(presorted=1))
        expect(EINVAL, "update ACCUM without DCTR_PLAN_HAS_GACC", U(opt=ACCUM, plan=ctypes.byref(no_gacc)))
        expect(EINVAL, "update Adagrad without DCTR_PLAN_HAS_STATE", U(opt=ADAGRAD, plan=ctypes.byref(no_state)))
        expect(ENOSUP, "update max_dim = 64 vec + 1", U(plan=ctypes.byref(too_wide)))
        expect(ENOSUP, "update vec = 3", U(plan=ctypes.byref(bad_vec)))
        expect(ENOSUP, "update B > 2^20", U(B=(1 << 20) + 1))
        expect(ENOSUP, "update max_vocab = 2^31", U(max_vocab=1 << 31))
        expect(EINVAL, "update plan = NULL", U(plan=None))
        expect(EINVAL, "update units = NULL", U(units=None))
        expect(EINVAL, "update ids_t = NULL", U(ids_t=None))
        expect(EINVAL, "update n_units = 0", U(n_units=0))
        expect(EINVAL, "update B = -1", U(B=-1))
        expect(EINVAL, "update ld_gw = 0", U(ld_gw=0))
        expect(EINVAL, "update g_fm without fm_s", U(fm_s=None))
        expect(EINVAL, "update g_wdense without X", U(g_wdense=True, X=None))
        expect(EINVAL, "update g_wdense without g_wide", U(g_wdense=True, g_wide=False))
        expect(0, "update B = 0", U(B=0))
        if c.vec == 4:
            expect(EALIGN, "update g_out off by one float", U(g_out=ctypes.c_void_p(c.rptr("g_out").value + 4)))
            expect(EALIGN, "update ld_g = ld + 1", U(ld_g=c.ld_out + 1))
            expect(EALIGN, "update fm_s off by one float", U(fm_s=ctypes.c_void_p(c.rptr("fm_s").value + 4)))
            expect(EALIGN, "update ld_s = ld + 1", U(ld_s=c.ld_s + 1))
        # dctr_embed_segments
        S = c.raw_segments
        expect(EINVAL, "segments workspace = NULL", S(workspace=None))
        expect(EINVAL, "segments workspace one int short", S(workspace_ints=c.n_units * c.P * (1 + KBUCKET) - 1))
        expect(EINVAL, "segments plan = NULL", S(plan=None))
        expect(EINVAL, "segments ids_t = NULL", S(ids_t=None))
        expect(ENOSUP, "segments max_dim = 64 vec + 1", S(plan=ctypes.byref(too_wide)))
        expect(0, "segments B = 0", S(B=0))
        # dctr_embed_ids
        I = c.raw_ids
        expect(EINVAL, "ids parts_t without a plan", I(plan=False))
        expect(EINVAL, "ids units = NULL", I(units=None))
        expect(EINVAL, "ids X = NULL", I(X=None))
        expect(EINVAL, "ids ids_t = NULL", I(ids_t=None))
        expect(EINVAL, "ids n_units = 0", I(n_units=0))
        expect(EINVAL, "ids B = -1", I(B=-1))
        expect(0, "ids B = 0", I(B=0))
        # dctr_embed_fwd
        F = c.raw_fwd
        expect(EINVAL, "fwd plan = NULL", F(plan=None))
        expect(EINVAL, "fwd X = NULL", F(X=None))
        expect(EINVAL, "fwd B = -1", F(B=-1))
        expect(EINVAL, "fwd ldx < n_xcols", F(ldx=c.n_xcols - 1))
        expect(EINVAL, "fwd vec = 3", F(plan=ctypes.byref(bad_vec)))
        expect(ENOSUP, "fwd max_dim = 64 vec + 1", F(plan=ctypes.byref(too_wide)))
        expect(EINVAL, "fwd ld_wide = 0", F(ld_wide=0))
        expect(EINVAL, "fwd fm without out", F(out=False, fm_s=False))
        expect(EINVAL, "fwd fm_s without out", F(out=False, fm=False))
        expect(EINVAL, "fwd fm_s with ld_s < emb_dim", F(ld_s=c.emb_dim - 1))
        expect(EINVAL, "fwd ids_t without units", F(units=None))
        expect(EINVAL, "fwd parts_t without ids_t", F(ids_t=None))
        expect(EINVAL, "fwd per-field wide with ld_wide < n_wide + 1",
               F(plan=ctypes.byref(bad_plan(flags=c.plan.flags | L.PLAN_WIDE_PER_FIELD)), ld_wide=c.n_wide))
        expect(0, "fwd B = 0", F(B=0))
        if c.vec == 4:
            expect(EALIGN, "fwd out off by one float", F(out=ctypes.c_void_p(c.rptr("out").value + 4)))
            expect(EALIGN, "fwd ld_out = ld + 1", F(ld_out=c.ld_out + 1))
            expect(EALIGN, "fwd fm_s off by one float", F(fm_s=ctypes.c_void_p(c.rptr("fm_s").value + 4)))
            expect(EALIGN, "fwd ld_s = ld + 1", F(ld_s=c.ld_s + 1))
        # dctr_embed_bwd / dctr_embed_apply
        Bw, Ap = c.raw_bwd, c.raw_apply
        expect(EINVAL, "bwd mode = 2", Bw(mode=2))
        expect(EINVAL, "bwd ACCUM without DCTR_PLAN_HAS_GACC", Bw(mode=0, plan=ctypes.byref(no_gacc)))
        expect(EINVAL, "bwd g_fm without out", Bw(out=None))
        expect(EINVAL, "bwd X = NULL", Bw(X=None))
        expect(ENOSUP, "bwd max_dim = 64 vec + 1", Bw(plan=ctypes.byref(too_wide)))
        expect(ENOSUP, "bwd SGD with max pooling", Bw(mode=1, plan=ctypes.byref(bad_plan(flags=c.plan.flags | L.PLAN_HAS_MAXPOOL))))
        expect(0, "bwd B = 0", Bw(B=0))
        expect(EINVAL, "apply opt = 2", Ap(opt=2, lr=0.0))
        expect(EINVAL, "apply without DCTR_PLAN_HAS_GACC", Ap(plan=ctypes.byref(no_gacc)))
        expect(EINVAL, "apply Adagrad without DCTR_PLAN_HAS_STATE", Ap(opt=1, plan=ctypes.byref(no_state)))
        expect(EINVAL, "apply plan = NULL", Ap(plan=None))
        expect(0, "apply B = 0", Ap(B=0))
        if c.vec == 4:
            expect(EALIGN, "bwd g_out off by one float", Bw(g_out=ctypes.c_void_p(c.rptr("g_out").value + 4)))
            expect(EALIGN, "bwd ld_g = ld + 1", Bw(ld_g=c.ld_out + 1))


# ---- general units: pooled fields and shared tables, through the product's EmbeddingPlan ---------------------------------
TOL["out"] = OUT_TOL          # (the pooled slices of out: sum and mean pooling add; fixed and max-pooled slices are copies)


GBAND = 16          # elements of sentinel around every buffer of a GeneralCase (16 of any dtype keep 16-byte alignment)


class GeneralCase(object):
    """user, item, hist (sum, T positions, shares item's table, mask mode), tags (mean, 5 positions, a length column), mh
    (mean, 4, mask mode), kw (max, 3) on both sides of the model, structs from ``EmbeddingPlan.bind()``: the host arithmetic
    (kmagic / kshift, slots, den and amax offsets) is the product's, as shipped.  The tables, Adagrad state and gacc slabs are
    the plan's own tensors ("untouched rows keep their bits" without guard bands); X, out, g_out, fm_s, wide, g_wide are
    padded with sentinel columns, the workspace has exactly the advertised size with a band behind it.  Lengths are 0 (sum /
    mean only), 1 and maxlen in the first samples, random after them; with ``hot`` 85 % of hist's positions are id 5."""

    def __init__(self, lib, dev, dim, B, T=4, hot=False, seed=0):
        from deepctr_torch._hip import lib as L
        from deepctr_torch._hip import plan as PL
        from deepctr_torch.inputs import SparseFeat, VarLenSparseFeat, build_input_features, create_embedding_matrix
        self.L, self.lib, self.dev, self.B, self.dim = L, lib, torch.device(dev), B, dim
        self.stream = L.stream_handle(self.dev)
        rng = self.rng = np.random.RandomState(seed)
        sp = lambda name, v, emb=None: SparseFeat(name, v, embedding_dim=dim, embedding_name=emb)          # noqa: E731
        cols = [sp("user", 37), sp("item", 23), VarLenSparseFeat(sp("hist", 23, "item"), T, "sum"),
                VarLenSparseFeat(sp("tags", 11), 5, "mean", "tags_len"), VarLenSparseFeat(sp("mh", 13), 4, "mean"),
                VarLenSparseFeat(sp("kw", 9), 3, "max")]
        fi = self.fi = build_input_features(cols)
        self.deep_t = create_embedding_matrix(cols, 0.5, sparse=False, device=dev)
        self.wide_t = create_embedding_matrix(cols, 0.5, linear=True, sparse=False, device=dev)
        plan = self.plan = PL.EmbeddingPlan(fi, deep_columns=cols, deep_tables=self.deep_t, wide_columns=cols,
                                            wide_tables=self.wide_t)
        assert plan.gen is not None and plan.unit_path and not plan.simple_units
        self.params = plan.table_params
        gen = torch.Generator().manual_seed(seed)
        self.state = []
        for q in self.params:
            q.requires_grad_(False)
            q.copy_((torch.randn(q.shape, generator=gen) * 0.5).to(self.dev))
            self.state.append((torch.rand(q.shape, generator=gen) * 0.45 + 0.05).to(self.dev))
        plan.ensure_gacc()
        plan.set_state(dict(zip(self.params, self.state)))
        self.cplan = plan.bind(self.dev)
        self.P = int(lib.dctr_embed_update_partitions(self.cplan, B))
        self.ws_ints = int(lib.dctr_embed_update_workspace_ints(self.cplan, plan.n_grid_units, B))
        # ---- X ------------------------------------------------------------------------------------------------------------
        nx = plan.n_xcols
        X = np.zeros((B, nx), F32)
        X[:, fi["user"][0]] = rng.randint(0, 37, B)
        X[:, fi["item"][0]] = rng.randint(0, 23, B)
        for name, vocab, least in (("hist", 23, 0), ("tags", 11, 0), ("mh", 13, 0), ("kw", 9, 1)):
            lo, hi = fi[name]
            n = rng.randint(least, hi - lo + 1, B)
            n[:3] = [max(least, 0), 1, hi - lo][:B]          # lengths 0 (sum / mean only), 1 and maxlen
            seq = rng.randint(1, vocab, (B, hi - lo))
            if hot and name == "hist":
                seq = np.where(rng.rand(B, hi - lo) < 0.85, 5, seq)
                n[3:] = hi - lo
            if name == "kw" and B > 3:
                seq[3] = [2, 2, 1]          # two equal maxima: the first wins
                n[3] = 3
            X[:, lo:hi] = np.where(np.arange(hi - lo)[None, :] < n[:, None], seq, 0)
            if name == "tags":
                X[:, fi["tags_len"][0]] = n
        # ---- buffers: name -> (whole tensor, view of what the header addresses) ---------------------------------------------
        D4 = _round_up(dim, 4)
        self.ld_out, self.ld_s, self.ld_wide, self.ld_gw, self.ldx = plan.ld_out + 4, D4 + 4, 3, 3, nx + 3
        g = plan.gen
        self.buf = {}
        mk = self._mk
        mk("X", B, nx, self.ldx, X)
        mk("out", B, plan.width, self.ld_out)
        mk("g_out", B, plan.width, self.ld_out, rng.normal(0, 1, (B, plan.width)))
        mk("fm_s", B, dim, self.ld_s)
        mk("fm", 1, B, B)
        mk("g_fm", 1, B, B, rng.normal(0, 1, (1, B)))
        mk("wide", B, 1, self.ld_wide)
        mk("g_wide", B, 1, self.ld_gw, rng.normal(0, 1, (B, 1)))
        mk("den_t", max(g["n_den"], 1), B, B)
        mk("ids_t", plan.n_vcols, B, B, dtype=torch.int32, sent=ISENT)
        mk("parts_t", plan.n_vcols, B, B, dtype=torch.int16, sent=-777)
        mk("amax", B, max(g["ld_amax"], 1), max(g["ld_amax"], 1), dtype=torch.uint8, sent=0xEE)
        mk("err", 1, 1, 1, np.zeros((1, 1)), dtype=torch.int32, sent=ISENT)
        mk("ws", 1, self.ws_ints, self.ws_ints, np.zeros((1, self.ws_ints)), dtype=torch.int32, sent=ISENT)
        plan.point_step_buffers(self.buf["den_t"][1], self.buf["amax"][1])
        self.sync()

    def _mk(self, name, rows, cols, ld, init=None, dtype=torch.float32, sent=SENT):
        whole = torch.full((GBAND + rows * ld + GBAND,), sent, dtype=dtype)
        view = whole[GBAND:GBAND + rows * ld].view(rows, ld)[:, :cols]
        if init is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(dtype))
        whole = whole.to(self.dev)
        self.buf[name] = (whole, whole[GBAND:GBAND + rows * ld].view(rows, ld)[:, :cols])

    def ptr(self, name, on=True):
        return ctypes.c_void_p(self.buf[name][1].data_ptr()) if on else None

    def sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)

    def snapshot(self):
        self.sync()
        snap = dict((k, w.cpu().numpy().copy()) for k, (w, _) in self.buf.items())
        for i, (q, st) in enumerate(zip(self.params, self.state)):
            snap[("w", i)], snap[("s", i)] = q.detach().cpu().numpy().copy(), st.cpu().numpy().copy()
            snap[("g", i)] = self.plan.gacc_of(q).cpu().numpy().copy()
        return snap

    def view(self, snap, name):
        """the addressed part of a buffer in a snapshot"""
        whole, v = self.buf[name]
        rows, cols = v.shape
        ld = v.stride(0)
        return snap[name][GBAND:GBAND + rows * ld].reshape(rows, ld)[:, :cols]

    def save(self):
        self.sync()
        self._saved = ([w.clone() for w, _ in self.buf.values()], [q.detach().clone() for q in self.params],
                       [s.clone() for s in self.state], [self.plan.gacc_of(q).clone() for q in self.params])

    def restore(self):
        bufs, ws, ss, gs = self._saved
        for (w, _), b in zip(self.buf.values(), bufs):
            w.copy_(b)
        for q, st, w0, s0, g0 in zip(self.params, self.state, ws, ss, gs):
            q.copy_(w0)
            st.copy_(s0)
            self.plan.gacc_of(q).copy_(g0)
        self.sync()

    def pidx(self, param):
        return next(i for i, q in enumerate(self.params) if q is param)

    # ---- the header's pooling, in one dtype ------------------------------------------------------------------------------
    def field_rows(self, X, f):
        """(rows [B, len], valid [B, len], count [B]) of a field: ids truncate, an id outside the table means row 0; a sum /
        mean position is valid while t < length (length mode) or its id != 0 (mask mode); max: every position is an entry"""
        ids = np.trunc(X[:, f.col:f.col + f.len].astype(np.float64)).astype(np.int64)
        rows = np.where((ids < 0) | (ids >= f.vocab), 0, ids)
        if f.pool == 0:
            return rows, np.ones_like(rows, bool), np.ones(len(X))
        if f.len_col >= 0:
            n = np.trunc(X[:, f.len_col].astype(np.float64)).astype(np.int64)
            valid = np.arange(f.len)[None, :] < n[:, None]
            return rows, valid, n.astype(np.float64)
        valid = ids != 0
        return rows, valid, valid.sum(axis=1).astype(np.float64)

    def pooled(self, snap, f, dt):
        """(pooled [B, dim], argmax [B, dim] | None)"""
        rows, valid, cnt = self.field_rows(self.view(snap, "X"), f)
        e = snap[("w", self.pidx(f.param))][rows].astype(dt)          # [B, len, dim]
        if f.pool == 0:
            return e[:, 0], None
        if f.pool == 3:
            v = np.where(valid[:, :, None], e, -np.inf)
            return v.max(axis=1), v.argmax(axis=1)
        tot = np.zeros((len(rows), f.dim), dt)
        for t in range(f.len):
            tot += np.where(valid[:, t, None], e[:, t], dt(0))
        if f.pool == 2:
            tot = tot / (cnt.astype(dt) + dt(F32(1e-8)))[:, None]
        return tot, None

    # ---- dctr_embed_ids + dctr_embed_fwd -----------------------------------------------------------------------------------
    def fwd(self):
        plan, lib = self.plan, self.lib
        before = self.snapshot()
        rc = lib.dctr_embed_ids(self.cplan, plan.units_ptr(), plan.n_grid_units, self.ptr("X"), self.ldx, self.B,
                                self.ptr("ids_t"), self.ptr("parts_t"), self.stream)
        assert rc == 0, "dctr_embed_ids (general): code %d" % rc
        rc = lib.dctr_embed_fwd(self.cplan, self.ptr("X"), self.ldx, self.B, self.ptr("out"), self.ld_out, self.ptr("wide"),
                                self.ld_wide, self.ptr("fm"), self.ptr("err"), plan.units_ptr(), plan.n_grid_units, None, None,
                                self.ptr("fm_s"), self.ld_s, self.stream)
        assert rc == 0, "dctr_embed_fwd (general): code %d" % rc
        after = self.snapshot()
        tag = "embed_fwd general dim %d B=%d" % (self.dim, self.B)
        X = self.view(before, "X")
        want = dict((k, v.copy()) for k, v in before.items())
        g = plan.gen
        # (a) ids_t, parts_t, den_t, amax, err
        kP = dict((u, d["k"] * self.P) for u, d in enumerate(g["vunits"]))
        wi, wp, wd = self.view(want, "ids_t"), self.view(want, "parts_t"), self.view(want, "den_t")
        for c, sl in enumerate(g["slots"]):
            f = self._slot_field(sl)
            ids = np.trunc(X[:, sl["col"]].astype(np.float64)).astype(np.int64)
            wi[c] = ids
            rows = np.where((ids < 0) | (ids >= f.vocab), 0, ids)
            _, valid, cnt = self.field_rows(X, f)
            tags = (rows % kP[sl["vu0"]]).astype(np.uint16)
            if sl["pool"] in (1, 2):
                tags = np.where(valid[:, sl["t"]], tags, 0xFFFF).astype(np.uint16)
            wp[c] = tags.view(np.int16)
            if sl["pool"] == 2:
                wd[sl["den"]] = (cnt.astype(F32) + F32(1e-8))
        self.view(want, "err")[...] = 0
        wa = self.view(want, "amax")
        res = {}
        for dt in (np.float64, np.float32):
            S = np.zeros((self.B, self.dim), dt)
            Q = np.zeros_like(S)
            W = np.zeros((self.B, 1), dt)
            O = np.zeros((self.B, plan.width), dt)
            for i, f in enumerate(plan.deep):
                e, arg = self.pooled(before, f, dt)
                O[:, f.out_off:f.out_off + f.dim] = e
                S += e
                Q += e * e
                if arg is not None and dt is np.float64:
                    wa[:, g["am_deep"][i]:g["am_deep"][i] + f.dim] = arg
            for i, f in enumerate(plan.wide):
                e, arg = self.pooled(before, f, dt)
                W += e
                if arg is not None and dt is np.float64:
                    wa[:, g["am_wide"][i]] = arg[:, 0]
            for k, v in (("out", O), ("wide", W), ("fm", (dt(0.5) * (S * S - Q).sum(axis=1))[None, :]), ("fm_s", S)):
                res.setdefault(k, []).append(v)
        got_out = self.view(after, "out")
        for f in plan.deep:
            if f.pool in (0, 3):          # copies of table rows: bit for bit
                sl = slice(f.out_off, f.out_off + f.dim)
                assert np.array_equal(_bits(got_out[:, sl]), _bits(res["out"][1][:, sl])), \
                    "%s: out's slice of field %s is not the table row, bit for bit" % (tag, f.name)
        for k in ("out", "wide", "fm", "fm_s"):
            x = self.view(after, k)
            _record_into("fwd-pooled", k, x, res[k][0], [res[k][1]], tag)
            self.view(want, k)[...] = x
        for k in sorted(want, key=str):
            assert np.array_equal(_bits(after[k]) if after[k].dtype == np.float32 else after[k], _bits(want[k])
                                  if want[k].dtype == np.float32 else want[k]), \
                "%s: %s differs from the contract (an integer output, a pad column, a guard band, an input or a table)" % (tag, k)

    def _slot_field(self, sl):
        plan = self.plan
        col0 = sl["col"] - sl["t"]
        for f in plan.deep + plan.wide:
            if f.col == col0 and f.len == sl["len"] and f.pool == sl["pool"]:
                return f
        raise AssertionError("slot %r names no field" % (sl,))

    # ---- dctr_embed_update -------------------------------------------------------------------------------------------------
    def entry_grads(self, snap, dt, g_fm, fold_out=True):
        """{table index: (rows [n], G [n, dim])}: every valid (field, position, sample) entry in (field, position, sample)
        order; S is the caller's fm_s, a pooled field's value the caller's out, den and amax the forward's side outputs"""
        plan, g = self.plan, self.plan.gen
        X = self.view(snap, "X")
        gO, S = self.view(snap, "g_out").astype(dt), self.view(snap, "fm_s").astype(dt)
        out, gF = self.view(snap, "out").astype(dt), self.view(snap, "g_fm")[0].astype(dt)
        gW, am = self.view(snap, "g_wide").astype(dt), self.view(snap, "amax")
        per = {}
        for side, fields, offs in (("deep", plan.deep, g["am_deep"]), ("wide", plan.wide, g["am_wide"])):
            for i, f in enumerate(fields):
                rows, valid, cnt = self.field_rows(X, f)
                pi = self.pidx(f.param)
                if side == "deep":
                    h = gO[:, f.out_off:f.out_off + f.dim].copy()
                    if g_fm and f.pool != 0:
                        h += gF[:, None] * (S - out[:, f.out_off:f.out_off + f.dim])
                else:
                    h = gW.copy()
                den = (cnt.astype(F32) + F32(1e-8)).astype(dt)
                for t in range(f.len):
                    G = h.copy()
                    if side == "deep" and g_fm and f.pool == 0:
                        G += gF[:, None] * (S - snap[("w", pi)][rows[:, 0]].astype(dt))
                    if f.pool == 2:
                        G = G / den[:, None]
                    elif f.pool == 3:
                        G = np.where(am[:, offs[i]:offs[i] + f.dim] == t, G, dt(0))
                    keep = valid[:, t] if f.pool in (1, 2) else np.ones(len(X), bool)
                    ent = per.setdefault(pi, ([], []))
                    ent[0].append(rows[keep, t])
                    ent[1].append(G[keep])
        return dict((pi, (np.concatenate(r), np.concatenate(G))) for pi, (r, G) in per.items())

    def update(self, opt, g_fm=True, route=None, reuse=False):
        """dctr_embed_update on general units.  route: None (every workgroup scans), "bucket" (workspace, presorted = 0),
        "presorted" (dctr_embed_segments first)"""
        plan, lib = self.plan, self.lib
        tag = "embed_update general %s dim %d B=%d%s route=%s" % (OPT_NAME[opt], self.dim, self.B, " g_fm" if g_fm else "", route)
        before = self.snapshot()
        common = (self.cplan, plan.units_ptr(), plan.n_grid_units, plan.max_vocab, self.ptr("ids_t"), self.ptr("parts_t"), self.B)
        if route == "presorted":
            rc = lib.dctr_embed_segments(*(common + (self.ptr("ws"), self.ws_ints, self.stream)))
            assert rc == 0, "dctr_embed_segments (general): code %d" % rc
        rc = lib.dctr_embed_update(*(common + (
            self.ptr("g_out"), self.ld_out, self.ptr("out"), self.ld_out, self.ptr("fm_s", g_fm), self.ld_s, self.ptr("g_fm", g_fm),
            self.ptr("g_wide"), self.ld_gw, opt, LR[opt], EPS, self.ptr("X"), self.ldx, None, None, self.ptr("ws", bool(route)),
            self.ws_ints if route else 0, 1 if route == "presorted" else 0, self.stream)))
        assert rc == 0, "%s: code %d" % (tag, rc)
        after = self.snapshot()
        if not reuse:
            self._models = []
            for dt, rev in ((np.float64, False), (np.float32, False), (np.float32, True)):
                lr, eps = dt(F32(LR[opt])), dt(F32(EPS))
                new = {}
                for pi, (rows, G) in self.entry_grads(before, dt, g_fm).items():
                    uniq, acc = seg_sum(rows, G, rev)
                    w, st, ga = [before[(k, pi)].astype(dt) for k in ("w", "s", "g")]
                    if opt == SGD:
                        w[uniq] = w[uniq] - lr * acc
                        new[("w", pi)] = (w, uniq)
                    elif opt == ADAGRAD:
                        st[uniq] = st[uniq] + acc * acc
                        w[uniq] = w[uniq] - lr * (acc / (np.sqrt(st[uniq]) + eps))
                        new[("w", pi)], new[("s", pi)] = (w, uniq), (st, uniq)
                    else:
                        ga[uniq] = ga[uniq] + acc
                        new[("g", pi)] = (ga, uniq)
                self._models.append(new)
        ref, r32a, r32b = self._models
        name = {"w": "table", "s": "state", "g": "gacc"}
        for k in sorted(after, key=str):
            if k in ref:
                _record_into("update-general", name[k[0]], after[k], ref[k][0], [r32a[k][0], r32b[k][0]], "%s table %d" % (tag, k[1]))
                mask = np.ones(len(after[k]), bool)
                mask[ref[k][1]] = False
                assert np.array_equal(_bits(after[k][mask]), _bits(before[k][mask])), \
                    "%s: a row of table %d (%s) whose id is not in the batch changed" % (tag, k[1], name[k[0]])
            elif k == "ws":
                n = plan.n_grid_units * self.P
                assert not after[k][GBAND:GBAND + n].any(), "%s: the workspace's counters are not zero again" % tag
                assert np.all(after[k][:GBAND] == ISENT) and np.all(after[k][GBAND + self.ws_ints:] == ISENT), \
                    "%s: the band around the workspace was written" % tag
            else:
                a, b = (_bits(after[k]), _bits(before[k])) if after[k].dtype == np.float32 else (after[k], before[k])
                assert np.array_equal(a, b), "%s: %s changed (an input, a pad column, a guard band or another slab)" % (tag, k)

    def bits(self):
        snap = self.snapshot()
        return dict((k, _bits(v) if v.dtype == np.float32 else v) for k, v in snap.items() if isinstance(k, tuple))

    # ---- dctr_embed_bwd (ACCUM) + dctr_embed_apply ---------------------------------------------------------------------------
    def bwd_apply(self, opt, g_fm=True):
        plan, lib = self.plan, self.lib
        tag = "embed_bwd general dim %d B=%d" % (self.dim, self.B)
        before = self.snapshot()
        gw = torch.from_numpy(np.ascontiguousarray(self.view(before, "g_wide")[:, 0])).to(self.dev)          # (bwd: a plain [B])
        rc = lib.dctr_embed_bwd(self.cplan, self.ptr("X"), self.ldx, self.B, self.ptr("g_out"), self.ld_out, self.ptr("out"),
                                self.ld_out, self.ptr("g_fm", g_fm), ctypes.c_void_p(gw.data_ptr()), 0, 0.0, self.stream)
        assert rc == 0, "%s: code %d" % (tag, rc)
        mid = self.snapshot()
        models = []
        for dt in (np.float64, np.float32):
            new = {}
            for pi, (rows, G) in self.entry_grads(before, dt, g_fm).items():
                uniq, acc = seg_sum(rows, G, False)
                ga = before[("g", pi)].astype(dt)
                ga[uniq] = ga[uniq] + acc
                new[pi] = ga
            models.append(new)
        for pi in sorted(models[0]):
            _record_into("bwd-pooled", "gacc", mid[("g", pi)], models[0][pi], [models[1][pi]], "%s table %d" % (tag, pi))
        for k in mid:
            if not (isinstance(k, tuple) and k[0] == "g"):
                assert np.array_equal(mid[k], before[k]) or (mid[k].dtype == np.float32 and np.array_equal(_bits(mid[k]), _bits(before[k]))), \
                    "%s: %s changed" % (tag, k)
        rc = lib.dctr_embed_apply(self.cplan, self.ptr("X"), self.ldx, self.B, opt, LR[opt], EPS, self.stream)
        assert rc == 0, "dctr_embed_apply (general): code %d" % rc
        after = self.snapshot()
        tag = "embed_apply general %s dim %d B=%d" % (OPT_NAME[opt], self.dim, self.B)
        for pi in range(len(self.params)):
            assert not after[("g", pi)].any(), "%s table %d: gacc is not exactly zero after the apply" % (tag, pi)
            res = []
            for dt in (np.float64, np.float32):
                lr, eps = dt(F32(LR[opt])), dt(F32(EPS))
                w, st, G = mid[("w", pi)].astype(dt), mid[("s", pi)].astype(dt), mid[("g", pi)].astype(dt)
                if opt == ADAGRAD:
                    st = st + G * G
                    w = np.where(G != 0, w - lr * (G / (np.sqrt(st) + eps)), w)
                else:
                    w = w - lr * G
                res.append((w, st))
            _record_into("apply-pooled", "table", after[("w", pi)], res[0][0], [res[1][0]], "%s table %d" % (tag, pi))
            hit = (mid[("g", pi)] != 0)
            assert np.array_equal(_bits(after[("w", pi)][~hit]), _bits(mid[("w", pi)][~hit])), "%s table %d: an element without a gradient moved" % (tag, pi)
            if opt == ADAGRAD:
                _record_into("apply-pooled", "state", after[("s", pi)], res[0][1], [res[1][1]], "%s table %d" % (tag, pi))
            else:
                assert np.array_equal(_bits(after[("s", pi)]), _bits(mid[("s", pi)])), "%s table %d: SGD wrote the state" % (tag, pi)


def _record_into(entry, tensor, x, r, r32s, tag):
    """(d) for the general cases: the same rule as EmbedCase._record"""
    assert np.all(np.isfinite(x)), "%s %s: not finite" % (tag, tensor)
    top = float(np.abs(r).max()) if r.size else 0.0
    if top == 0.0:
        assert np.all(x == 0), "%s %s: nonzero where the reference is identically zero" % (tag, tensor)
        return
    err = float(np.abs(x.astype(np.float64) - r).max()) / top
    err32 = max(float(np.abs(q.astype(np.float64) - r).max()) for q in r32s) / top
    w = WORST.setdefault((entry, tensor), [0.0, 0.0])
    w[0], w[1] = max(w[0], err), max(w[1], err32)
    assert err <= tol(entry, tensor), "%s %s: max|d| / max|ref| %.3e (max|ref| %.3g), bound %.2e (plain float32: %.3e)" % (
        tag, tensor, err, top, tol(entry, tensor), err32)


def lookup_pooled(lib, dev, dim):
    for B in (1, 17, 65):
        GeneralCase(lib, dev, dim, B, seed=B + dim).fwd()


def update_general(lib, dev, dim, B, hot=False):
    """all three modes, with and without g_fm; no pre-pass, the in-line buckets (``k_bucket<true>``) and the tag-scan pre-pass
    give the same bits; ACCUM twice adds"""
    c = GeneralCase(lib, dev, dim, B, T=8 if hot else 4, hot=hot, seed=B + dim)
    c.fwd()
    c.save()
    for opt in (SGD, ADAGRAD, ACCUM):
        for g_fm in (True, False):
            first = None
            for route in (None, "bucket", "presorted"):
                c.restore()
                c.update(opt, g_fm=g_fm, route=route, reuse=first is not None)
                bits = c.bits()
                first = first or bits
                same_bits(first, bits, "general %s B=%d g_fm=%s: route %s against no pre-pass" % (OPT_NAME[opt], B, g_fm, route))
    c.restore()
    c.update(ACCUM)
    c.update(ACCUM)          # (the model starts from the arena as it stands: the second launch must add)


def update_general_long_history(lib, dev):
    """a history of 126 positions over the item table: 127 slots x B = 520 is more than 65 536 entries of one unit, where
    dctr_embed_segments leaves the tag scan for ``k_bucket<true>`` + ``k_embed_segments<true, true>``"""
    c = GeneralCase(lib, dev, 4, 520, T=126, seed=9)
    assert c.plan.gen["max_unit_slots"] * c.B > 65536
    c.fwd()
    c.save()
    first = None
    for route in (None, "presorted"):
        c.restore()
        c.update(ADAGRAD, route=route, reuse=first is not None)
        bits = c.bits()
        first = first or bits
        same_bits(first, bits, "general long history: the bucket pre-pass against no pre-pass")


def atomic_fallback_pooled(lib, dev, dim):
    for B in (1, 65, 300):
        c = GeneralCase(lib, dev, dim, B, seed=B)
        c.fwd()
        c.save()
        for opt in (SGD, ADAGRAD):
            c.restore()
            c.bwd_apply(opt)


def _plan_with(c, **kw):
    """a copy of the case's plan with some scalars replaced (kept alive on the case)"""
    p = c.L.Plan.from_buffer_copy(c.plan)
    for k, v in kw.items():
        setattr(p, k, v)
    c._plans = getattr(c, "_plans", []) + [p]
    return p


def case_list():
    """[(id, fn(lib, dev))]: every case of tests/test_gpu_embed_abi.py; tests/test_embed_abi_host.py runs the same list"""
    out = []
    lay = (("contiguous", False), ("interleaved", True))
    for d in LOOKUP_DIMS:
        for lname, inter in lay:
            out.append(("lookup-vec%d-dim%d-%s" % (vec_of(d), d, lname), lambda lib, dev, d=d, i=inter: lookup_grid(lib, dev, d, i)))
    out.append(("lookup-mixed-dims", lambda lib, dev: lookup_shape(lib, dev, MIXED, n_dense=2)))
    out.append(("lookup-mixed-dims-interleaved", lambda lib, dev: lookup_shape(lib, dev, MIXED, n_dense=2, interleaved=True)))
    for n in (1, 4, 5, 32, 33):
        out.append(("lookup-deep-fields-%d" % n, lambda lib, dev, n=n: lookup_shape(lib, dev, [(9, 4, False)] * n)))
    for n, d in ((0, 4), (1, 4), (8, 4), (9, 4), (16, 8), (17, 8)):
        units = [(9, d, False)] + [(9, 0, True)] * n
        out.append(("lookup-wide-fields-%d-dim%d" % (n, d), lambda lib, dev, u=units: lookup_shape(lib, dev, u, n_wdense=1)))
    for n in (0, 4, 5, 13):
        out.append(("lookup-dense-%d" % n, lambda lib, dev, n=n: lookup_shape(lib, dev, geometry_units(4), n_dense=n)))
    out.append(("lookup-dense-off-minus-1", lambda lib, dev: lookup_shape(lib, dev, geometry_units(4), n_dense=4, dense_off=False)))
    for n in (0, 1, 5):
        for ww in (True, False):
            out.append(("lookup-wdense-%d-%s" % (n, "w" if ww else "no-w"),
                        lambda lib, dev, n=n, ww=ww: lookup_shape(lib, dev, geometry_units(4), n_wdense=n, wdense_w=ww)))
    out.append(("lookup-outputs", lookup_outputs))
    for lname, inter in lay:
        out.append(("lookup-ids-%s" % lname, lambda lib, dev, i=inter: lookup_ids(lib, dev, i)))
    for d in UPDATE_DIMS:
        for lname, inter in lay:
            out.append(("update-geometry-dim%d-%s" % (d, lname),
                        lambda lib, dev, d=d, i=inter: update_geometry(lib, dev, geometry_units(d), d, vec_of(d), i)))
    for lname, inter in lay:
        out.append(("update-geometry-mixed-%s" % lname, lambda lib, dev, i=inter: update_geometry(lib, dev, MIXED, 20, 4, i, False)))
        out.append(("update-geometry-wide-only-%s" % lname,
                    lambda lib, dev, i=inter: update_geometry(lib, dev, [(50, 0, True), (7, 0, True)], 1, 1, i)))
        out.append(("update-geometry-deep-only-%s" % lname,
                    lambda lib, dev, i=inter: update_geometry(lib, dev, [(50, 16, False), (7, 16, False)], 16, 4, i)))
    for name, units, d, v, common in FORCED_PAIRS:
        for lname, inter in lay:
            out.append(("update-geometry-%s-%s" % (name, lname),
                        lambda lib, dev, u=units, d=d, v=v, c=common, i=inter: update_geometry(lib, dev, u, d, v, i, c)))
    for d in (16, 5, 256):
        out.append(("update-p-change-dim%d" % d, lambda lib, dev, d=d: p_change(lib, dev, d)))
    out.append(("update-wide-per-field", update_wpf))
    for d in (16, 5):
        for B in (300, 16384):
            out.append(("update-routes-dim%d-B%d" % (d, B), lambda lib, dev, d=d, B=B: update_routes(lib, dev, d, B)))
    for d in (16, 256):
        for name in ("hot", "split", "split-split-hot", "512", "513"):
            out.append(("update-skew-dim%d-%s" % (d, name), lambda lib, dev, d=d, n=name: update_skew(lib, dev, d, n)))
    for n in (1, 3):
        out.append(("update-dense-half-%d" % n, lambda lib, dev, n=n: update_dense_half(lib, dev, n)))
    for d in (16, 5, 20, "mixed"):
        out.append(("atomic-fallback-%s" % (("dim%d" % d) if d != "mixed" else d), lambda lib, dev, d=d: atomic_fallback(lib, dev, d)))
    for d in (4, 16):
        out.append(("lookup-pooled-dim%d" % d, lambda lib, dev, d=d: lookup_pooled(lib, dev, d)))
        for B in (17, 300):
            out.append(("update-general-dim%d-B%d" % (d, B), lambda lib, dev, d=d, B=B: update_general(lib, dev, d, B)))
        out.append(("update-general-dim%d-hot" % d, lambda lib, dev, d=d: update_general(lib, dev, d, 300, hot=True)))
    out.append(("update-general-long-history", update_general_long_history))
    out.append(("atomic-fallback-pooled", lambda lib, dev: atomic_fallback_pooled(lib, dev, 4)))
    out.append(("refusals", refusals))
    return out
