"""GPU: MLR's mixture kernels through the C ABI (csrc/mlr.hip: dctr_mlr_fwd / _bwd / _supported).

``y``, ``z``, ``g_wide`` and ``g_dense`` against a float64 numpy evaluation of the formulas include/dctr.h documents, on the
same inputs: 1e-5 on ``y`` and ``z``, 2e-5 x max|g_ref| on the gradients (no floor).  The same formulas are also evaluated
in float32 numpy; if that evaluation already deviates from float64 by more than a quarter of a bar, the case's bar becomes
4 x that deviation (each figure is printed before it is asserted).

Shapes: the smallest at which the kernel can go wrong.  The forward's tile is 16 samples, the backward's 64: B in {1, 15, 16,
17, 63, 64, 65, 257}.  R in {2, 3, 4, 8} with and without the bias head.  Fields per head 0 (dense-only heads), 1, 3 and 17
-- at R = 8 that is 137 fixed-length fields, more than the 128 one pass of the forward's workgroup (16 field slots x 8 loads
in flight) covers.  Dense columns per head 0, 1, 5, different for region and bias heads.  VarLen sum / mean (mask and length
mode) / max fields with empty sequences (not under max pooling: the reference turns an empty max-pooled sequence into -1e9,
which no float32 sum survives -- its own test data avoids them too), duplicate ids, both tasks."""
import ctypes

import numpy as np
import pytest
import torch

from mlr_helpers import mixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENOSUP = -2
Y_TOL, G_TOL = 1e-5, 2e-5


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _varlen(prefix):
    from deepctr_torch.inputs import SparseFeat, VarLenSparseFeat
    return [VarLenSparseFeat(SparseFeat(prefix + "vsum", 6, 4), 4, "sum"),
            VarLenSparseFeat(SparseFeat(prefix + "vmean", 7, 4), 5, "mean"),
            VarLenSparseFeat(SparseFeat(prefix + "vmax", 8, 4), 3, "max"),
            VarLenSparseFeat(SparseFeat(prefix + "vlen", 5, 4), 4, "mean", length_name=prefix + "vlen_length")]


class Case(object):
    """R region heads over ``n_sparse`` sparse + ``n_dense`` dense (+ VarLen) columns and an optional bias head over columns
    of its own (``bias = (n_sparse, n_dense, varlen)``; its dense feature is the region's when both have one: two heads then
    read the same X columns with different weights), freshly drawn N(0, 0.8) / N(0, 0.3) weights and a batch with duplicates."""

    def __init__(self, R, n_sparse, n_dense, B, bias=None, varlen=False, task="binary", seed=0):
        from deepctr_torch._hip.ops import MLRHeads
        from deepctr_torch._hip.plan import EmbeddingPlan
        from deepctr_torch.inputs import DenseFeat, SparseFeat, build_input_features
        from deepctr_torch.models.basemodel import Linear
        torch.manual_seed(seed)
        rng = np.random.RandomState(seed)
        region = [SparseFeat("s%d" % i, 5 + 2 * i, 4) for i in range(n_sparse)] + \
            ([DenseFeat("d", n_dense)] if n_dense else []) + (_varlen("r") if varlen else [])
        sides = [region] * R
        if bias is not None:
            bs, bd, bv = bias
            sides.append([SparseFeat("c%d" % i, 4 + 3 * i, 4) for i in range(bs)] +
                         ([DenseFeat("d" if bd == n_dense else "e", bd)] if bd else []) + (_varlen("b") if bv else []))
        self.fi = fi = build_input_features([c for side in sides for c in side])
        self.lins = [Linear(cols, fi, init_std=0.1, device=DEV).to(DEV) for cols in sides]
        with torch.no_grad():
            for h, lin in enumerate(self.lins):
                for p in lin.parameters():
                    p.normal_(0, 0.8 if h < R else 0.3)
        self.plan = EmbeddingPlan(fi, wide_sides=[(cols, lin.embedding_dict) for cols, lin in zip(sides, self.lins)],
                                  wide_per_field=True)
        self.heads = MLRHeads(self.plan, [getattr(lin, "weight", None) for lin in self.lins], R, bias is not None, task)
        self.R, self.H, self.B, self.binary = R, len(sides), B, task == "binary"
        X = np.zeros((B, self.plan.n_xcols), np.float32)
        seen = set()
        for c in [c for side in sides for c in side]:
            if c.name in seen:
                continue
            seen.add(c.name)
            lo, hi = fi[c.name]
            if isinstance(c, DenseFeat):
                X[:, lo:hi] = rng.rand(B, hi - lo)
            elif isinstance(c, SparseFeat):
                X[:, lo] = rng.randint(0, c.vocabulary_size, B)
                X[:B // 4, lo] = X[0, lo]                      # duplicates
            else:
                T = hi - lo
                lens = rng.randint(1 if c.combiner == "max" else 0, T + 1, B)
                ids = rng.randint(1, c.vocabulary_size, (B, T))
                ids[np.arange(T)[None, :] >= lens[:, None]] = 0
                X[:, lo:hi] = ids
                if c.length_name:
                    X[:, fi[c.length_name][0]] = lens
        self.Xh = X
        self.X = torch.from_numpy(X).to(DEV)
        self.cplan, self.cmlr = self.plan.bind(DEV), self.heads.bind(DEV)

    # ---- the library -------------------------------------------------------------------------------------------------
    def forward(self, X=None, ids=False):
        from deepctr_torch._hip import lib as L
        p = self.plan
        X = self.X if X is None else X
        B = X.shape[0]
        y = torch.full((B,), float("nan"), device=DEV)
        z = torch.full((B, self.H), float("nan"), device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        ids_t = torch.full((p.n_vcols, B), -7, dtype=torch.int32, device=DEV) if ids else None
        parts_t = torch.full((p.n_vcols, B), -7, dtype=torch.int16, device=DEV) if ids else None
        rc = L.lib().dctr_mlr_fwd(self.cplan, self.cmlr, _ptr(X), X.stride(0), B, _ptr(y), _ptr(z), z.stride(0), _ptr(err),
                                  _ptr(ids_t), _ptr(parts_t), p.units_ptr(), p.n_grid_units, L.stream_handle(DEV))
        torch.cuda.synchronize()
        return rc, y.cpu().numpy(), z.cpu().numpy(), int(err.item()), ids_t, parts_t

    def backward(self, g_y, z):
        from deepctr_torch._hip import lib as L
        p, B = self.plan, self.B
        nd = self.heads.n_dense
        g_wide = torch.full((B, p.ld_wide), float("nan"), device=DEV)
        g_dense = torch.full((max(nd, 1),), float("nan"), device=DEV)
        n = int(L.lib().dctr_mlr_bwd_workspace_floats(self.cmlr, B))
        assert n == (B + 63) // 64 * nd
        ws = torch.full((max(n, 1),), float("nan"), device=DEV)
        rc = L.lib().dctr_mlr_bwd(self.cplan, self.cmlr, _ptr(self.X), self.X.stride(0), B, _ptr(g_y), _ptr(z), z.stride(0),
                                  _ptr(g_wide), p.ld_wide, _ptr(g_dense), _ptr(ws), L.stream_handle(DEV))
        torch.cuda.synchronize()
        return rc, g_wide.cpu().numpy(), g_dense.cpu().numpy()[:nd]

    # ---- numpy ---------------------------------------------------------------------------------------------------------
    def field_values(self, dtype, X=None):
        """[B, n_wide]: every wide field's (pooled) first-order weight, ``dtype`` arithmetic; out-of-range ids read row 0"""
        X = self.Xh if X is None else X
        out = np.zeros((X.shape[0], len(self.plan.wide)), dtype)
        for f, fd in enumerate(self.plan.wide):
            w = fd.param.detach().cpu().numpy()[:, 0].astype(dtype)
            ids = X[:, fd.col:fd.col + fd.len].astype(np.int64)
            ids = np.where((ids < 0) | (ids >= fd.vocab), 0, ids)
            if fd.pool == 0:
                out[:, f] = w[ids[:, 0]]
                continue
            lens = X[:, fd.len_col].astype(np.int64) if fd.len_col >= 0 else None
            m = (np.arange(fd.len)[None, :] < lens[:, None]) if lens is not None else (ids != 0)
            rows = w[ids]
            if fd.pool == 3:
                out[:, f] = np.where(m, rows, rows - dtype(1e9)).max(axis=1)
            else:
                tot = (rows * m).sum(axis=1, dtype=dtype)
                if fd.pool == 2:
                    tot = tot / ((lens if lens is not None else m.sum(axis=1)).astype(dtype) + dtype(1e-8))
                out[:, f] = tot
        return out

    def logits(self, dtype, X=None):
        X = self.Xh if X is None else X
        V = self.field_values(dtype, X)
        Z = np.zeros((X.shape[0], self.H), dtype)
        for f, h in enumerate(self.plan.head_of):
            Z[:, h] += V[:, f]
        for h, cols in enumerate(self.heads.dense_cols):
            if cols:
                w = self.heads.weights[h].detach().cpu().numpy()[:, 0].astype(dtype)
                for j, col in enumerate(cols):
                    Z[:, h] += X[:, col].astype(dtype) * w[j]
        return Z

    def expected(self, g_y, dtype):
        """(y, z, g_wide [B, n_wide + 1], g_dense [n_dense]) in ``dtype``"""
        Z = self.logits(dtype)
        y, dz = mixture(Z, self.R, self.H > self.R, self.binary, dtype)
        gz = dz * g_y.astype(dtype)[:, None]
        nw = len(self.plan.wide)
        gw = np.zeros((self.B, nw + 1), dtype)
        gw[:, :nw] = gz[:, self.plan.head_of] if nw else 0
        gd = [np.sum(gz[:, h] * self.Xh[:, col].astype(dtype), dtype=dtype)
              for h, cols in enumerate(self.heads.dense_cols) for col in cols]
        return y, Z, gw, np.asarray(gd, dtype)


def _bar(name, base, ref64, ref32, scale=1.0):
    """the issue's rule: ``base x scale``, or 4 x the float32 formulas' own deviation when that exceeds a quarter of it"""
    bar = base * scale
    dev32 = float(np.max(np.abs(np.asarray(ref32, np.float64) - ref64))) if ref64.size else 0.0
    if dev32 > bar / 4:
        print("%s: float32 numpy deviates %.3e > bar / 4 = %.3e -> bar %.3e" % (name, dev32, bar / 4, 4 * dev32))
        bar = 4 * dev32
    return bar


def _check(name, got, ref64, ref32, base, scale=1.0):
    bar = _bar(name, base, ref64, ref32, scale)
    err = float(np.max(np.abs(got.astype(np.float64) - ref64))) if ref64.size else 0.0
    print("%s: max|d| = %.3e, bar %.3e" % (name, err, bar))
    assert np.all(np.isfinite(got))
    assert err <= bar, "%s: max|d| = %.3e > %.3e" % (name, err, bar)


CASES = {
    # name: (R, n_sparse, n_dense, B, bias (n_sparse, n_dense, varlen) | None, varlen, task)
    "r2_one_field_b1": (2, 1, 0, 1, None, False, "binary"),
    "r3_dense_only_bias_b15": (3, 3, 5, 15, (0, 1, False), False, "binary"),
    "r4_dense_only_regions_b16": (4, 0, 1, 16, (3, 0, False), False, "binary"),
    "r8_137_fields_b17": (8, 17, 1, 17, (1, 5, False), False, "binary"),
    "r3_bias_b63": (3, 3, 1, 63, (1, 0, False), False, "binary"),
    "r4_no_bias_b64": (4, 1, 5, 64, None, False, "binary"),
    "r2_regression_b65": (2, 3, 0, 65, (3, 1, False), False, "regression"),
    "r3_varlen_b257": (3, 3, 5, 257, (1, 1, True), True, "binary"),
    "r4_shared_dense_regression_b257": (4, 3, 1, 257, (1, 1, False), True, "regression"),
}


def _case(name, **kw):
    R, ns, nd, B, bias, varlen, task = CASES[name]
    return Case(R, ns, nd, B, bias=bias, varlen=varlen, task=task, **kw)


@pytest.mark.parametrize("name", list(CASES))
def test_parity_with_float64_and_run_to_run_bits(name):
    c = _case(name)
    assert c.heads.supported(DEV)
    rng = np.random.RandomState(1)
    g_y = rng.randn(c.B).astype(np.float32)
    y64, z64, gw64, gd64 = c.expected(g_y, np.float64)
    y32, z32, gw32, gd32 = c.expected(g_y, np.float32)
    rc, y, z, err, _, _ = c.forward()
    assert rc == 0 and err == 0
    _check("y", y, y64, y32, Y_TOL)
    _check("z", z, z64, z32, Y_TOL)
    zt, gt = torch.from_numpy(z).to(DEV), torch.from_numpy(g_y).to(DEV)
    rc, gw, gd = c.backward(gt, zt)
    assert rc == 0
    nw = len(c.plan.wide)
    if nw:
        _check("g_wide", gw[:, :nw + 1], gw64, gw32, G_TOL, float(np.max(np.abs(gw64))))
        assert not gw[:, nw].any()
    if gd64.size:
        _check("g_dense", gd, gd64, gd32, G_TOL, float(np.max(np.abs(gd64))))
    # a second run: identical bits for every output
    rc2, y2, z2, _, _, _ = c.forward()
    rc3, gw2, gd2 = c.backward(gt, zt)
    assert rc2 == 0 and rc3 == 0
    assert np.array_equal(y, y2) and np.array_equal(z, z2) and np.array_equal(gd, gd2)
    if nw:
        assert np.array_equal(gw[:, :nw + 1], gw2[:, :nw + 1])


@pytest.mark.parametrize("name", ["r3_varlen_b257", "r8_137_fields_b17"])
def test_rows_do_not_depend_on_the_batch(name):
    """rows computed alone (B = 1) equal the same rows inside the whole batch, bit for bit"""
    c = _case(name)
    _, y, z, _, _, _ = c.forward()
    for b in sorted(set(b for b in (0, 1, 15, 16, 64, c.B - 1) if b < c.B)):
        rc, y1, z1, _, _, _ = c.forward(c.X[b:b + 1].contiguous())
        assert rc == 0 and np.array_equal(y1[0], y[b]) and np.array_equal(z1[0], z[b]), b


def test_out_of_range_id_reads_row_zero_and_flags():
    c = _case("r3_dense_only_bias_b15")
    col = c.fi["s1"][0]
    X = c.Xh.copy()
    X[5, col], X[12, col] = 1000, -3
    rc, y, z, err, _, _ = c.forward(torch.from_numpy(X).to(DEV))
    assert rc == 0 and (err & 1)
    X[5, col] = X[12, col] = 0
    y64, _ = mixture(c.logits(np.float64, X), c.R, True, True)
    assert float(np.max(np.abs(y - y64))) <= Y_TOL
    rc, y0, z0, err0, _, _ = c.forward(torch.from_numpy(X).to(DEV))
    assert err0 == 0 and np.array_equal(y, y0) and np.array_equal(z, z0)


def test_side_outputs_for_the_update():
    """ids_t / parts_t as dctr_embed_ids writes them (a simple plan); a max pool's arg-max bytes where the gather puts them"""
    from deepctr_torch._hip import lib as L
    c = _case("r8_137_fields_b17")
    p = c.plan
    assert p.simple_units and p.gen is None
    rc, _, _, _, ids_t, parts_t = c.forward(ids=True)
    assert rc == 0
    ref_i = torch.empty_like(ids_t)
    ref_p = torch.empty_like(parts_t)
    L.check(L.lib().dctr_embed_ids(c.cplan, p.units_ptr(), p.n_grid_units, _ptr(c.X), c.X.stride(0), c.B, _ptr(ref_i),
                                   _ptr(ref_p), L.stream_handle(DEV)), "dctr_embed_ids")
    torch.cuda.synchronize()
    assert torch.equal(ids_t, ref_i) and torch.equal(parts_t, ref_p)

    c = _case("r3_varlen_b257")
    p = c.plan
    assert p.gen is not None and p.has_maxpool
    den_t, amax = p.step_buffers(c.B, DEV)
    amax.fill_(255)
    p.point_step_buffers(den_t, amax)
    rc, _, _, _, _, _ = c.forward()
    assert rc == 0
    A = amax.cpu().numpy()
    n = 0
    for f, fd in enumerate(p.wide):
        if fd.pool != 3:
            continue
        off = p.gen["am_wide"][f]
        w = fd.param.detach().cpu().numpy()[:, 0]
        ids = c.Xh[:, fd.col:fd.col + fd.len].astype(np.int64)
        v = np.where(ids != 0, w[ids], w[ids] - np.float32(1e9))
        assert np.array_equal(A[:, off], v.argmax(axis=1).astype(np.uint8)), f
        n += 1
    assert n == c.R + 1
    p.point_step_buffers(None, None)
    rc, _, _, _, ids_t, _ = c.forward(ids=True)          # a general unit spans several X columns: dctr_embed_ids
    assert rc == -1


def test_plan_with_a_deep_side_is_refused():
    from deepctr_torch._hip import lib as L
    from deepctr_torch._hip.plan import EmbeddingPlan
    from deepctr_torch.inputs import SparseFeat, create_embedding_matrix
    c = _case("r2_one_field_b1")
    cols = [SparseFeat("s0", 5, 4)]
    deep = create_embedding_matrix(cols, device=DEV)
    plan = EmbeddingPlan(c.fi, deep_columns=cols, deep_tables=deep, wide_sides=[(cols, lin.embedding_dict) for lin in c.lins],
                         wide_per_field=True)
    cplan = plan.bind(DEV)
    assert L.lib().dctr_mlr_supported(cplan, c.cmlr) == 0 and L.lib().dctr_mlr_supported(c.cplan, c.cmlr) == 1
    y, z = torch.zeros(1, device=DEV), torch.zeros(1, 2, device=DEV)
    s = L.stream_handle(DEV)
    assert L.lib().dctr_mlr_fwd(cplan, c.cmlr, _ptr(c.X), c.X.stride(0), 1, _ptr(y), _ptr(z), 2, None, None, None, None, 0,
                                s) == ENOSUP
    gw = torch.zeros(1, 3, device=DEV)
    assert L.lib().dctr_mlr_bwd(cplan, c.cmlr, _ptr(c.X), c.X.stride(0), 1, _ptr(y), _ptr(z), 2, _ptr(gw), 3, None, None,
                                s) == ENOSUP
    # without the per-field flag the update would read g_wide as one column: refused as well
    flat = EmbeddingPlan(c.fi, wide_sides=[(cols, lin.embedding_dict) for lin in c.lins])
    assert L.lib().dctr_mlr_supported(flat.bind(DEV), c.cmlr) == 0
    torch.cuda.synchronize()
