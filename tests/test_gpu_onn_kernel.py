"""GPU: ONN's pair lookup through the C ABI (csrc/pair_embed.hip: dctr_pair_embed_fwd / _bwd).

Forward ``out`` and backward ``g_rows`` are ONE fp32 multiply per element, so they are compared BIT FOR BIT with
``numpy.float32`` products of the same rows -- no tolerance.  ``wide`` is compared bit for bit with ``dctr_embed_fwd``'s own
``wide`` for the same plan (the two kernels share that device code).  Then the row gradients go through
``dctr_embed_update`` (SGD and Adagrad, pre-sorted by ``dctr_embed_segments`` and not) against a numpy scatter-add of the
same fp32 ``g_rows`` in float64, within tests/test_gpu_update_general.py's bound for that comparison
(2e-5 x max(1, max|ref|)).

Shapes: the smallest at which the kernel can go wrong -- F = 2 (one pair) at B = 1 and 33; D = 6 (vec 2) and D = 5
(vec 1, idle lanes in every lane group); F = 5, D = 16, B = 257 (ragged against any samples-per-workgroup, more items than
one pass of the lane groups holds); F = 26 (325 pairs, 650 pair tables + 2 wide-only units), D = 16, B = 96."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENOSUP = -2


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Case(object):
    """A pair plan over freshly drawn tables + a batch.  ``vocabs``: per sparse feature; ``strided``: every pair table is a
    view of a wider slab (ld = 2 D + 4 > D); ``roomy``: every pair table is the first ``vocab`` rows of a 4x larger
    allocation (an unguarded out-of-range id then reads allocated memory); ``extra_wide``: sparse columns of the linear side
    only (wide-only units)."""

    def __init__(self, F, D, B, n_dense=2, vocabs=None, strided=False, roomy=False, extra_wide=0, seed=0):
        from deepctr_torch._hip.plan import EmbeddingPlan
        from deepctr_torch.inputs import DenseFeat, SparseFeat, build_input_features
        from deepctr_torch.models.basemodel import Linear
        torch.manual_seed(seed)
        rng = np.random.RandomState(seed)
        vocabs = list(vocabs) if vocabs is not None else [7 + 3 * i for i in range(F)]
        sparse = [SparseFeat("s%d" % i, vocabs[i], D) for i in range(F)]
        dense = [DenseFeat("d", n_dense)] if n_dense else []
        lin_cols = sparse + [SparseFeat("w%d" % i, 9 + i, D) for i in range(extra_wide)] + dense
        self.fi = fi = build_input_features(lin_cols)
        self.lin = Linear(lin_cols, fi, init_std=0.1, device=DEV).to(DEV)
        with torch.no_grad():
            for p in self.lin.parameters():
                p.normal_(0, 0.3)
        self.pairs = [(i, j) for i in range(F - 1) for j in range(i + 1, F)]
        self.keep, fields = [], []
        for (i, j) in self.pairs:
            for e, f in ((1, i), (2, j)):
                V = vocabs[f]
                if strided:
                    slab = torch.randn(V, 2 * D + 4, device=DEV) * 0.3
                    w = slab[:, :D]
                elif roomy:
                    slab = torch.randn(4 * V + 8, D, device=DEV) * 0.3
                    w = slab[:V]
                else:
                    slab = w = torch.randn(V, D, device=DEV) * 0.3
                self.keep.append(slab)
                fields.append(("s%d+s%d.emb%d" % (i, j, e), torch.nn.Parameter(w), fi["s%d" % f][0]))
        self.plan = EmbeddingPlan(fi, deep_columns=sparse + dense, deep_fields=fields, wide_columns=lin_cols,
                                  wide_tables=self.lin.embedding_dict, wide_dense_weight=getattr(self.lin, "weight", None),
                                  pair=True)
        self.F, self.D, self.B, self.P, self.n_dense = F, D, B, len(self.pairs), n_dense
        X = np.zeros((B, self.plan.n_xcols), np.float32)
        for c in lin_cols:
            lo, hi = fi[c.name]
            if isinstance(c, SparseFeat):
                X[:, lo] = rng.randint(0, c.vocabulary_size, B)
                X[:B // 4, lo] = X[0, lo]                      # duplicates
            else:
                X[:, lo:hi] = rng.rand(B, hi - lo)
        self.Xh = X
        self.X = torch.from_numpy(X).to(DEV)
        self.cplan = self.plan.bind(DEV)

    def tables(self):
        return [f.param.detach().cpu().numpy() for f in self.plan.deep]

    def ids(self, k, X=None):
        X = self.Xh if X is None else X
        f = self.plan.deep[k]
        ids = X[:, f.col].astype(np.int64)
        return np.where((ids < 0) | (ids >= f.vocab), 0, ids)

    def forward(self, X=None, wide=True):
        from deepctr_torch._hip import lib as L
        p = self.plan
        X = self.X if X is None else X
        B = X.shape[0]
        out = torch.full((B, p.ld_out), float("nan"), device=DEV)
        w = torch.full((B,), float("nan"), device=DEV) if (wide and p.has_wide) else None
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        rc = L.lib().dctr_pair_embed_fwd(self.cplan, _ptr(X), X.stride(0), B, _ptr(out), p.ld_out, _ptr(w), 1, _ptr(err),
                                         L.stream_handle(DEV))
        torch.cuda.synchronize()
        return rc, out.cpu().numpy(), (w.cpu().numpy() if w is not None else None), int(err.item())

    def expected_out(self, X=None):
        X = self.Xh if X is None else X
        T = self.tables()
        p = self.plan
        ref = np.zeros((X.shape[0], p.width), np.float32)
        for k in range(self.P):
            ref[:, k * self.D:(k + 1) * self.D] = T[2 * k][self.ids(2 * k, X)] * T[2 * k + 1][self.ids(2 * k + 1, X)]
        for j, col in enumerate(p.dense_cols):
            ref[:, p.dense_off + j] = X[:, col]
        return ref

    def embed_fwd_wide(self):
        """``wide`` of dctr_embed_fwd for the same plan (no deep output asked for)."""
        from deepctr_torch._hip import lib as L
        p = self.plan
        w = torch.empty((self.B,), device=DEV)
        L.check(L.lib().dctr_embed_fwd(self.cplan, _ptr(self.X), self.X.stride(0), self.B, None, p.ld_out, _ptr(w), 1, None,
                                       None, None, 0, None, None, None, 0, L.stream_handle(DEV)), "dctr_embed_fwd")
        torch.cuda.synchronize()
        return w.cpu().numpy()

    def backward(self, g_out):
        from deepctr_torch._hip import lib as L
        p = self.plan
        g_rows = torch.full((self.B, p.ld_rows), float("nan"), device=DEV)
        rc = L.lib().dctr_pair_embed_bwd(self.cplan, _ptr(self.X), self.X.stride(0), self.B, _ptr(g_out), g_out.stride(0),
                                         _ptr(g_rows), p.ld_rows, L.stream_handle(DEV))
        torch.cuda.synchronize()
        return rc, g_rows

    def expected_rows(self, g_out):
        T = self.tables()
        D = self.D
        ref = np.zeros((self.B, 2 * self.P * D), np.float32)
        for k in range(self.P):
            g = g_out[:, k * D:(k + 1) * D]
            o1, o2 = self.plan.deep[2 * k].out_off, self.plan.deep[2 * k + 1].out_off
            ref[:, o1:o1 + D] = g * T[2 * k + 1][self.ids(2 * k + 1)]
            ref[:, o2:o2 + D] = g * T[2 * k][self.ids(2 * k)]
        return ref

    def g_out(self, seed=1):
        g = torch.from_numpy(np.random.RandomState(seed).randn(self.B, self.plan.ld_out).astype(np.float32))
        return g.to(DEV), g.numpy()


def _check_both_directions(c):
    rc, out, wide, err = c.forward()
    assert rc == 0 and err == 0
    ref = c.expected_out()
    assert np.array_equal(out[:, :c.plan.width], ref), "out differs from the fp32 products"
    if wide is not None:
        assert np.array_equal(wide, c.embed_fwd_wide()), "wide differs from dctr_embed_fwd's"
    g_dev, g_host = c.g_out()
    rc, g_rows = c.backward(g_dev)
    assert rc == 0
    assert np.array_equal(g_rows.cpu().numpy()[:, :2 * c.P * c.D], c.expected_rows(g_host)), "g_rows differs"
    return g_rows


SHAPES = [(2, 4, 1), (2, 4, 33), (3, 6, 20), (3, 5, 20), (5, 16, 257), (26, 16, 96)]


@pytest.mark.parametrize("F,D,B", SHAPES, ids=["F%d-D%d-B%d" % s for s in SHAPES])
def test_products_and_row_gradients_bit_for_bit(F, D, B):
    c = Case(F, D, B, extra_wide=2 if F == 26 else 0)
    assert c.plan.vec == (4 if D % 4 == 0 else 2 if D % 2 == 0 else 1) and c.plan.simple_units
    if F == 26:
        assert len(c.plan.units) == 650 + 2
    _check_both_directions(c)


def test_vocab_one_table_every_id_a_duplicate():
    _check_both_directions(Case(5, 16, 257, vocabs=[9, 1, 14, 30, 5]))


def test_tables_as_strided_views():
    c = Case(5, 16, 257, strided=True)
    assert all(f.param.stride(0) == 36 for f in c.plan.deep)
    _check_both_directions(c)


@pytest.mark.parametrize("n_dense", [0, 1, 3])
def test_dense_tail(n_dense):
    c = Case(5, 16, 257, n_dense=n_dense)
    assert c.plan.width == 160 + n_dense and c.plan.ld_out == (160 if n_dense == 0 else 164)
    _check_both_directions(c)
    c = Case(3, 5, 20, n_dense=n_dense)           # vec 1: 15 + n_dense columns in rows of 16 / 16 / 20
    assert c.plan.width == 15 + n_dense and c.plan.ld_out == (16 if n_dense < 3 else 20)
    _check_both_directions(c)


def test_no_linear_side_and_no_pairs():
    from deepctr_torch._hip import lib as L
    c = Case(5, 16, 40)
    rc, out, wide, err = c.forward(wide=False)      # wide = NULL
    assert rc == 0 and np.array_equal(out[:, :c.plan.width], c.expected_out())
    one = Case(1, 4, 37, n_dense=3)                 # P = 0: the dense block and the logit only
    assert not one.plan.deep and one.plan.width == 3
    rc, out, wide, err = one.forward()
    assert rc == 0 and np.array_equal(out[:, :3], one.expected_out()) and np.array_equal(wide, one.embed_fwd_wide())
    g_dev, _ = one.g_out()
    assert one.backward(g_dev)[0] == 0
    assert L.lib().dctr_pair_embed_fwd(one.cplan, _ptr(one.X), one.X.stride(0), 0, None, 4, None, 1, None,
                                       L.stream_handle(DEV)) == 0           # B = 0


def test_out_of_range_id_reads_row_zero_and_raises_the_flag():
    c = Case(5, 16, 257, roomy=True)
    X = c.Xh.copy()
    b, feat = 130, 2
    col = c.fi["s%d" % feat][0]
    vocab = [f for f in c.plan.deep if f.col == col][0].vocab
    X[b, col] = vocab + 3                           # outside the table, inside its allocation
    rc, out, wide, err = c.forward(X=torch.from_numpy(X).to(DEV))
    assert rc == 0 and err & 1
    X0 = X.copy()
    X0[b, col] = 0
    ref = c.expected_out(X0)
    ref_dense = c.expected_out(X)                   # (the dense block is X's; ids() clamps the same way)
    assert np.array_equal(ref, ref_dense)
    assert np.array_equal(out[b, :c.plan.width], ref[b]), "the out-of-range id must read as row 0"
    rows = np.arange(c.B) != b
    assert np.array_equal(out[rows][:, :c.plan.width], c.expected_out()[rows]), "other samples must be unaffected"
    X[b, col] = -1
    rc, out, wide, err = c.forward(X=torch.from_numpy(X).to(DEV))
    assert rc == 0 and err & 1 and np.array_equal(out[b, :c.plan.width], ref[b])
    assert c.forward()[3] == 0


def _plain_plan(cols):
    from deepctr_torch._hip.plan import EmbeddingPlan
    from deepctr_torch.inputs import build_input_features, create_embedding_matrix
    fi = build_input_features(cols)
    deep = create_embedding_matrix(cols, 0.1, sparse=False, device=DEV)
    return EmbeddingPlan(fi, deep_columns=cols, deep_tables=deep)


def _both_refuse(plan, cplan=None):
    from deepctr_torch._hip import lib as L
    cplan = plan.bind(DEV) if cplan is None else cplan
    B = 8
    X = torch.zeros((B, plan.n_xcols), device=DEV)
    out = torch.zeros((B, 256), device=DEV)
    rows = torch.zeros((B, 256), device=DEV)
    s = L.stream_handle(DEV)
    assert L.lib().dctr_pair_embed_fwd(cplan, _ptr(X), X.stride(0), B, _ptr(out), 256, None, 1, None, s) == ENOSUP
    assert L.lib().dctr_pair_embed_bwd(cplan, _ptr(X), X.stride(0), B, _ptr(out), 256, _ptr(rows), 256, s) == ENOSUP
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0 and float(rows.abs().sum()) == 0          # nothing was launched


def test_refusals_return_enosup():
    from deepctr_torch._hip import lib as L
    from deepctr_torch._hip.plan import EmbeddingPlan
    from deepctr_torch.inputs import SparseFeat, VarLenSparseFeat
    _both_refuse(_plain_plan([SparseFeat("a", 5, 4), VarLenSparseFeat(SparseFeat("h", 6, 4), 3, "mean")]))   # pooled VarLen
    _both_refuse(_plain_plan([SparseFeat("a", 5, 4), SparseFeat("b", 6, 8)]))                                # mixed dims
    w = [torch.nn.Parameter(torch.randn(5, 4, device=DEV)) for _ in range(3)]
    _both_refuse(EmbeddingPlan({"a": (0, 1)}, deep_fields=[("x", w[0], 0), ("y", w[1], 0), ("z", w[2], 0)]))  # odd n_deep
    c = Case(3, 4, 8)
    c.cplan._obj.flags |= L.PLAN_WIDE_PER_FIELD
    _both_refuse(c.plan, c.cplan)
    c = Case(3, 4, 8)
    chunks = torch.zeros(4, dtype=torch.int64, device=DEV)
    c.cplan._obj.out_chunks, c.cplan._obj.chunk_rows = chunks.data_ptr(), 8
    _both_refuse(c.plan, c.cplan)


# ---- the row gradients through the sorted update ---------------------------------------------------------------------
@pytest.mark.parametrize("presorted", [0, 1], ids=["scan", "presorted"])
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("F,B", [(5, 257), (26, 96)], ids=["F5", "F26"])
def test_row_gradients_through_the_sorted_update(F, B, opt, presorted):
    from deepctr_torch._hip import lib as L
    lib = L.lib()
    c = Case(F, 16, B, extra_wide=2 if F == 26 else 0)
    p = c.plan
    params = p.table_params
    lr, eps = 0.05, 1e-10
    state = {}
    if opt == "adagrad":
        state = {id(q): torch.full_like(q.data, 0.05) for q in params}
        p.set_state({q: state[id(q)] for q in params})
    cplan = c.cplan = p.bind(DEV)
    assert p.update_kernel_ok(B), "the sorted update must take %d units" % len(p.units)
    before = {id(q): q.detach().cpu().numpy().astype(np.float64) for q in params}
    g_rows = _check_both_directions(c)
    g_wide = torch.from_numpy(np.random.RandomState(5).randn(B).astype(np.float32)).to(DEV)
    nu = p.n_grid_units
    s = L.stream_handle(DEV)
    ids_t = torch.empty((nu, B), dtype=torch.int32, device=DEV)
    parts_t = torch.empty((nu, B), dtype=torch.int16, device=DEV)
    L.check(lib.dctr_embed_ids(cplan, p.units_ptr(), nu, _ptr(c.X), c.X.stride(0), B, _ptr(ids_t), _ptr(parts_t), s), "ids")
    ws, n_ws = None, 0
    if presorted:
        n_ws = int(lib.dctr_embed_update_workspace_ints(cplan, nu, B))
        ws = torch.zeros(max(n_ws, 1), dtype=torch.int32, device=DEV)
        L.check(lib.dctr_embed_segments(cplan, p.units_ptr(), nu, p.max_vocab, _ptr(ids_t), _ptr(parts_t), B, _ptr(ws), n_ws,
                                        s), "segments")
    L.check(lib.dctr_embed_update(cplan, p.units_ptr(), nu, p.max_vocab, _ptr(ids_t), _ptr(parts_t), B, _ptr(g_rows),
                                  p.ld_rows, None, p.ld_out, None, 0, None, _ptr(g_wide), 1,
                                  L.UPD_SGD if opt == "sgd" else L.UPD_ADAGRAD, lr, eps, _ptr(c.X), c.X.stride(0), None, None,
                                  _ptr(ws), n_ws, presorted, s), "dctr_embed_update")
    torch.cuda.synchronize()
    R = g_rows.cpu().numpy().astype(np.float64)
    gw = g_wide.cpu().numpy().astype(np.float64)
    work = [(f, R[:, f.out_off:f.out_off + f.dim]) for f in p.deep] + [(f, gw[:, None]) for f in p.wide]
    for f, G in work:
        ids = c.Xh[:, f.col].astype(np.int64)
        acc = np.zeros((f.vocab, f.dim), np.float64)
        np.add.at(acc, ids, G)
        w0 = before[id(f.param)]
        if opt == "sgd":
            want = w0 - lr * acc
        else:
            st = 0.05 + acc * acc
            want = w0 - lr * acc / (np.sqrt(st) + eps)
            err = float(np.max(np.abs(state[id(f.param)].cpu().numpy() - st)))
            assert err <= 2e-5 * max(1.0, float(np.max(np.abs(st)))), "%s state: %.3e" % (f.name, err)
        err = float(np.max(np.abs(f.param.detach().cpu().numpy() - want)))
        assert err <= 2e-5 * max(1.0, float(np.max(np.abs(want)))), "%s: max|d|=%.3e" % (f.name, err)
