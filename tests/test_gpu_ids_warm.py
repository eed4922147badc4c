"""dctr_embed_ids (csrc/update.hip: k_embed_ids, k_embed_ids_gen) after it learnt to warm the memory-side cache.

The kernels turn X into ``ids_t`` / ``parts_t`` (/ ``den_t``) -- integers and exact counts, so every element must be EQUAL to
the numpy statement -- and, with a plan, issue loads of the table rows the next gather reads.  Those loads must leave no
trace: the tables keep their bits, the plan's error word stays clear (an id outside the vocabulary issues no load; the gather
reports it later), and the device is still healthy afterwards.

Checkers: ``ids_t`` is the id column cast to int32.  A simple unit's partition tag is what oracle/prepass_oracle.py
``segments_direct`` states: the clamped id (outside the vocabulary -> 0) modulo the plan's partition count; the test reads a
sample's tag and clamped id back out of that function's sorted keys.  A general unit (pooled fields) has k P partitions: the
tag is (id mod P) + P ((id div P) mod k) -- split_id of csrc/update_kernels.hpp restated -- and 0xFFFF for a position the
pooling masks out (sum / mean: id == 0, or t >= length where the field has a length column); mean pooling's divisor row is
the number of valid positions + 1e-8.

Batches: 1, 63, 64 (the workgroup's 16-sample tiles: one short, ragged, whole) and 4096."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = [1, 63, 64, 4096]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _plan(deep_cols, wide_cols):
    from deepctr_torch._hip.plan import EmbeddingPlan
    from deepctr_torch.inputs import build_input_features, create_embedding_matrix
    fi = build_input_features(list(deep_cols) + [c for c in wide_cols if c not in deep_cols])
    deep = create_embedding_matrix(deep_cols, 0.1, sparse=False, device=DEV)
    wide = create_embedding_matrix(wide_cols, 0.1, linear=True, sparse=False, device=DEV)
    return EmbeddingPlan(fi, deep_columns=deep_cols, deep_tables=deep, wide_columns=wide_cols, wide_tables=wide), fi


def _snapshot(plan):
    return [q.detach().clone() for q in plan.table_params]


def _assert_no_trace(plan, before):
    torch.cuda.synchronize()                                    # (raises if a launch faulted)
    for q, b in zip(plan.table_params, before):
        assert torch.equal(q.detach(), b), "a table changed under dctr_embed_ids"
    assert int(plan.err_flag(torch.device(DEV)).item()) == 0, "the plan's error word was touched"


def _simple_case(B, seed=3):
    """a (deep + wide, vocab 50) | b (deep + wide, vocab 1) | c (deep only, vocab 1000) | d (wide only, vocab 7) + one dense"""
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    a, b, c, d = SparseFeat("a", 50, 16), SparseFeat("b", 1, 16), SparseFeat("c", 1000, 16), SparseFeat("d", 7, 16)
    plan, fi = _plan([a, b, c, DenseFeat("x", 1)], [a, b, d])
    rng = np.random.RandomState(seed + B)
    X = np.zeros((B, plan.n_xcols), np.float32)
    for f in (a, b, c, d):
        X[:, fi[f.name][0]] = rng.randint(0, f.vocabulary_size, B)
    X[:, fi["x"][0]] = rng.rand(B)
    # ids outside the vocabulary in some samples, on both sides of it and on every kind of unit
    for k, (name, bad) in enumerate([("a", -1), ("a", 50), ("b", 1), ("c", 1000), ("c", -7), ("d", 7), ("d", 1 << 20)]):
        X[(5 * k + 2) % B, fi[name][0]] = bad
    return plan, X


@pytest.mark.parametrize("B", BATCHES)
def test_simple_units_equal_the_numpy_statement(B):
    from prepass_oracle import ceil_log2, segments_direct
    from deepctr_torch._hip import lib as L
    lib = L.lib()
    plan, Xh = _simple_case(B)
    kinds = set((di >= 0, wi >= 0) for di, wi, _, _ in plan.units)
    assert kinds == {(True, True), (True, False), (False, True)}, "the case must hold every kind of unit"
    dev = torch.device(DEV)
    cplan = plan.bind(dev)
    before = _snapshot(plan)
    X = torch.from_numpy(Xh).to(dev)
    nu = len(plan.units)
    P = int(lib.dctr_embed_update_partitions(cplan, B))
    assert P >= 1
    s = L.stream_handle(dev)
    ids_t = torch.full((nu, B), -12345, dtype=torch.int32, device=dev)
    parts_t = torch.full((nu, B), -1, dtype=torch.int16, device=dev)
    L.check(lib.dctr_embed_ids(cplan, plan.units_ptr(), nu, _p(X), X.stride(0), B, _p(ids_t), _p(parts_t), s), "ids")
    _assert_no_trace(plan, before)
    ids, parts = ids_t.cpu().numpy(), parts_t.cpu().numpy().view(np.uint16)
    bbits = ceil_log2(max(B, 2))
    for u, (di, wi, col, _) in enumerate(plan.units):
        vocab = plan.deep[di].vocab if di >= 0 else plan.wide[wi].vocab
        raw = Xh[:, col].astype(np.int32)
        assert np.array_equal(ids[u], raw), "ids_t of unit %d" % u
        counts, keys = segments_direct(raw.astype(np.int64), vocab, P, bucket=B + 1)
        want_part = np.full(B, -1, np.int64)
        want_id = np.full(B, -1, np.int64)
        for q in range(P):
            k = keys[q].astype(np.int64)
            assert len(k) == counts[q]
            smp = k & ((1 << bbits) - 1)
            want_part[smp] = q
            want_id[smp] = (k >> bbits) * P + q
        assert (want_part >= 0).all()
        assert np.array_equal(parts[u].astype(np.int64), want_part), "parts_t of unit %d" % u
        clamped = np.where((ids[u] < 0) | (ids[u] >= vocab), 0, ids[u])
        assert np.array_equal(clamped, want_id), "clamped ids of unit %d" % u
    # without a plan: ids only (nothing to warm, no tags)
    ids2 = torch.full((nu, B), -12345, dtype=torch.int32, device=dev)
    L.check(lib.dctr_embed_ids(None, plan.units_ptr(), nu, _p(X), X.stride(0), B, _p(ids2), None, s), "ids without a plan")
    _assert_no_trace(plan, before)
    assert torch.equal(ids2, ids_t)
    # with a plan and no tags
    ids3 = torch.full((nu, B), -12345, dtype=torch.int32, device=dev)
    L.check(lib.dctr_embed_ids(cplan, plan.units_ptr(), nu, _p(X), X.stride(0), B, _p(ids3), None, s), "ids without tags")
    _assert_no_trace(plan, before)
    assert torch.equal(ids3, ids_t)


def test_more_units_than_one_pass_and_long_rows():
    """70 units (the kernel takes 64 per pass) of dim 40: rows of 160 bytes, two or three 64-byte pieces each, most of them
    not aligned to a piece"""
    from deepctr_torch.inputs import SparseFeat
    from deepctr_torch._hip import lib as L
    lib = L.lib()
    cols = [SparseFeat("s%d" % i, 3 + 5 * i, 40) for i in range(70)]
    plan, fi = _plan(cols, cols[::3])
    B = 37
    rng = np.random.RandomState(9)
    Xh = np.zeros((B, plan.n_xcols), np.float32)
    for f in cols:
        Xh[:, fi[f.name][0]] = rng.randint(-1, f.vocabulary_size + 1, B)     # both ends one past the vocabulary
    dev = torch.device(DEV)
    cplan = plan.bind(dev)
    before = _snapshot(plan)
    X = torch.from_numpy(Xh).to(dev)
    nu = len(plan.units)
    assert nu == 70
    P = int(lib.dctr_embed_update_partitions(cplan, B))
    ids_t = torch.full((nu, B), -12345, dtype=torch.int32, device=dev)
    parts_t = torch.full((nu, B), -1, dtype=torch.int16, device=dev)
    L.check(lib.dctr_embed_ids(cplan, plan.units_ptr(), nu, _p(X), X.stride(0), B, _p(ids_t), _p(parts_t),
                               L.stream_handle(dev)), "ids")
    _assert_no_trace(plan, before)
    ids, parts = ids_t.cpu().numpy(), parts_t.cpu().numpy().view(np.uint16)
    for u, (di, wi, col, _) in enumerate(plan.units):
        vocab = plan.deep[di].vocab if di >= 0 else plan.wide[wi].vocab
        raw = Xh[:, col].astype(np.int32)
        assert np.array_equal(ids[u], raw), u
        assert np.array_equal(parts[u], np.where((raw < 0) | (raw >= vocab), 0, raw) % P), u


@pytest.mark.parametrize("B", BATCHES)
def test_general_units_equal_the_numpy_statement(B):
    from deepctr_torch.inputs import SparseFeat, VarLenSparseFeat
    from deepctr_torch._hip import lib as L
    lib = L.lib()
    a = SparseFeat("a", 30, 8)
    hm = VarLenSparseFeat(SparseFeat("hm", 40, 8), 5, "mean")                       # mask mode: id 0 is padding
    hl = VarLenSparseFeat(SparseFeat("hl", 1, 8), 4, "sum", length_name="hl_len")   # length mode, vocab 1
    hx = VarLenSparseFeat(SparseFeat("hx", 25, 8), 3, "max")
    hw = VarLenSparseFeat(SparseFeat("hw", 9, 8), 3, "mean", length_name="hw_len")  # wide only
    plan, fi = _plan([a, hm, hl, hx], [a, hm, hw])
    assert plan.gen is not None, "pooled fields make general units"
    rng = np.random.RandomState(17 + B)
    Xh = np.zeros((B, plan.n_xcols), np.float32)
    Xh[:, fi["a"][0]] = rng.randint(0, 30, B)
    for f in (hm, hl, hx, hw):
        lo, hi = fi[f.name]
        Xh[:, lo:lo + f.maxlen] = rng.randint(0, f.sparsefeat.vocabulary_size, (B, f.maxlen))
    Xh[:, fi["hl_len"][0]] = rng.randint(0, 5, B)
    Xh[:, fi["hw_len"][0]] = rng.randint(0, 4, B)
    for k, (name, off, bad) in enumerate([("a", 0, -1), ("a", 0, 30), ("hm", 2, 40), ("hm", 0, -3), ("hl", 1, 1),
                                          ("hx", 2, 25), ("hw", 0, 9)]):
        Xh[(7 * k + 3) % B, fi[name][0] + off] = bad
    dev = torch.device(DEV)
    cplan = plan.bind(dev)
    den_t, amax = plan.step_buffers(B, dev)
    assert den_t is not None
    den_t.fill_(float("nan"))
    plan.point_step_buffers(den_t, amax)
    before = _snapshot(plan)
    X = torch.from_numpy(Xh).to(dev)
    nv, nu = plan.n_vcols, plan.n_grid_units
    P = int(lib.dctr_embed_update_partitions(cplan, B))
    s = L.stream_handle(dev)
    ids_t = torch.full((nv, B), -12345, dtype=torch.int32, device=dev)
    parts_t = torch.full((nv, B), -2, dtype=torch.int16, device=dev)
    L.check(lib.dctr_embed_ids(cplan, plan.units_ptr(), nu, _p(X), X.stride(0), B, _p(ids_t), _p(parts_t), s), "ids")
    _assert_no_trace(plan, before)
    ids, parts = ids_t.cpu().numpy(), parts_t.cpu().numpy().view(np.uint16)
    den = den_t.cpu().numpy()
    g = plan.gen
    masked = 0
    for c, sl in enumerate(g["slots"]):
        vu = g["vunits"][sl["vu0"]]
        vocab, k = g["vocabs"][sl["vu0"]], vu["k"]
        raw = Xh[:, sl["col"]].astype(np.int32)
        assert np.array_equal(ids[c], raw), "ids_t of column %d" % c
        valid = np.ones(B, bool)
        if sl["pool"] in (1, 2):                                   # sum / mean
            valid = (sl["t"] < Xh[:, sl["len_col"]].astype(np.int32)) if sl["len_col"] >= 0 else (raw != 0)
        cl = np.where((raw < 0) | (raw >= vocab), 0, raw).astype(np.int64)
        tag = cl % P + P * ((cl // P) % k)
        want = np.where(valid, tag, 0xFFFF)
        masked += int((~valid).sum())
        assert np.array_equal(parts[c].astype(np.int64), want), "parts_t of column %d" % c
        if sl["den"] >= 0 and sl["t"] == 0:
            first = sl["col"]
            if sl["len_col"] >= 0:
                cnt = Xh[:, sl["len_col"]].astype(np.int32).astype(np.float32)
            else:
                cnt = (Xh[:, first:first + sl["len"]].astype(np.int32) != 0).sum(1).astype(np.float32)
            assert np.array_equal(den[sl["den"]], cnt + np.float32(1e-8)), "den_t row %d" % sl["den"]
    assert masked > 0 or B == 1, "the case must mask some positions out"
    assert np.isfinite(den).all()
