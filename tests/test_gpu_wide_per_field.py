"""GPU: the per-field-wide mode of the model plan on its own (DCTR_PLAN_WIDE_PER_FIELD: csrc/embed.hip, update_kernels.hpp).
Per-field first-order weights and the dense column against plain indexing of the tables (fixed fields, pooled sum / mean /
max, a shared table); one sgd and one adagrad update from a random per-field gradient against index_add_ on a dense copy
(tests/test_gpu_update.py's tolerance); a plan over the same columns WITHOUT the bit still returns the summed wide [B] and
takes a per-sample g_wide."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _columns(kind):
    from deepctr_torch.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    if kind == "fixed":
        return [SparseFeat("s%d" % i, v, 8) for i, v in enumerate((7, 50, 1000, 13, 5))] + \
               [DenseFeat("d0", 1), DenseFeat("d1", 2)]
    if kind == "many":           # more wide fields than the gather's first pass holds per lane group
        return [SparseFeat("s%d" % i, 11 + i, 16) for i in range(39)] + [DenseFeat("d0", 1)]
    return [SparseFeat("user", 11, 4), SparseFeat("item", 9, 4), DenseFeat("price", 1),
            VarLenSparseFeat(SparseFeat("hist_sum", 9, 4, embedding_name="item"), 4, "sum"),      # shares `item`
            VarLenSparseFeat(SparseFeat("tags_mean", 7, 4), 5, "mean"),
            VarLenSparseFeat(SparseFeat("kw_max", 8, 4), 3, "max"),
            VarLenSparseFeat(SparseFeat("seq", 6, 4), 4, "mean", length_name="seq_length")]


def _batch(cols, fi, B, seed):
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    rng = np.random.RandomState(seed)
    X = np.zeros((B, max(hi for _, hi in fi.values())), np.float32)
    for c in cols:
        lo, hi = fi[c.name]
        if isinstance(c, SparseFeat):
            X[:, lo] = rng.randint(0, c.vocabulary_size, B)
            X[:B // 4, lo] = X[0, lo]                      # duplicates
        elif isinstance(c, DenseFeat):
            X[:, lo:hi] = rng.rand(B, hi - lo)
        else:
            T = hi - lo
            lens = rng.randint(1 if c.combiner == "max" else 0, T + 1, B)
            ids = rng.randint(1, c.vocabulary_size, (B, T))
            ids[np.arange(T)[None, :] >= lens[:, None]] = 0
            X[:, lo:hi] = ids
            if c.length_name:
                X[:, fi[c.length_name][0]] = lens
    return torch.from_numpy(X).to(DEV)


def _setup(kind, per_field, seed=0):
    from deepctr_torch._hip.plan import EmbeddingPlan
    from deepctr_torch.inputs import build_input_features, create_embedding_matrix
    from deepctr_torch.models.basemodel import Linear
    torch.manual_seed(seed)
    cols = _columns(kind)
    fi = build_input_features(cols)
    deep = create_embedding_matrix(cols, 0.1, sparse=False, device=DEV)
    lin = Linear(cols, fi, init_std=0.1, device=DEV).to(DEV)
    with torch.no_grad():
        for p in list(deep.parameters()) + list(lin.parameters()):
            p.normal_(0, 0.3)
    plan = EmbeddingPlan(fi, deep_columns=cols, deep_tables=deep, wide_columns=cols, wide_tables=lin.embedding_dict,
                         wide_dense_weight=lin.weight, wide_per_field=per_field)
    return cols, fi, deep, lin, plan


def _pooled_wide(lin, fi, c, X):
    """[B] first-order value of one linear column by plain indexing (sequence.py:49-77 for VarLen)"""
    from deepctr_torch.inputs import SparseFeat
    w = lin.embedding_dict[c.embedding_name].weight
    lo, hi = fi[c.name]
    if isinstance(c, SparseFeat):
        return w[X[:, lo].long(), 0]
    ids = X[:, lo:hi].long()
    T = hi - lo
    mask = (torch.arange(T, device=X.device)[None, :] < X[:, fi[c.length_name][0]].long()[:, None]) if c.length_name \
        else (ids != 0)
    rows = w[ids][:, :, 0]
    mf = mask.float()
    if c.combiner == "max":
        return (rows - (1 - mf) * 1e9).max(dim=1).values
    tot = (rows * mf).sum(1)
    return tot / (mf.sum(1) + 1e-8) if c.combiner == "mean" else tot


def _wide_columns(cols):
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    fixed = [c for c in cols if isinstance(c, SparseFeat)]
    var = [c for c in cols if not isinstance(c, (SparseFeat, DenseFeat))]
    dense = [c for c in cols if isinstance(c, DenseFeat)]
    return fixed + var, dense


@pytest.mark.parametrize("kind,B", [("fixed", 300), ("fixed", 1), ("many", 4099), ("pooled", 333)])
def test_per_field_values(kind, B):
    from deepctr_torch._hip import lib as L
    from deepctr_torch._hip import ops
    cols, fi, deep, lin, plan = _setup(kind, True)
    X = _batch(cols, fi, B, 1)
    with torch.no_grad():
        out, wide, _ = ops.embed(plan, X, full=True)
    plan.bind(X.device)
    assert plan.cplan.flags & L.PLAN_WIDE_PER_FIELD and plan.ld_wide == len(plan.wide) + 1
    assert wide.shape == (B, len(plan.wide) + 1)
    sparse, dense = _wide_columns(cols)
    assert [c.name for c in sparse] == [f.name for f in plan.wide]
    for f, c in enumerate(sparse):
        ref = _pooled_wide(lin, fi, c, X)
        assert float((wide[:, f] - ref).detach().abs().max()) <= 1e-6, c.name
    dcols = torch.cat([X[:, fi[c.name][0]:fi[c.name][1]] for c in dense], 1)
    ref = (dcols.double() @ lin.weight.double()).squeeze(1)
    assert float((wide[:, -1].double() - ref).abs().max()) <= 1e-6
    # the same columns without the bit: the summed wide [B], as always
    cols2, fi2, deep2, lin2, plan2 = _setup(kind, False)
    with torch.no_grad():
        out2, wide2, _ = ops.embed(plan2, X, full=True)
    assert tuple(wide2.shape) == (B,) and torch.equal(out2[:, :plan2.width], out[:, :plan.width])   # (padding columns are not written)
    assert float((wide2.double() - wide.double().sum(1)).abs().max()) <= 1e-5 * max(1.0, float(wide2.abs().max()))


@pytest.mark.parametrize("kind,B", [("fixed", 300), ("many", 4099), ("pooled", 333)])
@pytest.mark.parametrize("mode", ["sgd", "adagrad"])
def test_per_field_update(kind, B, mode):
    """One update from random per-field gradients (and a random gradient on the deep rows) against autograd on plain
    indexing of dense copies + index_add_'s dense gradient."""
    from deepctr_torch._hip import ops
    cols, fi, deep, lin, plan = _setup(kind, True)
    X = _batch(cols, fi, B, 2)
    params = plan.table_params
    lr = 0.05
    opt = torch.optim.SGD(params, lr=lr) if mode == "sgd" else torch.optim.Adagrad(params, lr=lr)
    state = None
    if mode == "adagrad":
        for p in params:
            opt.state[p]["sum"] = torch.rand_like(p) * 0.1 + 0.01
        plan.set_state({p: opt.state[p]["sum"] for p in params})
        plan.update = ("adagrad", lr, 1e-10)
        state = {id(p): opt.state[p]["sum"].clone() for p in params}
    else:
        plan.update = ("sgd", lr)
    before = {id(p): p.detach().clone() for p in params}
    w_dense_before = lin.weight.detach().clone()
    out, wide, _ = ops.embed(plan, X, full=True)
    g = torch.Generator().manual_seed(5)
    R_out = torch.randn(out.shape, generator=g).to(DEV)
    R_wide = torch.randn(wide.shape, generator=g).to(DEV)
    ((out * R_out).sum() + (wide * R_wide).sum()).backward()
    torch.cuda.synchronize()
    assert plan.update_kernel_ok(B)
    # reference: dense gradients by autograd over plain indexing of copies
    sparse, dense = _wide_columns(cols)
    copies = {id(p): before[id(p)].clone().requires_grad_(True) for p in params}

    class _Lin(object):
        pass
    ref_lin = _Lin()
    ref_lin.embedding_dict = {k: type("T", (), {"weight": copies[id(v.weight)]})() for k, v in lin.embedding_dict.items()}
    loss = 0
    for f, c in enumerate(sparse):
        loss = loss + (_pooled_wide(ref_lin, fi, c, X) * R_wide[:, f]).sum()
    # deep side: only its fixed / pooled rows through the same helper on the deep tables, one column of D at a time
    for fd in plan.deep:
        c = [c for c in sparse if c.name == fd.name][0]
        tab = copies[id(deep[c.embedding_name].weight)]
        for d in range(fd.dim):
            one = _Lin()
            one.embedding_dict = {c.embedding_name: type("T", (), {"weight": tab[:, d:d + 1]})()}
            loss = loss + (_pooled_wide(one, fi, c, X) * R_out[:, fd.out_off + d]).sum()
    grads = torch.autograd.grad(loss, [copies[id(p)] for p in params])

    def close(a, b, what):                 # (tests/test_gpu_update.py's bound)
        scale = max(1.0, float(b.abs().max()))
        err = float((a - b).abs().max())
        assert err <= 3e-5 * scale, "%s: max|d|=%.3e (scale %.3g)" % (what, err, scale)
    for p, G in zip(params, grads):
        if mode == "sgd":
            want = before[id(p)] - lr * G
        else:
            s = state[id(p)] + G * G
            want = torch.where(G != 0, before[id(p)] - lr * G / (s.sqrt() + 1e-10), before[id(p)])
            close(opt.state[p]["sum"], torch.where(G != 0, s, state[id(p)]), "state %s" % (tuple(p.shape),))
        close(p.detach(), want, "table %s" % (tuple(p.shape),))
    # the dense half of Linear: its gradient is X_dense^T g_wide[:, n_wide] (an autograd output, not a table)
    dcols = torch.cat([X[:, fi[c.name][0]:fi[c.name][1]] for c in dense], 1)
    want = dcols.double().t() @ R_wide[:, -1].double()
    close(lin.weight.grad.double().reshape(-1), want, "Linear.weight grad")
    assert torch.equal(lin.weight.detach(), w_dense_before)


def test_without_the_bit_nothing_changes():
    """A plan without the mode: wide is [B], its gradient per sample, one sgd update against index_add_."""
    from deepctr_torch._hip import ops
    cols, fi, deep, lin, plan = _setup("fixed", False)
    B = 257
    X = _batch(cols, fi, B, 3)
    plan.update = ("sgd", 0.1)
    before = {k: v.weight.detach().clone() for k, v in lin.embedding_dict.items()}
    out, wide, _ = ops.embed(plan, X, full=True)
    assert wide.shape == (B,)
    r = torch.randn(B, device=DEV)
    (wide * r).sum().backward()
    torch.cuda.synchronize()
    for c in [c for c in cols if c.name.startswith("s")]:
        want = before[c.name].clone()
        want.index_add_(0, X[:, fi[c.name][0]].long(), (-0.1 * r).unsqueeze(1))
        assert float((lin.embedding_dict[c.name].weight.detach() - want).abs().max()) <= 2e-5, c.name
