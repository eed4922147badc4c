"""GPU: dctr_iafm_fwd / dctr_iafm_bwd (csrc/iafm.hip) through the C ABI against a torch fp64 expression of the formulas
include/dctr.h documents (what ifm.py:74-83, difm.py:96-102 and basemodel.py:80-91 compute): values at 1e-5 x scale, every
gradient at 2e-5 x scale.  Both modes, odd batches, every lane layout (D 16 / 8 / 4 -> dwordx4, D 6 -> dwordx2, D 3 -> dword),
1 and 64 fields, a strided E with a poisoned tail, no sparse linear side, no linear side, logits a naive exp overflows on,
bit-reproducibility."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SOFTMAX, SUM = 0, 1
SHAPES = [(4096, 26, 16), (4099, 26, 16), (33, 7, 4), (17, 1, 8), (20, 5, 6), (64, 39, 3), (8, 64, 16)]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _reference(E, Wl, n_wl, Z1, Z2, mode):
    """fp64: (m, y_lin, y_fm)"""
    B, F, D = E.shape
    m = F * torch.softmax(Z1, dim=1) if mode == SOFTMAX else Z1 + Z2
    y_lin = torch.zeros(B, dtype=E.dtype, device=E.device)
    if Wl is not None:
        if n_wl:
            y_lin = y_lin + (m * Wl[:, :n_wl]).sum(1)
        y_lin = y_lin + Wl[:, n_wl]
    v = E * m.unsqueeze(-1)
    return m, y_lin, 0.5 * (v.sum(1).pow(2) - v.pow(2).sum(1)).sum(1)


def _close(a, r, what, tol):
    scale = max(1.0, float(r.abs().max())) if r.numel() else 1.0
    err = float((a.double() - r).abs().max()) if r.numel() else 0.0
    print("%-6s max|d| = %.3e (scale %.3g, bound %.1e)" % (what, err, scale, tol * scale))
    assert err <= tol * scale, "%s: max|d|=%.3e (scale %.3g)" % (what, err, scale)


def _inputs(B, F, D, mode, pad, linear, zmag, seed):
    g = torch.Generator().manual_seed(seed)
    ld_e = F * D + pad
    Ebuf = torch.full((B, ld_e), float("nan"))
    Ebuf[:, :F * D] = torch.randn(B, F * D, generator=g) * 0.5
    Z1 = torch.randn(B, F, generator=g) * zmag
    Z2 = torch.randn(B, F, generator=g) if mode == SUM else None
    n_wl = F if linear == "full" else 0
    Wl = None if linear == "none" else torch.randn(B, n_wl + 1, generator=g)
    g_lin, g_fm = torch.randn(B, generator=g), torch.randn(B, generator=g)
    mv = lambda t: None if t is None else t.to(DEV)                                   # noqa: E731
    return mv(Ebuf), mv(Wl), n_wl, mv(Z1), mv(Z2), mv(g_lin), mv(g_fm)


def _run(B, F, D, mode, Ebuf, Wl, n_wl, Z1, Z2, g_lin, g_fm):
    from deepctr_torch._hip import lib as L
    lib = L.lib()
    assert lib.dctr_iafm_supported(F, D) == 1
    ld_e = Ebuf.shape[1]
    m = torch.empty(B, F, device=DEV)
    y_lin, y_fm = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    s = L.stream_handle(DEV)
    L.check(lib.dctr_iafm_fwd(_p(Ebuf), ld_e, _p(Wl), n_wl + 1 if Wl is not None else 0, n_wl, _p(Z1), F, _p(Z2), F, mode,
                              B, F, D, _p(m), F, _p(y_lin), _p(y_fm), s), "dctr_iafm_fwd")
    POISON = -777.0
    gE = torch.full((B, ld_e), POISON, device=DEV)
    gWl = torch.full_like(Wl, POISON) if Wl is not None else None
    gZ = torch.full((B, F), POISON, device=DEV)
    L.check(lib.dctr_iafm_bwd(_p(Ebuf), ld_e, _p(Wl), n_wl + 1 if Wl is not None else 0, n_wl, _p(m), F, mode, B, F, D,
                              _p(g_lin), _p(g_fm), _p(gE), ld_e, _p(gWl), n_wl + 1 if Wl is not None else 0, _p(gZ), F, s),
            "dctr_iafm_bwd")
    torch.cuda.synchronize()
    return m, y_lin, y_fm, gE, gWl, gZ


def _check(B, F, D, mode, pad=0, linear="full", zmag=1.0, seed=0):
    Ebuf, Wl, n_wl, Z1, Z2, g_lin, g_fm = _inputs(B, F, D, mode, pad, linear, zmag, seed)
    m, y_lin, y_fm, gE, gWl, gZ = _run(B, F, D, mode, Ebuf, Wl, n_wl, Z1, Z2, g_lin, g_fm)
    E64 = Ebuf[:, :F * D].double().reshape(B, F, D).requires_grad_(True)
    W64 = Wl.double().requires_grad_(True) if Wl is not None else None
    Z164 = Z1.double().requires_grad_(True)
    Z264 = Z2.double().requires_grad_(True) if Z2 is not None else None
    rm, rl, rf = _reference(E64, W64, n_wl, Z164, Z264, mode)
    ins = [t for t in (E64, W64, Z164, Z264) if t is not None]
    gs = torch.autograd.grad((rl * g_lin.double()).sum() + (rf * g_fm.double()).sum(), ins, allow_unused=True)
    gs = dict(zip([id(t) for t in ins], gs))
    assert torch.isfinite(m).all() and torch.isfinite(y_lin).all() and torch.isfinite(y_fm).all()
    _close(m, rm.detach(), "m", 1e-5)
    _close(y_lin, rl.detach(), "y_lin", 1e-5)
    _close(y_fm, rf.detach(), "y_fm", 1e-5)
    _close(gE[:, :F * D], gs[id(E64)].reshape(B, F * D), "gE", 2e-5)
    if pad:
        assert bool((gE[:, F * D:] == -777.0).all()), "columns past the field block were written"
    if W64 is not None:
        gw = gs[id(W64)]
        _close(gWl, gw if gw is not None else torch.zeros_like(W64), "gWl", 2e-5)
    gz = gs[id(Z164)]
    _close(gZ, gz, "gZ", 2e-5)
    if Z264 is not None:
        _close(gZ, gs[id(Z264)], "gZ2", 2e-5)        # (one buffer serves Z1 and Z2)
    return m, y_lin, y_fm, gE, gWl, gZ


@pytest.mark.parametrize("mode", [SOFTMAX, SUM], ids=["softmax", "sum"])
@pytest.mark.parametrize("B,F,D", SHAPES)
def test_iafm_matches_fp64(B, F, D, mode):
    _check(B, F, D, mode, seed=B + F + D)


@pytest.mark.parametrize("mode", [SOFTMAX, SUM], ids=["softmax", "sum"])
@pytest.mark.parametrize("B,F,D,pad", [(4099, 26, 16, 16), (33, 7, 4, 4), (20, 5, 6, 2), (64, 39, 3, 3), (20, 5, 6, 3)])
def test_strided_rows_and_untouched_tail(B, F, D, pad, mode):
    """ld_e > F*D (the gather's padded buffer with its dense block): the tail is neither read (it holds NaN) nor written;
    an odd stride makes the rows fall back to narrower loads."""
    _check(B, F, D, mode, pad=pad, seed=pad)


@pytest.mark.parametrize("mode", [SOFTMAX, SUM], ids=["softmax", "sum"])
@pytest.mark.parametrize("linear", ["dense_only", "none"])
@pytest.mark.parametrize("B,F,D", [(4099, 26, 16), (20, 5, 6), (17, 1, 8)])
def test_linear_side_variants(B, F, D, linear, mode):
    """n_wl = 0 (a linear side of dense columns only: m does not touch y_lin) and Wl = NULL (y_lin = 0)."""
    m, y_lin, *_ = _check(B, F, D, mode, linear=linear, seed=3)
    if linear == "none":
        assert float(y_lin.abs().max()) == 0.0


@pytest.mark.parametrize("B,F,D", [(4096, 26, 16), (64, 39, 3), (8, 64, 16)])
def test_softmax_is_stable(B, F, D):
    """Z1 of magnitude 60: exp(z) overflows fp32 at 88.7, the row maximum must be subtracted first."""
    _check(B, F, D, SOFTMAX, zmag=60.0, seed=7)


def test_one_field_is_the_identity_factor():
    """F = 1: m = 1, FM = 0, no gradient reaches Z (IFM's P gets a zero gradient, like the reference's)."""
    m, y_lin, y_fm, gE, gWl, gZ = _check(17, 1, 8, SOFTMAX, seed=1)
    assert float((m - 1).abs().max()) == 0.0 and float(y_fm.abs().max()) == 0.0 and float(gZ.abs().max()) == 0.0


@pytest.mark.parametrize("mode", [SOFTMAX, SUM], ids=["softmax", "sum"])
def test_bit_reproducible(mode):
    args = _inputs(4099, 26, 16, mode, 16, "full", 1.0, 11)
    a = _run(4099, 26, 16, mode, *args)
    b = _run(4099, 26, 16, mode, *args)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_unsupported_shapes_are_refused():
    from deepctr_torch._hip import lib as L
    lib = L.lib()
    assert lib.dctr_iafm_supported(65, 16) == 0 and lib.dctr_iafm_supported(64, 64) == 0
    assert lib.dctr_iafm_supported(26, 16) == 1 and lib.dctr_iafm_supported(1, 1) == 1
    B, F, D = 4, 64, 64
    E = torch.zeros(B, F * D, device=DEV)
    Z = torch.zeros(B, F, device=DEV)
    m, y = torch.empty(B, F, device=DEV), torch.empty(B, device=DEV)
    rc = lib.dctr_iafm_fwd(_p(E), F * D, None, 0, 0, _p(Z), F, None, 0, SOFTMAX, B, F, D, _p(m), F, _p(y), _p(y),
                           L.stream_handle(DEV))
    assert rc == L.ENOSUP
