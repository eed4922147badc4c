"""CPU: the C-ABI driver of the interaction kernels (tests/interaction_abi.py) over the stand-in library
(tests/mock_ops.py honours the leading dimensions and the column rule): the driver's marshalling and its float64 references
are right before a device sees them -- and its checks bite: nine deliberately wrong stand-ins each make ``check()`` raise.
The stand-in does not model ``B == 0`` or ``DCTR_ENOSUP``: tests/test_gpu_interaction_abi.py and tests/test_gpu_cin_abi.py
have those.  For the CIN layer and the matrix CrossNet the file also shows that float32 arithmetic itself stays within a
quarter of each bound at every shape the device files use (as tests/test_dien_host.py does for DIEN)."""
import ctypes

import pytest

import numpy as np

import interaction_abi as IA
from mock_lib import _arr

DEV = "cpu"


@pytest.mark.parametrize("D", IA.SMALL_D)
@pytest.mark.parametrize("op", IA.OPS)
def test_smallest_shapes_over_the_stand_in(mock, op, D):
    n = 0
    for case in IA.smallest(mock, DEV, op, D):
        case.check()
        n += 1
    assert n >= 4
    assert any(c.startswith(op.split("_")[0]) for c in mock.calls)


def test_fm_strided_lanes_over_the_stand_in(mock):
    IA.FMCase(mock, DEV, 5, 2, 65, pad=5, accumulate=True).check()


def test_overflow_cases_are_what_they_claim(mock):
    """the inputs of the device file's overflow tests: scores past expf's range, and still finite through a stable softmax"""
    for case in (IA.afm_overflow(mock, DEV), IA.interacting_overflow(mock, DEV, True),
                 IA.interacting_overflow(mock, DEV, False)):
        case.reference(grad=False)
        IA.assert_overflows(case)
    tame = IA.AFMCase(mock, DEV, 5, 3, 4, 3)
    tame.reference(grad=False)
    with pytest.raises(AssertionError):
        IA.assert_overflows(tame)


# ---- the checks bite ---------------------------------------------------------------------------------------------------
def test_check_catches_a_write_past_the_documented_columns(mock, monkeypatch):
    real = mock.dctr_inner_product_fwd

    def bad(E, ld_e, B, F, D, reduce, out, ld_o, stream):
        rc = real(E, ld_e, B, F, D, reduce, out, ld_o, stream)
        P = F * (F - 1) // 2
        _arr(out, (B, P + 1), ld_o)[B - 1, P] = 0.0          # one float behind the last row's P columns
        return rc
    monkeypatch.setattr(mock, "dctr_inner_product_fwd", bad)
    with pytest.raises(AssertionError, match="outside the documented columns"):
        IA.InnerProductCase(mock, DEV, 5, 3, 3, True, pad=5).check()
    monkeypatch.setattr(mock, "dctr_inner_product_fwd", real)
    IA.InnerProductCase(mock, DEV, 5, 3, 3, True, pad=5).check()


def test_check_catches_an_ignored_leading_dimension(mock, monkeypatch):
    real = mock.dctr_afm_fwd

    def bad(E, ld_e, B, F, D, A, W, bias, h, p, y, stream):
        return real(E, F * D, B, F, D, A, W, bias, h, p, y, stream)          # rows F*D apart whatever ld_e says
    monkeypatch.setattr(mock, "dctr_afm_fwd", bad)
    with pytest.raises(AssertionError, match=r"afm y: (max\|d\||not finite)"):
        IA.AFMCase(mock, DEV, 5, 3, 4, 3, pad=5).check()
    IA.AFMCase(mock, DEV, 5, 3, 4, 3, pad=0).check()          # (without padding the two agree: the case needs its pad)


def test_check_catches_a_sample_missing_from_a_parameter_gradient(mock, monkeypatch):
    real = mock.dctr_crossnet_vec_bwd

    def bad(X, ld_x, B, W, L, kernels, bias, gY, ld_g, gX, ld_gx, g_kernels, g_bias, ws, stream):
        rc = real(X, ld_x, B, W, L, kernels, bias, gY, ld_g, gX, ld_gx, g_kernels, g_bias, ws, stream)
        # gX keeps all B rows; the parameter gradients are summed over the first B - 1 samples only
        return rc or real(X, ld_x, B - 1, W, L, kernels, bias, gY, ld_g, gX, ld_gx, g_kernels, g_bias, ws, stream)
    monkeypatch.setattr(mock, "dctr_crossnet_vec_bwd", bad)
    with pytest.raises(AssertionError, match=r"crossnet_vec g_(kernels|bias): max\|d\|"):
        IA.CrossNetCase(mock, DEV, 5, 7, 2, pad=5).check()


def test_pointers_are_plain_ctypes(mock):
    c = IA.FMCase(mock, DEV, 2, 2, 3, pad=1)
    assert isinstance(c.E.ptr(), ctypes.c_void_p) and c.E.ld == 7 and c.stream is None


# ---- the CIN layer, its glue and the matrix CrossNet ---------------------------------------------------------------------
@pytest.mark.parametrize("D", IA.SMALL_D)
@pytest.mark.parametrize("op", IA.NEW_OPS)
def test_smallest_shapes_of_the_cin_and_matrix_ops_over_the_stand_in(mock, op, D):
    n = 0
    for case in IA.smallest(mock, DEV, op, D):
        case.check()
        n += 1
    assert n >= 4
    assert any(c.startswith(op.split("_")[0]) for c in mock.calls)


def test_cin_layer_paths_over_the_stand_in(mock):
    """the symmetric split at an odd and an even M, the same inputs in two buffers, every leading dimension padded, H as the
    first half of a wider map, accumulate_x0, the options"""
    for kw in (dict(B=3, h=5, M=5, D=3, O=4, sym=True), dict(B=3, h=5, M=5, D=3, O=4, same=True),
               dict(B=3, h=6, M=6, D=3, O=4, sym=True, accumulate=True, pad=2),
               dict(B=3, h=2, M=3, D=4, O=5, pads=dict(h=3, x0=5, a=2, gh=7, gx=1)),
               dict(B=3, h=2, M=3, D=4, O=5, pads=dict(h=8), accumulate=True),
               dict(B=3, h=2, M=3, D=4, O=5, relu=0, bias=False, gbias=False)):
        IA.CinLayerCase(mock, DEV, **kw).check()


def test_cin_pool_positions_over_the_stand_in(mock):
    for kw in (dict(n_hidden=2, pool_from=2, w_head=True), dict(n_hidden=4, pool_from=0), dict(n_hidden=0, pool_from=0),
               dict(n_hidden=2, pool_from=2, lead=1, relu=False), dict(n_hidden=2, pool_from=2, pooled_grad=False),
               dict(n_hidden=0, pool_from=0, pooled_grad=False)):
        IA.CinPoolCase(mock, DEV, 3, 4, 4, pad=3, **kw).check()


def test_a_reference_that_is_zero_asks_for_exact_zeros(mock, monkeypatch):
    real = mock.dctr_cin_pool_bwd

    def bad(g_hidden, g_pooled, ld_gp, w_head, A_relu, B, O, D, n_hidden, pool_from, gA, stream):
        rc = real(g_hidden, g_pooled, ld_gp, w_head, A_relu, B, O, D, n_hidden, pool_from, gA, stream)
        _arr(gA, (B * O * D,))[3] = 1e-30
        return rc
    monkeypatch.setattr(mock, "dctr_cin_pool_bwd", bad)
    with pytest.raises(AssertionError, match="cin_pool gA: .*identically zero"):
        IA.CinPoolCase(mock, DEV, 3, 4, 4, 0, 0, pooled_grad=False).check()


def _cin_bwd_variant(mock, monkeypatch, change):
    """``change(args) -> args`` applied to the arguments of the stand-in's dctr_cin_layer_bwd, ``after(args)`` once it ran"""
    real = mock.dctr_cin_layer_bwd
    names = ("gA", "A", "ld_a", "relu", "H", "ld_h", "X0", "ld_x0", "W", "B", "h", "M", "D", "O", "gH", "ld_gh", "gX0",
             "ld_gx", "accumulate_x0", "gW", "gbias", "ws", "stream")

    def bad(*args):
        a = dict(zip(names, args))
        after = change(a)
        rc = real(*[a[n] for n in names])
        if after:
            after(a)
        return rc
    monkeypatch.setattr(mock, "dctr_cin_layer_bwd", bad)
    return real


def test_check_catches_a_write_behind_the_advertised_workspace(mock, monkeypatch):
    def change(a):
        def after(a):
            n = mock.dctr_cin_bwd_workspace_floats(a["B"], a["h"], a["M"], a["D"], a["O"])
            _arr(a["ws"], (n + 1,))[n] = 0.0
        return after
    real = _cin_bwd_variant(mock, monkeypatch, change)
    with pytest.raises(AssertionError, match="cin_layer backward workspace: a float behind the advertised size"):
        IA.CinLayerCase(mock, DEV, 5, 2, 3, 4, 5, pad=1).check()
    monkeypatch.setattr(mock, "dctr_cin_layer_bwd", real)
    IA.CinLayerCase(mock, DEV, 5, 2, 3, 4, 5, pad=1).check()


def test_check_catches_an_ignored_ld_gh(mock, monkeypatch):
    def change(a):
        a["ld_gh"] = a["h"] * a["D"]          # rows h*D apart whatever ld_gh says
    _cin_bwd_variant(mock, monkeypatch, change)
    with pytest.raises(AssertionError, match=r"cin_layer gH: max\|d\|"):
        IA.CinLayerCase(mock, DEV, 5, 2, 3, 4, 5, pad=1).check()
    IA.CinLayerCase(mock, DEV, 5, 2, 3, 4, 5, pad=0).check()          # (without padding the two agree)


def test_check_catches_an_ignored_accumulate_x0(mock, monkeypatch):
    def change(a):
        a["accumulate_x0"] = 0
    _cin_bwd_variant(mock, monkeypatch, change)
    with pytest.raises(AssertionError, match=r"cin_layer gX0: max\|d\|"):
        IA.CinLayerCase(mock, DEV, 5, 2, 3, 4, 5, pad=1, accumulate=True).check()
    IA.CinLayerCase(mock, DEV, 5, 2, 3, 4, 5, pad=1).check()


def test_check_catches_a_lost_second_chunk_of_the_weight_gradient(mock, monkeypatch):
    def change(a):
        def after(a):
            _arr(a["gW"], (a["O"], a["h"] * a["M"]))[128:] = 0.0          # the output rows >= 128 never arrive
        return after
    _cin_bwd_variant(mock, monkeypatch, change)
    with pytest.raises(AssertionError, match=r"cin_layer gW: max\|d\|"):
        IA.CinLayerCase(mock, DEV, 2, 2, 3, 2, 130, pad=1).check()
    IA.CinLayerCase(mock, DEV, 2, 2, 3, 2, 128, pad=1).check()


def test_check_catches_a_dropped_partial_group_of_rows(mock, monkeypatch):
    real = mock.dctr_rows_tdot

    def bad(x, ld_x, w, B, N, out, ws, stream):
        return real(x, ld_x, w, B // 32 * 32 if B > 32 else B, N, out, ws, stream)          # the last, partial group of 32
    monkeypatch.setattr(mock, "dctr_rows_tdot", bad)
    with pytest.raises(AssertionError, match=r"rows_tdot out: max\|d\|"):
        IA.RowsTdotCase(mock, DEV, 33, 5, pad=1).check()
    IA.RowsTdotCase(mock, DEV, 32, 5, pad=1).check()


def test_check_catches_a_sample_missing_from_the_matrix_crossnet_bias_gradient(mock, monkeypatch):
    real = mock.dctr_crossnet_mat_bwd

    def bad(mref, x, ld_x, B, gY, ld_g, gx, ld_gx, ws, stream):
        m = mref._obj
        W = m.layer[0].K
        rc = real(mref, x, ld_x, B - 1, gY, ld_g, gx, ld_gx, ws, stream)
        short = [_arr(m.layer[l].gbias, (W,)).copy() for l in range(m.n_layers)]
        rc = rc or real(mref, x, ld_x, B, gY, ld_g, gx, ld_gx, ws, stream)
        for l in range(m.n_layers):
            _arr(m.layer[l].gbias, (W,))[...] = short[l]          # gx and gW keep all B samples, gbias lacks the last
        return rc
    monkeypatch.setattr(mock, "dctr_crossnet_mat_bwd", bad)
    with pytest.raises(AssertionError, match=r"crossnet_mat gbias\d: max\|d\|"):
        IA.CrossNetMatCase(mock, DEV, 5, 7, 2).check()
    monkeypatch.setattr(mock, "dctr_crossnet_mat_bwd", real)
    IA.CrossNetMatCase(mock, DEV, 5, 7, 2).check()


def test_the_stand_in_refuses_a_short_leading_dimension(mock):
    for name in ("a", "h", "x0", "gh", "gx"):
        case = IA.CinLayerCase(mock, DEV, 2, 2, 3, 4, 5, pad=1)
        case.force_ld[name] = {"a": 5 * 4, "h": 2 * 4, "x0": 3 * 4, "gh": 2 * 4, "gx": 3 * 4}[name] - 1
        assert case.backward() == IA.EINVAL, name
        assert case.sentinel_everywhere(case.bwd_out), name


# ---- float32 itself keeps within a quarter of each bound -------------------------------------------------------------------
def _quarter(case):
    for name, (ratio, bound) in sorted(case.float32_ratios().items()):
        print("%s %s: float32 max|d| / max|ref| %.3e (a quarter of the bound: %.2e)" % (case.op, name, ratio, 0.25 * bound))
        assert ratio <= 0.25 * bound, "%s %s: float32 deviates by %.3e x max|ref|, bound %.1e" % (case.op, name, ratio, bound)


@pytest.mark.parametrize("kw", [kw for _, kw in IA.CIN_LAYER_CASES], ids=[i for i, _ in IA.CIN_LAYER_CASES])
def test_float32_keeps_a_quarter_of_the_cin_bounds(mock, kw):
    _quarter(IA.CinLayerCase(mock, DEV, **kw))


@pytest.mark.parametrize("B,W,L", IA.CROSSNET_MAT_CASES)
def test_float32_keeps_a_quarter_of_the_matrix_crossnet_bounds(mock, B, W, L):
    _quarter(IA.CrossNetMatCase(mock, DEV, B, W, L))


@pytest.mark.parametrize("D", IA.SMALL_D)
@pytest.mark.parametrize("op", ["cin_layer", "crossnet_mat"])
def test_float32_keeps_a_quarter_of_the_bounds_at_the_smallest_shapes(mock, op, D):
    """the ``smallest()`` cases run on the device too"""
    for case in IA.smallest(mock, DEV, op, D):
        _quarter(case)
