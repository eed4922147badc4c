"""CPU: the C-ABI driver of the older interaction kernels (tests/interaction_abi.py) over the stand-in library
(tests/mock_ops.py honours the leading dimensions and the column rule): the driver's marshalling and its float64 references
are right before a device sees them -- and its checks bite: three deliberately wrong stand-ins each make ``check()`` raise.
The stand-in does not model ``B == 0`` or ``DCTR_ENOSUP``: tests/test_gpu_interaction_abi.py has those."""
import ctypes

import pytest

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
