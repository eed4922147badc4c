"""Host tests of ``_hip/marshal.py`` on CPU tensors over the ``mock`` stand-in: which tensors pass through to the C ABI
without a copy (the models' step times rest on the column-slice views of the gather's output doing so), which leading
dimension goes with them, and what a copy looks like when one is needed."""
import pytest
import torch

from deepctr_torch._hip import lib as L
from deepctr_torch._hip import marshal as M


@pytest.fixture()
def buf():
    return torch.arange(100, dtype=torch.float32).reshape(5, 20)


# ---- rows2 ------------------------------------------------------------------------------------------------------------
def test_rows2_contiguous_is_the_same_object(mock):
    t = torch.randn(5, 8)
    out, ld = M.rows2(t, "t")
    assert out is t and ld == 8


def test_rows2_column_slice_passes_through(mock, buf):
    v = buf[:, 4:12]
    out, ld = M.rows2(v, "v")
    assert out is v and out.data_ptr() == v.data_ptr() == buf.data_ptr() + 4 * 4 and ld == 20


def test_rows2_one_row_slice_has_its_width_as_ld(mock, buf):
    v = buf[2:3, 4:12]
    out, ld = M.rows2(v, "v")
    assert out is v and ld == 8


def test_rows2_converts_float64(mock):
    t = torch.randn(5, 8, dtype=torch.float64)
    out, ld = M.rows2(t, "t")
    assert out.dtype == torch.float32 and ld == 8
    assert torch.equal(out, t.float())


def test_rows2_copies_a_transposed_tensor(mock):
    t = torch.randn(8, 5).t()
    out, ld = M.rows2(t, "t")
    assert out is not t and out.is_contiguous() and ld == 8
    assert torch.equal(out, t)


def test_rows2_copies_an_expanded_tensor(mock):
    t = torch.randn(1, 8).expand(5, 8)
    out, ld = M.rows2(t, "t")
    assert out.data_ptr() != t.data_ptr() and out.stride() == (8, 1) and ld == 8
    assert torch.equal(out, t)


def test_rows2_requires_the_gpu():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.rows2(torch.zeros(2, 2), "t")


# ---- rows3 ------------------------------------------------------------------------------------------------------------
def test_rows3_view_of_a_wider_buffer_passes_through(mock):
    full = torch.randn(4, 40)
    v = full[:, :24].view(4, 3, 8)
    out, ld = M.rows3(v, "v")
    assert out is v and out.data_ptr() == full.data_ptr() and ld == 40


def test_rows3_copies_a_permuted_tensor(mock):
    t = torch.randn(3, 4, 8).permute(1, 0, 2)
    out, ld = M.rows3(t, "t")
    assert out is not t and out.is_contiguous() and ld == 24
    assert torch.equal(out, t)


# ---- padded_rows ------------------------------------------------------------------------------------------------------
def _aligned(shape):
    """a float32 tensor whose base pointer is a multiple of 16 bytes"""
    raw = torch.randn(shape[0] * shape[1] + 4)
    off = (-raw.data_ptr() // 4) % 4
    return raw[off:off + shape[0] * shape[1]].view(shape)


def test_padded_rows_copies_a_misaligned_base():
    base = _aligned((5, 20))
    v = base[:, 1:9]
    assert v.data_ptr() % 16 != 0
    out, ld = M.padded_rows(v)
    assert out.data_ptr() != v.data_ptr() and ld == out.stride(0) and ld % 4 == 0 and out.data_ptr() % 16 == 0
    assert torch.equal(out[:, :8], v) and not out[:, 8:].any()


def test_padded_rows_pads_width_6_to_8_with_zeros():
    t = torch.randn(5, 6)
    out, ld = M.padded_rows(t)
    assert ld == 8 and tuple(out.shape) == (5, 8)
    assert torch.equal(out[:, :6], t) and torch.equal(out[:, 6:], torch.zeros(5, 2))


def test_padded_rows_aligned_strided_slice_passes_through():
    base = _aligned((5, 20))
    v = base[:, 4:12]
    out, ld = M.padded_rows(v)
    assert out is v and ld == 20


def test_padded_rows_ld_min_widens_the_copy():
    base = _aligned((5, 8))
    assert M.padded_rows(base)[0] is base
    out, ld = M.padded_rows(base, ld_min=10)
    assert out is not base and ld == 12 and tuple(out.shape) == (5, 12)
    assert torch.equal(out[:, :8], base) and not out[:, 8:].any()
    wide = _aligned((5, 12))[:, :8]
    assert M.padded_rows(wide, ld_min=10)[0] is wide


def test_padded_rows_vec_sets_the_alignment():
    v = _aligned((5, 20))[:, 1:9]           # 4-byte aligned base, row stride 20
    assert M.padded_rows(v, vec=1)[0] is v
    assert M.padded_rows(v, vec=2)[0] is not v


# ---- workspace / call -------------------------------------------------------------------------------------------------
def test_workspace_is_never_empty(mock, monkeypatch):
    monkeypatch.setattr(mock, "dctr_afm_bwd_workspace_floats", lambda *a: 0, raising=False)
    ws = M.workspace("dctr_afm_bwd_workspace_floats", 4, 8, 2, device="cpu")
    assert ws.dtype == torch.float32 and tuple(ws.shape) == (1,)
    monkeypatch.setattr(mock, "dctr_afm_bwd_workspace_floats", lambda B, D, A: B * D * A, raising=False)
    assert M.workspace("dctr_afm_bwd_workspace_floats", 4, 8, 2, device="cpu").numel() == 64


def test_call_raises_naming_the_entry_point(mock, monkeypatch):
    monkeypatch.setattr(mock, "dctr_fm_fwd", lambda *a: L.EINVAL, raising=False)
    with pytest.raises(RuntimeError, match="dctr_fm_fwd failed"):
        M.call("dctr_fm_fwd", None, 0, 0, 0, 0, None, None)


def test_call_returns_none_on_success(mock, monkeypatch):
    seen = []
    monkeypatch.setattr(mock, "dctr_fm_fwd", lambda *a: seen.append(a) or 0, raising=False)
    assert M.call("dctr_fm_fwd", 1, 2, 3) is None
    assert seen == [(1, 2, 3)]
