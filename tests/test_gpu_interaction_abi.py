"""GPU: the older interaction kernels, and the matrix CrossNet of csrc/cross_tower.hip (``test_crossnet_mat*``: the rules of the second
part of interaction_abi's docstring, what each case reaches in the tests' docstrings), through the C ABI at the sizes where
their launchers switch over (csrc/fm.hip,
afm.hip, interact.hip, cross.hip and the SENET / inner-product part of pairwise.hip), against float64 on the CPU.
tests/interaction_abi.py is the driver: padded leading dimensions, sentinel-filled outputs and workspace, the bounds of
tests/test_gpu_pairwise.py (values 1e-5, gradients 2e-5, CrossNet g_kernels 5e-5, each x max(1, max|ref|)), nothing written
outside the documented columns, two backward runs with identical bits, dctr_fm_bwd's ``accumulate``.

What each test reaches, read off the launcher's arithmetic at the test's shape:
  smallest shapes      B = 1 and 5, F = 1 / 2, D = 1, 3, 16, rows padded by 0 and 5 floats, every op; fm at D = 65: pick_lpr
                       stops at 64 lanes, lane 0 walks d = 0 and 64; bi_pooling with 0 and 3 dense values at
                       dense_off = F*D + 2.
  grid stride          afm_groups / groups_of cap the grid at 4096 one-wave workgroups: at B = 4097 workgroup 0 walks two
                       samples (b = 0, 4096) and every other one a single sample, at B = 8200 workgroups 0..7 walk three and
                       the rest two -- the barrier at the head of the loop and the register partials carried over.
  CrossNet             cross_groups: spw = ceil(B / 1024), groups = ceil(B / (4 spw)).
                       (1025, 5, 2)  spw 2, 129 groups: wave 512 owns the single sample 1024 (the `break`), waves 513..515
                                     none -- their zero rows still enter k_cross_reduce;
                       (2051, 69, 3) spw 3, 171 groups, NR = 2: wave 683 owns samples 2049, 2050 and breaks at 2051;
                       (7, 200, 2)   NR = 4 (128 < W <= 256);
                       (6, 2048, 2)  NR = 32 (1024 < W <= 2048), LDS 4 (4 L W + 4 L) = 65 568 B > 64 KB: hipFuncSetAttribute;
                       (5, 2048, 4)  the same with 131 136 B.
  inner product        F*D = 960: 16 rows of 961 floats are 61 504 B > 60 KB, so k_inner_fwd<1> (one sample per workgroup)
                       runs; the backward with the sum keeps 961 + 1771 floats per sample (k_inner_bwd<1>), the one
                       without needs 961 + 28 321 floats = 117 128 B > 60 KB per sample and returns DCTR_ENOSUP by design
                       (layers.pairwise_products sends that shape to PyTorch-ROCm): asserted as such.
  overflow             AFM and Interacting with scores beyond +90 and more than 100 apart inside one softmax (asserted on
                       the float64 reference): expf without the row maximum gives inf / inf.
  empty batch          every op told B = 0 on valid one-row buffers (the header promises DCTR_OK before any buffer check only
                       for the CCPM / DIN entry points; these ops validate their pointers first): DCTR_OK, nothing written,
                       parameter gradients zeroed.
  envelope             AFM D = 65, A = 33, F = 65; Interacting D = 33, F = 65; bilinear D = 17; CrossNet W = 2049 and the
                       backward's LDS at W = 2048, L = 5 (163 920 B > 150 KB): DCTR_ENOSUP, outputs untouched.  One step
                       inside: AFM's backward at (F, D, A) = (64, 64, 32) would need 774 KB of LDS (lds_bytes) and is refused,
                       its forward (41 KB) is checked; the full check runs at (2, 64, 32) and at the largest D the 150 KB
                       admit beside F = 64: (64, 12, 4) and (64, 8, 8) -- both above 64 KB, AFM's hipFuncSetAttribute branch.
                       Interacting at (F, D, H) = (64, 32, 1), which dctr_interacting_supported accepts (H = 2 it does not).

Bounds: every case, the B = 8200 and overflow ones included, is held to the project bounds above; none needed a measured
allowance.  (For comparison, the same formulas in plain float32 torch ops on the device deviate from float64 by at most
6.1e-6 at the AFM overflow case (gh), 2.7e-6 at Interacting B = 8200 (gW_Query), 1.6e-6 at the Interacting overflow case
(gW_key): the same order as the kernels.)  The largest max|d| / max(1, max|ref|) per tensor are printed (``-s``); on an
MI355X, over all cases of this file:
  fm            y 2.9e-7   gE 9.3e-8                          bi_pooling    out 2.6e-7   gG 7.9e-8
  inner_product out 1.2e-7 gE 2.4e-7                          senet         V 5.5e-8  a 2.2e-8  a1 5.0e-8  gE 5.9e-8
  afm           y 1.2e-7   gE 3.3e-7  gW 2.1e-6  gbias 1.0e-6                   gW1 1.4e-7  gW2 8.2e-8
                gh 7.6e-6  gp 4.1e-7                          crossnet_vec  Y 1.8e-7  gX 1.5e-7  g_kernels 2.3e-7
  interacting   out 1.4e-6 gE 2.4e-6  gW_Query 1.4e-6  gW_key 2.2e-6            g_bias 4.1e-7
                gW_Value 1.0e-6  gW_Res 3.1e-7
and, over max|ref| (not max(1, max|ref|)), for the matrix CrossNet over all its cases:
  crossnet_mat  Y 2.9e-7   gx 5.4e-7   gW (worst layer) 3.3e-7   gbias (worst layer) 1.6e-7"""
import ctypes

import numpy as np
import pytest
import torch

import interaction_abi as IA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENOSUP = IA.ENOSUP
SENT = IA.SENT

PARAM_GRADS = {"fm": (), "bi_pooling": (), "inner_product": (), "senet": ("gW1", "gW2"),
               "afm": ("gW", "gbias", "gh", "gp"), "interacting": ("gW_Query", "gW_key", "gW_Value", "gW_Res"),
               "crossnet_vec": ("g_kernels", "g_bias")}


def _lib():
    from deepctr_torch._hip import lib as L
    return L.lib()


def _refused(case, forward=True, backward=True):
    if forward:
        assert case.forward() == ENOSUP
        assert case.sentinel_everywhere(case.fwd_out)
    if backward:
        assert case.backward() == ENOSUP
        assert case.sentinel_everywhere(case.bwd_out)


@pytest.mark.parametrize("D", IA.SMALL_D)
@pytest.mark.parametrize("op", IA.OPS)
def test_smallest_shapes_and_padded_rows(op, D):
    for case in IA.smallest(_lib(), DEV, op, D):
        case.check()


def test_fm_strided_lanes():
    for B, F, pad, acc in ((1, 1, 0, False), (5, 2, 5, True), (5, 3, 5, False)):
        IA.FMCase(_lib(), DEV, B, F, 65, pad=pad, accumulate=acc, seed=B + F).check()


@pytest.mark.parametrize("B", [4097, 8200])
def test_afm_batch_above_the_grid_cap(B):
    IA.AFMCase(_lib(), DEV, B, 3, 4, 3, pad=5 if B == 4097 else 0, seed=B).check()


@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("B", [4097, 8200])
def test_interacting_batch_above_the_grid_cap(B, res):
    IA.InteractingCase(_lib(), DEV, B, 3, 4, 2, res=res, scaling=not res, pad=5 if B == 4097 else 0, seed=B).check()


@pytest.mark.parametrize("B,W,L", [(1025, 5, 2), (2051, 69, 3), (7, 200, 2), (6, 2048, 2), (5, 2048, 4)])
def test_crossnet_vec_switch_overs(B, W, L):
    IA.CrossNetCase(_lib(), DEV, B, W, L, pad=5 if W != 2048 else 0, seed=W + L).check()
    if W == 2048 and L == 2:
        IA.CrossNetCase(_lib(), DEV, B, W, L, pad=5, seed=1).check()


@pytest.mark.parametrize("reduce", [True, False])
def test_inner_product_one_sample_per_workgroup(reduce):
    case = IA.InnerProductCase(_lib(), DEV, 3, 60, 16, reduce, pad=5, seed=60)
    if reduce:
        case.check()
        return
    case.check(grad=False)
    _refused(case, forward=False)          # 117 128 B of LDS per sample: outside the backward's envelope (see above)


def test_afm_softmax_overflow():
    case = IA.afm_overflow(_lib(), DEV)
    case.check()
    IA.assert_overflows(case)


@pytest.mark.parametrize("res", [True, False])
def test_interacting_softmax_overflow(res):
    case = IA.interacting_overflow(_lib(), DEV, res)
    case.check()
    IA.assert_overflows(case)


def _one_row(op):
    lib = _lib()
    return {"fm": lambda: IA.FMCase(lib, DEV, 1, 2, 3, pad=5),
            "bi_pooling": lambda: IA.BiPoolingCase(lib, DEV, 1, 2, 3, n_dense=3, pad=5),
            "inner_product": lambda: IA.InnerProductCase(lib, DEV, 1, 3, 3, True, pad=5),
            "senet": lambda: IA.SenetCase(lib, DEV, 1, 2, 3, 3, pad=5),
            "afm": lambda: IA.AFMCase(lib, DEV, 1, 3, 4, 3, pad=5),
            "interacting": lambda: IA.InteractingCase(lib, DEV, 1, 3, 4, 2, pad=5),
            "crossnet_vec": lambda: IA.CrossNetCase(lib, DEV, 1, 5, 2, pad=5)}[op]()


@pytest.mark.parametrize("op", IA.OPS)
def test_empty_batch(op):
    case = _one_row(op)
    case.nB = 0
    assert case.forward() == 0
    assert case.sentinel_everywhere(case.fwd_out)
    assert case.backward() == 0
    for name, buf in case.bwd_out.items():
        if name in PARAM_GRADS[op]:
            assert float(np.abs(buf.get()).max()) == 0.0, name
            assert buf.untouched(), name
        else:
            assert case.sentinel_everywhere({name: buf}), name
    if PARAM_GRADS[op]:
        assert set(PARAM_GRADS[op]) <= set(case.bwd_out)


@pytest.mark.parametrize("F,D,A", [(2, 65, 4), (2, 4, 33), (65, 1, 1)])
def test_afm_envelope(F, D, A):
    _refused(IA.AFMCase(_lib(), DEV, 2, F, D, A, pad=5))


def test_afm_one_step_inside_the_envelope():
    lib = _lib()
    IA.AFMCase(lib, DEV, 3, 2, 64, 32, pad=5, seed=1).check()
    IA.AFMCase(lib, DEV, 2, 64, 12, 4, pad=5, seed=2).check()
    IA.AFMCase(lib, DEV, 2, 64, 8, 8, pad=0, seed=3).check()
    corner = IA.AFMCase(lib, DEV, 2, 64, 64, 32, pad=5, seed=4)
    corner.check(grad=False)
    _refused(corner, forward=False)          # the backward's 774 KB of LDS


@pytest.mark.parametrize("F,D,H", [(2, 33, 1), (2, 33, 3), (65, 2, 1)])
def test_interacting_envelope(F, D, H):
    lib = _lib()
    assert lib.dctr_interacting_supported(F, D, H) == 0
    _refused(IA.InteractingCase(lib, DEV, 2, F, D, H, pad=5))


def test_interacting_one_step_inside_the_envelope():
    lib = _lib()
    assert lib.dctr_interacting_supported(64, 32, 1) == 1 and lib.dctr_interacting_supported(64, 32, 2) == 0
    IA.InteractingCase(lib, DEV, 2, 64, 32, 1, pad=5, seed=5).check()


def test_crossnet_vec_envelope():
    lib = _lib()
    _refused(IA.CrossNetCase(lib, DEV, 2, 2049, 1, pad=5))
    case = IA.CrossNetCase(lib, DEV, 1, 2048, 5, pad=0)
    case.check(grad=False)
    _refused(case, forward=False)          # 4 (4 L W + 4 L) = 163 920 B of LDS


def test_bilinear_envelope():
    from deepctr_torch._hip import lib as L
    lib, stream = L.lib(), L.stream_handle(torch.device(DEV))
    B, F, D, P = 2, 2, 17, 1
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    full = lambda *s: torch.full(s, SENT, dtype=torch.float32, device=DEV)  # noqa: E731
    E, Wf, gout = torch.randn(B, F * D, device=DEV), torch.randn(1, D, D, device=DEV), torch.randn(B, P * D, device=DEV)
    sched = torch.tensor([[0, 1, 0, 0]], dtype=torch.int32, device=DEV)
    pair_w = torch.zeros(P, dtype=torch.int32, device=DEV)
    out, gE, gW = full(B, P * D), full(B, F * D), full(1, D, D)
    ws = full(max(1, int(lib.dctr_bilinear_bwd_workspace_floats(B, P, D))))
    assert lib.dctr_bilinear_fwd(ptr(E), F * D, None, 0, ptr(Wf), ptr(sched), 1, P, F, D, B, ptr(out), P * D, None, 0, 0, 0,
                                 stream) == ENOSUP
    assert lib.dctr_bilinear_bwd(ptr(E), F * D, None, 0, ptr(Wf), ptr(sched), 1, 1, ptr(pair_w), 1, P, F, D, B, ptr(gout),
                                 P * D, ptr(gE), None, ptr(gW), ptr(ws), None, 0, stream) == ENOSUP
    torch.cuda.synchronize()
    for t in (out, gE, gW, ws):
        assert float(t.min()) == SENT and float(t.max()) == SENT


# ---- CrossNet, matrix parameterisation (csrc/cross_tower.hip: k_cross_mat_fwd / _bwd + the tower's weight-gradient kernels) -
@pytest.mark.parametrize("B,W,L", IA.CROSSNET_MAT_CASES)
def test_crossnet_mat(B, W, L):
    """the rules of interaction_abi's second part (max|ref| as the scale, guarded 777 / NaN workspace, gW's padding columns
    zero).  A workgroup carries 16 samples: B = 1, 15, 16, 17, 33.  W = 1 .. 512 at L = 1: one to eight 64-column tiles of the
    weight gradient; LDS 16 x 4 x (round_up(W, 64) + 8) x 4 B in the backward -- 51 200 B at W = 192, 67 584 B at W = 193:
    hipFuncSetAttribute from there -- and 16 x 3 x (round_up(W, 16) + 8) x 4 B in the forward -- 62 976 B at W = 320, 66 048 B
    at W = 321: the opt-in, 99 840 B at W = 512.  L = 12 is DCTR_MLP_MAX_LAYERS.  At W = 40 the
    weight gradient's batch slices S = min(B / 64, 16) change at B = 64, 128 and 1024.
    (Found here: at W = 64, 192, 320, 512 with ld_w = W + 4 the padding columns of gW lie past the last 64-column tile of
    k_mlp_wgrad; no partial was written there and k_mlp_reduce summed what the workspace held -- NaN under this driver.
    The last tile of a row writes those zeros now.)"""
    IA.CrossNetMatCase(_lib(), DEV, B, W, L).check()


def test_crossnet_mat_smallest_shapes():
    for D in IA.SMALL_D:
        for case in IA.smallest(_lib(), DEV, "crossnet_mat", D):
            case.check()


def _mat_refused(case, code, forward=True):
    if forward:
        assert case.forward() == code
        assert case.sentinel_everywhere(case.fwd_out)
    assert case.backward() == code
    assert case.sentinel_everywhere(case.bwd_out)


def test_crossnet_mat_envelope_and_argument_checks():
    """W = 513: DCTR_ENOSUP; a leading dimension that is no multiple of 4: DCTR_EALIGN; a non-NULL w_out: DCTR_EINVAL -- each
    before any launch, the outputs untouched; B = 0: DCTR_OK, nothing written"""
    lib = _lib()
    assert lib.dctr_crossnet_mat_supported(512, 1) == 1 and lib.dctr_crossnet_mat_supported(513, 1) == 0
    _mat_refused(IA.CrossNetMatCase(lib, DEV, 2, 513, 1), ENOSUP)
    for which in ("x", "w", "h"):          # W = 5 in rows of 8 floats, told 7
        case = IA.CrossNetMatCase(lib, DEV, 2, 5, 2)
        case.force_ld[which] = 7
        _mat_refused(case, IA.EALIGN)
    case = IA.CrossNetMatCase(lib, DEV, 2, 5, 2)
    case.force_ld["gx"] = 7
    _mat_refused(case, IA.EALIGN, forward=False)
    case = IA.CrossNetMatCase(lib, DEV, 2, 5, 2)
    case.w_out = case.bs[0]
    _mat_refused(case, IA.EINVAL)
    case = IA.CrossNetMatCase(lib, DEV, 1, 5, 2)
    case.nB = 0
    _mat_refused(case, 0)


def test_zz_report():
    IA.report()
