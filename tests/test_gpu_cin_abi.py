"""GPU: the CIN kernels of csrc/cin.hip and xDeepFM's glue (dctr_cin_layer_*, dctr_cin_pool_*, dctr_rows_dot, dctr_rows_tdot)
through the C ABI, against float64 on the CPU.  tests/interaction_abi.py is the driver (the rules of its docstring's second
part): padded leading dimensions, sentinel-filled outputs, workspaces of exactly the advertised size with a guard behind them
and 777 / NaN inside, values within 1e-5 x max|ref| and gradients within 2e-5 x max|ref| (NOT max(1, max|ref|)), the saved
activation handed to the backward is the float64 forward rounded to float32, a second run with identical bits.

What each case reaches is in its id and in ``interaction_abi._cin_layer_cases`` (read off the launchers' arithmetic):
  O               the forward's k_cin_fwd<OT, CT> for OT = 1..4, its separately launched narrower last chunk (O_pad % 128 != 0
                  beyond the first chunk), the backward's chunks of 128 adding up in gH / gX0
  cols            B * D around the 256-column tile of the data kernels; a sample straddles the tile edge at D = 3, 5, 17
  M               1, 2, 31, 32 (an odd M pads to M_pad); M = 33 is refused with DCTR_ENOSUP both ways, nothing written
  wgrad           h * M = 255 / 256 / 258 / 1664: 1 / 1 / 2 / 7 column groups of k_cin_wgrad; hspan = min(h, 255 / M + 2)
                  switches between h = 10, 11 and 12 at M = 26; B * D = 64 / 65: one / two partial sets; B = 2100, D = 16:
                  the cap of 512 partial sets; (h, M) = (93, 2) / (94, 2) / (130, 1): ph = 93 / 95 / 131 -- from 95 on
                  k_cin_wgrad opts in to more than 64 KB of dynamic LDS
  flat            k_cin_bwd_data_flat<3 | 4, 26> (M = 26, H != X0, three or four row tiles): not taken at O = 64, one flat chunk
                  and a regular one at O = 129, two flat chunks (the second accumulating) at O = 224
  sym             one buffer for H and X0: k_cin_prep_wsym + k_cin_bwd_data_sym + k_cin_wgrad_reduce_sym; gH and gX0 hold the
                  split include/dctr.h documents and add up to the gradient on X0; M = 5, O = 8, B = 64 is the shape whose
                  folded weight slices once overran the workspace (3072 floats into 832); ``two-buffers``: the same inputs
                  through the general kernels, same float64 reference
  options         relu x bias x gbias, accumulate_x0 on the general (O > 128), symmetric and flat paths, every leading
                  dimension padded, H as the first half of a map twice as wide, B = 0, short leading dimensions refused
  pool / rows     as the tests say

The largest max|d| / max|ref| per tensor are printed (``-s``); on an MI355X, over all cases of this file:
  cin_layer  A 3.3e-6   gH 2.7e-7   gX0 3.2e-7   gH+gX0 2.6e-7   gW 1.0e-6   gbias 3.0e-7
  cin_pool   pooled 1.6e-7   gA 5.2e-8          rows_dot  out 3.6e-6          rows_tdot  out 2.7e-7"""
import numpy as np
import pytest

import interaction_abi as IA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = IA.SENT


def _lib():
    from deepctr_torch._hip import lib as L
    return L.lib()


@pytest.mark.parametrize("kw", [kw for _, kw in IA.CIN_LAYER_CASES], ids=[i for i, _ in IA.CIN_LAYER_CASES])
def test_cin_layer(kw):
    IA.CinLayerCase(_lib(), DEV, **kw).check()


@pytest.mark.parametrize("D", IA.SMALL_D)
@pytest.mark.parametrize("op", ["cin_layer", "cin_pool", "rows_dot", "rows_tdot"])
def test_smallest_shapes_and_padded_rows(op, D):
    for case in IA.smallest(_lib(), DEV, op, D):
        case.check()


def test_cin_layer_beyond_32_fields_is_refused():
    """M = 33: DCTR_ENOSUP in both directions before any launch, every output still the sentinel"""
    case = IA.CinLayerCase(_lib(), DEV, 2, 2, 33, 4, 5, pad=1)
    assert case.forward() == IA.ENOSUP
    assert case.sentinel_everywhere(case.fwd_out)
    assert case.backward() == IA.ENOSUP
    assert case.sentinel_everywhere(case.bwd_out)


def test_cin_layer_empty_batch():
    """B = 0 on valid one-row buffers: the forward touches nothing, the backward zeroes gW and gbias and nothing else"""
    case = IA.CinLayerCase(_lib(), DEV, 1, 2, 3, 4, 5, pad=1)
    case.nB = 0
    assert case.forward() == 0
    assert case.sentinel_everywhere(case.fwd_out)
    assert case.backward() == 0
    for name, buf in case.bwd_out.items():
        if name in ("gW", "gbias"):
            assert float(np.abs(buf.get()).max()) == 0.0, name
            assert buf.untouched(), name
        else:
            assert case.sentinel_everywhere({name: buf}), name


@pytest.mark.parametrize("name", ["a", "h", "x0", "gh", "gx"])
def test_cin_layer_bwd_refuses_a_short_leading_dimension(name):
    """dctr_cin_layer_bwd used to validate no leading dimension (the forward did): DCTR_EINVAL before any launch now"""
    case = IA.CinLayerCase(_lib(), DEV, 2, 2, 3, 4, 5, pad=1)
    case.force_ld[name] = {"a": 5 * 4, "h": 2 * 4, "x0": 3 * 4, "gh": 2 * 4, "gx": 3 * 4}[name] - 1
    if name in ("a", "h", "x0"):
        assert case.forward() == IA.EINVAL
        assert case.sentinel_everywhere(case.fwd_out)
    assert case.backward() == IA.EINVAL
    assert case.sentinel_everywhere(case.bwd_out)


# ---- the pooling glue ------------------------------------------------------------------------------------------------------
POSITIONS = {"split": dict(n_hidden=3, pool_from=3), "non-split": dict(n_hidden=6, pool_from=0),
             "last": dict(n_hidden=0, pool_from=0)}


@pytest.mark.parametrize("pos", sorted(POSITIONS))
@pytest.mark.parametrize("D", [1, 3, 4, 6, 16])
def test_cin_pool_widths_and_layer_positions(D, pos):
    """D % 4 == 0 takes k_cin_pool_bwd4 (and the forward's float4 loads), the others the scalar kernels; ld_pooled and ld_gp
    padded; with and without w_head"""
    for w_head in (False, True):
        IA.CinPoolCase(_lib(), DEV, 5, 6, D, w_head=w_head, pad=3, **POSITIONS[pos]).check()


def test_cin_pool_misaligned_g_hidden_takes_the_scalar_kernel():
    """g_hidden one float off a 16-byte boundary at D = 4: k_cin_pool_bwd instead of k_cin_pool_bwd4"""
    IA.CinPoolCase(_lib(), DEV, 5, 6, 4, 3, 3, lead=1, pad=3).check()
    IA.CinPoolCase(_lib(), DEV, 5, 6, 4, 6, 0, lead=1, w_head=True).check()


@pytest.mark.parametrize("relu", [True, False])
def test_cin_pool_absent_operands(relu):
    """A_relu NULL / present x g_pooled NULL (the hidden rows' gradient alone; at the last layer nothing at all: the
    reference is identically zero and gA must be exactly zero)"""
    IA.CinPoolCase(_lib(), DEV, 5, 6, 4, 3, 3, relu=relu, pooled_grad=False, pad=3).check()
    IA.CinPoolCase(_lib(), DEV, 5, 6, 3, 0, 0, relu=relu, pooled_grad=False).check()
    IA.CinPoolCase(_lib(), DEV, 5, 6, 3, 3, 3, relu=relu, w_head=True, pad=1).check()


@pytest.mark.parametrize("B,O,D", [(5, 17, 3), (4, 4, 16), (1, 257, 1), (5, 205, 1), (41, 5, 5)])
def test_cin_pool_sizes_around_a_workgroup(B, O, D):
    """B * O * D = 255, 256, 257, 1025, 1025: the last workgroup of 256 threads full, one element over, four workgroups + 1"""
    nh = O // 2
    IA.CinPoolCase(_lib(), DEV, B, O, D, nh, nh, pad=1).check()
    IA.CinPoolCase(_lib(), DEV, B, O, D, O, 0, w_head=True).check()


# ---- the two row products --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 192, 257])
def test_rows_dot(N):
    """one wave per row, four rows per workgroup: B = 1, 3, 4, 5; N below, at and above the 64 lanes; ld_x padded"""
    for B in (1, 3, 4, 5):
        IA.RowsDotCase(_lib(), DEV, B, N, pad=3 if B != 4 else 0).check()


@pytest.mark.parametrize("N", [1, 15, 16, 17, 192, 257])
def test_rows_tdot(N):
    """rows in groups of 32 (B = 1, 31, 32, 33, 65: one partial, one full, full + partial, two full + one row), the groups'
    sums added in group order from a guarded workspace that held 777, then NaN: identical bits"""
    for B in (1, 31, 32, 33, 65):
        IA.RowsTdotCase(_lib(), DEV, B, N, pad=3 if B != 32 else 0).check()


def test_zz_report():
    IA.report()
