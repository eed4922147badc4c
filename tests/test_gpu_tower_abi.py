"""GPU: the DNN tower and its fused train step (csrc/mlp.hip, csrc/tower_tiles.hpp) through the C ABI against float64.
tests/tower_abi.py is the driver and holds the case list (``case_list()``; tests/test_tower_abi_host.py runs the same list
over the stand-in on the CPU): ``dctr_mlp_t`` built by hand, every operand in one sentinel-guarded arena with padded leading
dimensions (777 in the pad columns of x and W), parameters / gradients / Adagrad state in three flat slabs, a workspace of
exactly the advertised size with NaN inside, a float64 statement of include/dctr.h's contract beside the same statement in
plain float32.  Tower outputs and gradients within 1e-5 x max(1, max|ref|), y_pred 1e-6, g_logit 2e-6, loss 1e-5 x
max(1, |ref|), parameters and Adagrad state after the in-kernel step over max|ref| within max(4 x plain float32's deviation,
4 ulps); every float the header does not say is written keeps its bits.

Every geometry runs ``-fwd-bwd`` (dctr_mlp_fwd + dctr_mlp_bwd, with and without w_out, the backward twice: same bits),
``-train`` (dctr_mlp_train_step with step = NULL, defer_wgrad = 0 and again: same bits; defer_wgrad = 1 +
dctr_mlp_train_wgrad: y_pred, g_logit, gx, h, dh compared behind the first call, and the same bits as the direct route in
the whole arena behind the second), ``-sgd`` / ``-adagrad`` (three successive steps by both routes: the same bits); the
groups marked (t, a) run ``-train`` and ``-adagrad`` only.  What each group reaches -- ``fast`` (tower_fast), ``kc``
(pick_kc) and ``bwd_off`` as dctr_mlp_train_step computes them, restated in ``tower_abi.launch_arm`` and asserted per case:
  fast1-keep    B 64, 429 -> (256, 128): fast = 1 (mlp_fwd_fast + mlp_bwd_fast_q<4>), lds_f 61 952 + lds_b 33 792 <= 150 KB:
                bwd_off > 0, the top layers' relu masks come from the forward's LDS tiles.  The arm of every model test; first.
  fast2-keep    B 37 and B 1, 13 -> (8,): fast = 2 (mlp_bwd_fast_q<2>, 32-column groups), bwd_off > 0.
  fast1-alias   B 37, 500 -> (512, 64): fast = 1, lds_f 99 840 + lds_b 66 560 > 150 KB: bwd_off = 0 -- the backward's gradient
                tiles alias the forward's image, hb0 / hb1 = nullptr, every relu mask comes back from global memory.
  fast0-keep    B 50, 754 -> (64, 32, 16): K0p 768 > kc 512: fast = 0, mlp_fwd_body stages the input in two chunks and hands
                its top tile to mlp_bwd_body (htop != nullptr).
  fast0-alias   B 70, 429 -> (1024, 512, 256): kc = 256, fast = 0, bwd_off = 0 (htop = nullptr);  B 40, 1100 -> (1152, 64):
                kc = 64, lds_f = 153 088 bytes, 512 under the limit.  dctr_mlp_bwd alone takes its own value of fast
                (tower_fast(m, 512)): 0 for both, a layer is wider than 512.
  rows (t, a)   B 15, 16, 17, 33 at 13 -> (8,): the clamped row index ``hbc`` of a ragged last tile, group_sum<16> over a partly
                empty tile, the tile partials of loss and g_bias in k_mlp_reduce's extra workgroup.
  layers12      DCTR_MLP_MAX_LAYERS layers of widths 8 .. 24 at B 20.     identity   18 -> 10 -> 7 with relu = 0, B 33.
  bias-null / gW-null / gx-null (t, a)   a layer with bias = NULL (its gbias slot keeps the sentinel: launch_wgrad_reduce
                passes no destination, and the step leaves its parameter slot alone), a layer with gW = NULL (its W is not
                stepped), gx = NULL (the layer-0 pass of the backward is skipped).
  gx-pad (t, a) K = 32 and 64: gx's pad columns behind the last column group stay as they were.
  x-pad-nan (t, a)   NaN in x's columns [K, ld_x) through mlp_fwd_fast's staging, mlp_fwd_body's chunked staging and
                k_mlp_wgrad's column pairs: nothing of it reaches a result (include/dctr.h says so since this file).
  head (t, a)   part0 / part1 both, either, neither (absent parts borrow y's address), head bias = NULL, g_bias = NULL; the
                saturated rows (+40 | y = 1 on every risky row, -40 | y = 0 on one other) are in every train case.
  adagrad-eps0.1   eps large enough that sqrt(s) + eps and sqrt(s + eps) differ.
  split-batch   B 200, 39 -> (256, 128): plan_wgrad gives S = 3 slices of 72, 72, 56 rows (read back from the advertised
                workspace size), through the train step by both routes and with both optimizers.
  empty-batch   B = 0: DCTR_OK from all four entry points, the arena untouched.

Largest max|d| / scale observed on an MI355X over all cases of this file (kernel | plain float32 numpy at the same cases);
h .. g_bias over max(1, max|ref|) (y_pred, g_logit: absolute), parameters and state over max|ref|:
  h         1.3e-6 | 9.7e-7      logit    9.9e-7 | 6.0e-7      y_pred   3.3e-7 | 2.1e-7      g_logit  3.3e-7 | 2.1e-7
  dh        1.9e-7 | 2.1e-7      gx       3.0e-7 | 2.2e-7      gW       8.2e-7 | 5.8e-7      gbias    3.3e-7 | 3.5e-7
  g_w_out   1.1e-6 | 1.8e-6      loss     1.6e-7 | 1.6e-7      g_bias   1.4e-6 | 1.2e-6
  param W   1.2e-7 | 1.2e-7      bias     1.3e-7 | 1.3e-7      w_out    1.3e-7 | 2.3e-7      head bias  1.1e-7 | 1.1e-7
  state W   1.5e-7 | 2.6e-7      bias     1.1e-7 | 1.8e-7      w_out    1.4e-7 | 4.1e-7      head bias  3.3e-7 | 2.4e-7
The kernels lose what plain float32 loses: the MFMA chains sum in another order than the host's BLAS, nothing more.  Both
routes through the weight gradients leave the same bits everywhere, as the code says (one launch_wgrad_reduce, the same
arguments); nothing was relaxed.  The arms no test had run (fast = 0 inside k_mlp_train, bwd_off = 0 with either fast) pass
as they are: no defect was found in csrc/mlp.hip or csrc/tower_tiles.hpp, and no kernel was changed.  With Adagrad's state
seeded by the floor alone (no gradient history: ``TowerCase._seed_state``) the 12-layer case's state sat at 4.83e-7 of max|s|
against the 4-ulp floor of 4.77e-7 -- a gradient 2 ulps off float64 after 24 matrix products, squared into a state made of
nothing else; the state is seeded as tests/lazy_abi.py seeds its own since."""
import pytest

import tower_abi as TA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = TA.case_list()


def _lib():
    from deepctr_torch._hip import lib as L
    return L.lib()


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_case(name):
    """one case of ``tower_abi.case_list()``; the established arm (fast 1, the forward's image kept) comes first"""
    dict(CASES)[name](_lib(), DEV)


@pytest.fixture(scope="module", autouse=True)
def largest_ratios():
    """behind the module's last test: prints (``-s``) the module docstring's table over whatever cases ran; every entry was
    asserted against its bound where it was measured"""
    yield
    for kind, (ratio, ratio32) in sorted(TA.WORST.items()):
        print("WORST %-16s kernel %.2e   float32 %.2e" % (kind, ratio, ratio32))
