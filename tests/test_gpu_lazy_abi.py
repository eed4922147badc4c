"""GPU: the lazy table-update kernels (csrc/lazy.hip, csrc/lazy_opt.hpp) through the C ABI against float64.
tests/lazy_abi.py is the driver and holds the case list (``case_list()``; tests/test_lazy_abi_host.py runs the same list over
the stand-in on the CPU): sentinel-guarded arenas, a float64 model of include/dctr.h's contract, stamps compared exactly,
every row the model did not touch in a call bit-identical, weights within tests/test_gpu_lazy.py's bars x max(1, max|ref|)
(1e-4, RMSprop 3e-4, only where rows replay 300 steps: ids-*, long-gaps-*; 2e-5 everywhere else, where no row takes more
than 43 steps), optimizer state relative to max|ref| of the tensor within max(4 x the deviation of plain float32 numpy at
the same case, 4 float32 ulps).

What each group reaches, read off the launcher (``launch<MODE>``) and ``lazy_block``:
  geometry      vec = 1 at dims 1, 3, 5, 64 (lpr 1, 4, 8, 64; ``adam_replay_step<float>``) and vec = 4 at dims 4, 8, 20, 64, 256
                (lpr 1, 2, 8, 16, 64; the packed pairs): lpr = 1 is ``shift == 0`` -- flush and sweep do not split off the wide
                pass; lpr = 64 is one row per wavefront; dims 3, 5, 20 leave trailing lanes with ``e0 >= un.dim``.  Mixed
                launches: units narrower than max_dim, a wide-only unit (deep = NULL) and a deep-only unit (wide = NULL) beside
                full units, vocabularies 1, 3, 50, 300 under one max_vocab.  Contiguous, and table + s1 interleaved in one slab
                with 4 pad floats per row.  Every kind: catch-up of rows 0..8, which carry the gaps 0..8, apply, step_inc,
                flush.
  sgd-lam0.1    SGD has no state to compare, and at lambda = 1e-3 one replayed step (2e-5 |w|) is the size of the short bar:
                a geometry, ids, sweep and long-gaps case each at lambda = 0.1, where one lost or doubled step is 2e-3 |w|.
  refusals      max_dim 65 / 257 -> DCTR_ENOSUP; vec 2, kind 4, K 0, B -1, NULL units / step / opt -> DCTR_EINVAL; B = 0 and
                max_vocab = 0 -> DCTR_OK; nothing written by any of them.
  ids           B = 1, 17, 63, 64, 65, 300 over vocab 300: one id five times, -1 / vocab / 2^31 - 1 (row 0), gaps 0..300;
                ``k_lazy_order`` on exactly from B = 64 (and never for SGD / Adagrad without an L2 term): order_ws a
                permutation per unit or untouched; with and without order_ws the same bits.
  sweep         K = 7 over vocab 50 (last window 2 rows), 3 (windows 3..6 empty) and 1; K = 1; K = 64 over vocab 50
                (wlen 1); K steps of {catch-up, sweep, apply, step_inc} from a step that is no multiple of K: exactly the
                window's rows move, no stamp ends more than K behind.
  adam-scalars  gaps of 12 steps across the end of adam_ss and of adam_bc (betas (0.5, 0.9): 56 / 358 entries, and the
                defaults: 358 / 37 414) and at step 1 000 000; with the three tables, with adam_rbc = NULL (``rcpf(bc)``),
                with no tables (``AdamClock``, chosen by the struct alone); through catch-up, flush and apply (the clamp of
                ``adam_tab``, of ``adam_tab_uniform``, the prefetch of entry T + 1 and the separate ``n_bc`` index of adam_rbc).
                The tables end against a sentinel band: one float too far is 777.
  long-gaps     every kind, 300 steps from step 0 and from step 40; 16 rows of one wavefront with gaps 1, 20, .. 300
                (``replay_in_step`` with most lanes sitting out) through catch-up and through flush.
  routes        40 steps without data gradients: step_inc x 40 + flush | catch-up(17) + sweep(7) per step + flush | catch-up(17)
                per step + flush (order_ws given, the ordering pass off below B = 64) | catch-up(70) with order_ws every fifth
                step + flush (``k_lazy_order`` on) give identical bits in tables, states and stamps, two runs too; and at dims
                (8, 4) vec = 4 and vec = 1 give identical bits -- lazy_opt.hpp's "one lane or a packed pair computes the same
                bits".  On the MI355X all of these hold, for every kind: the comment states the code, nothing was relaxed.
  dense         dctr_dense_opt_reg: every kind, n = 1, 255, 256, 257, 1000, lam NULL / given, three successive steps; Adam
                with tables from *step = n_ss - 1 and n_bc - 1 and with the in-kernel clock; the refusals.

Largest max|d| / scale observed on an MI355X over all cases of this file, per kind (kernel | plain float32 numpy at the same
cases); w over max(1, max|ref|), states over max|ref|:
                 w                     s1                    s2
  sgd            2.9e-6 | 2.9e-6
  adagrad        1.4e-6 | 1.4e-6       1.2e-6 | 1.2e-6
  adam           1.5e-6 | 1.5e-6       1.2e-6 | 1.2e-6       1.7e-6 | 1.7e-6
  rmsprop        1.2e-6 | 1.2e-6       1.8e-6 | 2.1e-6
  dense sgd      1.1e-7 | 1.1e-7
  dense adagrad  8.5e-8 | 8.5e-8       1.4e-7 | 1.4e-7
  dense adam     1.2e-7 | 1.2e-7       1.8e-7 | 1.8e-7       1.6e-7 | 1.6e-7
  dense rmsprop  8.2e-8 | 8.2e-8       1.3e-7 | 1.3e-7
(all maxima come from the 300-step cases.)  The two columns agree to the digits shown because the same roundings dominate
both: a replayed step moves a weight of magnitude 1 by about 1e-3, so the 1.5-ulp reciprocal and root change the step by
3e-10 -- far below the 6e-8 by which storing the weight rounds -- and the moments follow the weight.  Single cases do differ
(Adam's exp_avg_sq after 300 steps: 1.52e-6 against 1.42e-6); none came near four times the float32 deviation.  No defect was
found in csrc/lazy.hip or csrc/lazy_opt.hpp."""
import pytest

import lazy_abi as LA

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = LA.case_list()


def _lib():
    from deepctr_torch._hip import lib as L
    return L.lib()


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_case(name):
    """one case of ``lazy_abi.case_list()``.  The route and vec = 1 / vec = 4 bit-identities (``routes-*``) hold on the MI355X as
    lazy_opt.hpp states them -- the arithmetic does not differ by route, and the comment does not overstate."""
    dict(CASES)[name](_lib(), DEV)


@pytest.fixture(scope="module", autouse=True)
def largest_ratios():
    """behind the module's last test: prints (``-s``) the module docstring's table over whatever cases ran; every entry was
    asserted against its bound where it was measured"""
    yield
    for (kind, k), (ratio, ratio32) in sorted(LA.WORST.items()):
        print("WORST %-16s %-3s kernel %.2e   float32 %.2e" % (kind, k, ratio, ratio32))
