"""k_mlp_wgrad's XCD-local (slice, tile) assignment (csrc/wgrad_assign.hpp), through the C ABI.

The weight-gradient launch deals its GEMM workgroups to (batch slice, 64x64 tile) pairs by a remap of the workgroup id; every
pair writes its own partial of the split-batch workspace and k_mlp_reduce sums the slices.  A pair that no workgroup takes
leaves its partial unwritten, a pair taken twice leaves another's unwritten: the workspace is filled with NaN before the
call, so either shows in the gradients.  ``dctr_mlp_train_wgrad`` reads the activations ``h`` and the backward's ``dh`` as
they lie in memory, so the test hands it random ones and the checker is the plain product in float64:

    gW[l] = dh[l]^T in[l],   gbias[l] = sum_b dh[l],   g_w_out = g_logit^T h[top],   loss = sum of the head's partials

at the tolerance tests/test_gpu_mlp.py holds the same quantities to (1e-5 x max(1, max|reference|): fp32 re-association
only, the MFMA f32 instructions are exact fmaf chains).  A tower without ``w_out`` has no such entry point: it goes
through ``dctr_mlp_bwd``, whose backward-data launch writes ``dh`` first; the product is then taken with the ``dh`` read back.

Shapes: fewer than 8 GEMM workgroups (the map is the identity), a workgroup count that is no multiple of 8 over two layers,
the Criteo tower (252 GEMM + 4 projection workgroups), no projection workgroups, a ragged last slice."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import max_abs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


def _r4(n):
    return (n + 3) // 4 * 4


def _close(tag, got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), "%s: %d non-finite values (an unwritten partial)" % (tag, (~np.isfinite(got)).sum())
    scale = max(1.0, float(np.max(np.abs(ref))))
    err = max_abs(got, ref)
    print("%s: max|d| = %.3e, bound %.3e" % (tag, err, TOL * scale))
    assert err <= TOL * scale, "%s: max|d| = %.3e (scale %.3e)" % (tag, err, scale)


class _Tower:
    def __init__(self, B, K, hidden, proj, seed=0):
        from deepctr_torch._hip import lib as L
        g = torch.Generator().manual_seed(seed)
        self.B, self.K, self.hidden, self.proj = B, K, hidden, proj
        self.ldx = _r4(K) + 4
        self.x = torch.randn(B, self.ldx, generator=g).to(DEV)
        self.W, self.h, self.dh, self.gW, self.gb = [], [], [], [], []
        Kin = K
        for N in hidden:
            self.W.append((torch.randn(N, _r4(Kin), generator=g) * 0.05).to(DEV))
            self.h.append(torch.randn(B, _r4(N), generator=g).to(DEV))
            self.dh.append((torch.randn(B, _r4(N), generator=g) * 0.1).to(DEV))
            self.gW.append(torch.full((N, _r4(Kin)), float("nan"), device=DEV))
            self.gb.append(torch.full((N,), float("nan"), device=DEV))
            Kin = N
        self.bias = [torch.zeros(N, device=DEV) for N in hidden]
        self.w_out = (torch.randn(hidden[-1], generator=g) * 0.05).to(DEV)
        self.g_w_out = torch.full((hidden[-1],), float("nan"), device=DEV)
        self.g_logit = (torch.randn(B, generator=g) * 0.1).to(DEV)
        d = L.Mlp()
        d.n_layers = len(hidden)
        Kin = K
        for l, N in enumerate(hidden):
            e = d.layer[l]
            e.W, e.bias, e.h, e.dh = self.W[l].data_ptr(), self.bias[l].data_ptr(), self.h[l].data_ptr(), self.dh[l].data_ptr()
            e.gW, e.gbias = self.gW[l].data_ptr(), self.gb[l].data_ptr()
            e.K, e.N, e.ld_w, e.ld_h, e.relu = Kin, N, _r4(Kin), _r4(N), 1
            Kin = N
        if proj:
            d.w_out, d.g_w_out = self.w_out.data_ptr(), self.g_w_out.data_ptr()
        self.desc = d

    def run(self):
        """one weight-gradient call on a NaN-filled workspace -> dict of the gradients (numpy)"""
        from deepctr_torch._hip import lib as L
        lib = L.lib()
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        s = L.stream_handle(torch.device(DEV))
        B = self.B
        n_slab = lib.dctr_mlp_bwd_workspace_floats(ctypes.byref(self.desc), B)
        assert n_slab > 0
        out = {}
        if self.proj:
            n_ws = lib.dctr_mlp_train_workspace_floats(ctypes.byref(self.desc), B)
            n_head = (n_ws - n_slab) // 2
            ws = torch.full((n_ws,), float("nan"), device=DEV)
            # the head's per-row-tile partials (loss | d bias), which the train launch leaves behind the slabs
            head = torch.arange(1, 2 * n_head + 1, device=DEV, dtype=torch.float32) / 64
            ws[n_slab:] = head
            loss, g_bias = torch.full((), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
            L.check(lib.dctr_mlp_train_wgrad(ctypes.byref(self.desc), p(self.x), self.ldx, B, p(self.g_logit), p(ws), p(loss),
                                             p(g_bias), None, s), "dctr_mlp_train_wgrad")
            torch.cuda.synchronize()
            out["loss"], out["g_bias"] = loss.cpu().numpy(), g_bias.cpu().numpy()
            out["loss_ref"] = head[:n_head].double().sum().item()
            out["g_bias_ref"] = head[n_head:].double().sum().item()
            out["g_w_out"] = self.g_w_out.cpu().numpy()
        else:
            ws = torch.full((n_slab,), float("nan"), device=DEV)
            g = self.dh[-1].clone()          # d loss / d h_top
            L.check(lib.dctr_mlp_bwd(ctypes.byref(self.desc), p(self.x), self.ldx, B, p(g), g.stride(0), None, 0, p(ws), s),
                    "dctr_mlp_bwd")
            torch.cuda.synchronize()
        for l in range(len(self.hidden)):
            out["gW%d" % l], out["gb%d" % l] = self.gW[l].cpu().numpy(), self.gb[l].cpu().numpy()
        return out

    def reference(self):
        """the float64 products of the operands as they lie in memory now"""
        ref = {}
        inp = self.x.cpu().numpy().astype(np.float64)[:, :self.K]
        for l, N in enumerate(self.hidden):
            dh = self.dh[l].cpu().numpy().astype(np.float64)[:, :N]
            gW = np.zeros(tuple(self.gW[l].shape))
            gW[:, :inp.shape[1]] = dh.T @ inp                    # (padding columns of a row receive 0)
            ref["gW%d" % l], ref["gb%d" % l] = gW, dh.sum(0)
            inp = self.h[l].cpu().numpy().astype(np.float64)[:, :N]
        if self.proj:
            ref["g_w_out"] = self.g_logit.cpu().numpy().astype(np.float64) @ inp
        return ref


CASES = [  # B, K, hidden, projection, GEMM workgroups (tiles x slices) the launch must have
    (64, 40, (48,), True, 1),               # one tile, S = 1: fewer than 8 GEMM workgroups, the map is the identity
    (1024, 39, (256, 128), True, 192),      # two layers, 12 tiles x 16 slices
    (832, 39, (256, 128), True, 156),       # ... x 13 slices: no multiple of 8, the groups' runs differ in length
    (4096, 429, (256, 128), True, 252),     # the Criteo tower: 36 tiles x 7 slices (+ 4 projection workgroups)
    (1024, 40, (130, 64), False, 96),       # no w_out: no projection workgroups
    (1000, 39, (256, 128), True, 180),      # ragged batch: 15 slices of 72 rows, the 14th short, the last one empty
]


def _gemm_workgroups(t):
    """tiles x slices, from the workspace size the library reports (slices = workspace / one slab of partials)"""
    from deepctr_torch._hip import lib as L
    slab = tiles = 0
    Kin = t.K
    for N in t.hidden:
        slab += N * _r4(Kin) + _r4(N)
        tiles += ((N + 63) // 64) * ((Kin + 63) // 64)
        Kin = N
    if t.proj:
        slab += _r4(t.hidden[-1])
    n = L.lib().dctr_mlp_bwd_workspace_floats(ctypes.byref(t.desc), t.B)
    assert n % slab == 0
    return tiles * (n // slab)


@pytest.mark.parametrize("B,K,hidden,proj,n_wg", CASES)
def test_every_partial_written_once_and_gradients_match_float64(B, K, hidden, proj, n_wg):
    t = _Tower(B, K, hidden, proj)
    assert _gemm_workgroups(t) == n_wg, "the case no longer has the workgroup count it was chosen for"
    got = t.run()
    ref = t.reference()
    for k, v in ref.items():
        _close(k, got[k], v)
    if proj:
        _close("loss", got["loss"], got["loss_ref"])
        _close("g_bias", got["g_bias"], got["g_bias_ref"])
    # the same call again: the same bits (fixed-order sums, whatever workgroup computed a partial)
    again = t.run()
    for k in ref:
        assert np.array_equal(got[k], again[k]), "%s differs between two calls" % k
