"""Stand-ins for what AFN adds to the C ABI (CPU tests only; see tests/mock_lib.py): ``dctr_log_transform_fwd_train /
_fwd_eval / _bwd`` and the workspace query, in numpy float64 from the formulas include/dctr.h documents, on the very ctypes
arguments the product code passes.  ``forward`` / ``backward`` double as the float64 restatement of the layer that
tests/test_gpu_afn_kernel.py compares the kernels with.

``extend(mock)`` attaches them to the object the ``mock`` fixture returns."""
import ctypes

import numpy as np

from mock_lib import _arr

ENOSUP = -2
CLAMP = float(np.float32(1e-7))
EPS = 1e-5


def fits(F, E, H):
    """the envelope include/dctr.h states"""
    return 1 <= F <= 64 and 1 <= E <= 64 and 1 <= H <= 1024


def forward(X, W, bias, g0, b0, g1, b1, stats=None):
    """X [B, F, E] -> (out [B, E*H], stats [4, E] = mean0, var0, mean1, var1 (biased), cache), float64.  ``stats`` given:
    normalise with those (eval mode) instead of the batch's."""
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    bias, g0, b0, g1, b1 = [np.asarray(v, np.float64).reshape(-1) for v in (bias, g0, b0, g1, b1)]
    B, F, E = X.shape
    a = np.log(np.maximum(np.abs(X), CLAMP)).transpose(0, 2, 1)            # [B, E, F]
    if stats is None:
        m0, v0 = a.mean((0, 2)), a.var((0, 2))
    else:
        m0, v0 = np.asarray(stats[0], np.float64), np.asarray(stats[1], np.float64)
    r0 = 1.0 / np.sqrt(v0 + EPS)
    nhat = (a - m0[None, :, None]) * r0[None, :, None]
    n = nhat * g0[None, :, None] + b0[None, :, None]
    y = np.exp(n @ W + bias[None, None, :])                                # [B, E, H]
    if stats is None:
        m1, v1 = y.mean((0, 2)), y.var((0, 2))
    else:
        m1, v1 = np.asarray(stats[2], np.float64), np.asarray(stats[3], np.float64)
    r1 = 1.0 / np.sqrt(v1 + EPS)
    yhat = (y - m1[None, :, None]) * r1[None, :, None]
    out = yhat * g1[None, :, None] + b1[None, :, None]
    return out.reshape(B, -1), np.stack([m0, v0, m1, v1]), (nhat, n, y, yhat, r0, r1)


def backward(X, W, bias, g0, b0, g1, stats, gout):
    """the gradient of the train-mode forward for d loss / d out = gout [B, E*H] -> dict of float64 arrays"""
    X, W = np.asarray(X, np.float64), np.asarray(W, np.float64)
    g0, g1 = np.asarray(g0, np.float64).reshape(-1), np.asarray(g1, np.float64).reshape(-1)
    B, F, E = X.shape
    H = W.shape[1]
    _, _, (nhat, n, y, yhat, r0, r1) = forward(X, W, bias, g0, b0, g1, np.zeros(E), stats)
    g = np.asarray(gout, np.float64).reshape(B, E, H)
    gb1, gg1 = g.sum((0, 2)), (g * yhat).sum((0, 2))
    N1, N0 = B * H, B * F
    gz = (g1 * r1)[None, :, None] * (g - gb1[None, :, None] / N1 - yhat * gg1[None, :, None] / N1) * y
    gbias = gz.sum((0, 1))
    gW = np.einsum("bef,beh->fh", n, gz)
    gn = gz @ W.T                                                          # [B, E, F]
    gb0, gg0 = gn.sum((0, 2)), (gn * nhat).sum((0, 2))
    ga = (g0 * r0)[None, :, None] * (gn - gb0[None, :, None] / N0 - nhat * gg0[None, :, None] / N0)
    Xt = X.transpose(0, 2, 1)
    gX = np.where(np.abs(Xt) >= CLAMP, ga / np.where(Xt == 0, 1.0, Xt), 0.0).transpose(0, 2, 1)
    return {"gX": gX, "gW": gW, "gbias": gbias, "g_bn0_w": gg0, "g_bn0_b": gb0, "g_bn1_w": gg1, "g_bn1_b": gb1}


def _f64(ptr, n):
    addr = ptr.value if isinstance(ptr, ctypes.c_void_p) else int(ptr)
    return np.ctypeslib.as_array((ctypes.c_double * n).from_address(addr))


def extend(mock):
    def dctr_log_transform_workspace_floats(B, F, E, H):
        return 16

    def _common(X, ld_e, B, F, E, H, W, bias):
        assert ld_e >= F * E
        return (_arr(X, (B, F * E), ld_e).reshape(B, F, E), _arr(W, (F * H,)).reshape(F, H), _arr(bias, (H,)))

    def dctr_log_transform_fwd_train(X, ld_e, B, F, E, H, W, bias, g0, b0, g1, b1, out, ld_out, stats, ws, stream):
        mock.calls.append("log_transform_fwd_train")
        if not fits(F, E, H):
            return ENOSUP
        if B == 0:
            return 0
        assert ld_out >= E * H and _arr(ws, (1,)) is not None
        Xv, Wv, bv = _common(X, ld_e, B, F, E, H, W, bias)
        o, st, _ = forward(Xv, Wv, bv, *[_arr(p, (E,)) for p in (g0, b0, g1, b1)])
        _arr(out, (B, E * H), ld_out)[:] = o
        _f64(stats, 4 * E)[:] = st.reshape(-1)
        return 0

    def dctr_log_transform_fwd_eval(X, ld_e, B, F, E, H, W, bias, g0, b0, m0, v0, g1, b1, m1, v1, out, ld_out, stream):
        mock.calls.append("log_transform_fwd_eval")
        if not fits(F, E, H):
            return ENOSUP
        if B == 0:
            return 0
        assert ld_out >= E * H
        Xv, Wv, bv = _common(X, ld_e, B, F, E, H, W, bias)
        o, _, _ = forward(Xv, Wv, bv, *[_arr(p, (E,)) for p in (g0, b0, g1, b1)],
                          stats=[_arr(p, (E,)) for p in (m0, v0, m1, v1)])
        _arr(out, (B, E * H), ld_out)[:] = o
        return 0

    def dctr_log_transform_bwd(X, ld_e, B, F, E, H, W, bias, g0, b0, g1, stats, g_out, ld_g, gX, ld_gx, gW, gbias, gg0, gb0,
                               gg1, gb1, ws, stream):
        mock.calls.append("log_transform_bwd")
        if not fits(F, E, H):
            return ENOSUP
        if B == 0:
            for p, n in ((gW, F * H), (gbias, H), (gg0, E), (gb0, E), (gg1, E), (gb1, E)):
                _arr(p, (n,))[:] = 0
            return 0
        assert ld_g >= E * H and ld_gx >= F * E and _arr(ws, (1,)) is not None
        Xv, Wv, bv = _common(X, ld_e, B, F, E, H, W, bias)
        r = backward(Xv, Wv, bv, _arr(g0, (E,)), _arr(b0, (E,)), _arr(g1, (E,)), _f64(stats, 4 * E).reshape(4, E),
                     _arr(g_out, (B, E * H), ld_g))
        _arr(gX, (B, F * E), ld_gx)[:] = r["gX"].reshape(B, F * E)
        _arr(gW, (F * H,))[:] = r["gW"].reshape(-1)
        _arr(gbias, (H,))[:] = r["gbias"]
        for p, k in ((gg0, "g_bn0_w"), (gb0, "g_bn0_b"), (gg1, "g_bn1_w"), (gb1, "g_bn1_b")):
            _arr(p, (E,))[:] = r[k]
        return 0

    mock.dctr_log_transform_workspace_floats = dctr_log_transform_workspace_floats
    mock.dctr_log_transform_fwd_train = dctr_log_transform_fwd_train
    mock.dctr_log_transform_fwd_eval = dctr_log_transform_fwd_eval
    mock.dctr_log_transform_bwd = dctr_log_transform_bwd
    return mock
