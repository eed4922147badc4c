"""Stand-ins for what CCPM adds to the C ABI (CPU tests only; see tests/mock_lib.py): ``dctr_ccpm_fwd / _bwd`` and the
workspace query, computed in numpy (float64 inside) from the formulas include/dctr.h documents, on the very ctypes arguments
the product code passes.  The tie rule is the kernel's: equal values of a column keep their field order (a stable sort of the
negated activations).  The backward routes by the ``sel`` bytes it is handed, as the kernel does.

``extend(mock)`` attaches them to the object the ``mock`` fixture returns."""
import numpy as np

from mock_lib import _arr

ENOSUP = -2


def unpack(params, widths, filters):
    """packed vector -> [(W [C, Cin, w], bias [C])] per layer"""
    out, off, cin = [], 0, 1
    for w, c in zip(widths, filters):
        W = params[off:off + c * cin * w].reshape(c, cin, w)
        off += c * cin * w
        out.append((W, params[off:off + c]))
        off += c
        cin = c
    assert off == params.size
    return out


def _pad(x, w):
    top = (w - 1) // 2
    return np.pad(x, ((0, 0), (0, 0), (top, w - 1 - top), (0, 0)))


def forward(E, params, widths, filters, ks, sel=None):
    """E [B, F, D] -> (out [B, C_L, k_L, D], [sel_i [B, C_i, k_i, D]], [(padded input, pooled output)] per layer), float64.
    With ``sel`` (a list like the one returned) the pooling takes those rows instead of choosing."""
    x = np.asarray(E, np.float64)[:, None]
    sels, cache = [], []
    for i, ((W, b), w, k) in enumerate(zip(unpack(np.asarray(params, np.float64), widths, filters), widths, ks)):
        n = x.shape[2]
        xp = _pad(x, w)
        a = b[None, :, None, None] + sum(np.einsum("oc,bcfd->bofd", W[:, :, t], xp[:, :, t:t + n]) for t in range(w))
        y = np.tanh(a)
        order = np.argsort(-y, axis=2, kind="stable")[:, :, :k] if sel is None else np.asarray(sel[i], np.int64)
        out = np.take_along_axis(y, order, 2)
        sels.append(order)
        cache.append((xp, out))
        x = out
    return x, sels, cache


def backward(E, params, widths, filters, ks, sel, gout):
    """-> (gE [B, F, D], g_params packed), float64: the gradient of ``forward(..., sel)`` for d loss / d out = gout"""
    params = np.asarray(params, np.float64)
    _, sels, cache = forward(E, params, widths, filters, ks, sel)
    layers = unpack(params, widths, filters)
    g = np.asarray(gout, np.float64)
    gp = [None] * len(layers)
    for i in range(len(layers) - 1, -1, -1):
        (W, _), w, (xp, out) = layers[i], widths[i], cache[i]
        n = xp.shape[2] - (w - 1)
        top = (w - 1) // 2
        ga = np.zeros((g.shape[0], W.shape[0], n, g.shape[3]))
        np.put_along_axis(ga, sels[i], g * (1.0 - out * out), 2)
        gW = np.stack([np.einsum("bofd,bcfd->oc", ga, xp[:, :, t:t + n]) for t in range(w)], axis=2)
        gxp = np.zeros_like(xp)
        for t in range(w):
            gxp[:, :, t:t + n] += np.einsum("oc,bofd->bcfd", W[:, :, t], ga)
        gp[i] = np.concatenate([gW.reshape(-1), ga.sum((0, 2, 3))])
        g = gxp[:, :, top:top + n]
    return g[:, 0], np.concatenate(gp)


def fits(F, D, widths, filters, ks):
    """the envelope include/dctr.h states"""
    L = len(filters)
    if L > 4 or F > 64 or D > 64 or any(c > 16 for c in filters) or any(w > 16 for w in widths):
        return False
    C, n = [1] + list(filters), [F] + list(ks)
    n_params = sum(C[i] * C[i - 1] * widths[i - 1] + C[i] for i in range(1, L + 1))
    img = [C[i] * n[i] * D for i in range(L + 1)]
    act = max(C[i] * n[i - 1] * D for i in range(1, L + 1))
    return 4 * (n_params + max(img) + act) <= 65536 and \
        4 * (2 * n_params + sum(img) + 2 * max(img)) + (sum(img[1:]) + 3) // 4 * 4 <= 65536


def _spec(n_layers, width, filters, k):
    return [int(width[i]) for i in range(n_layers)], [int(filters[i]) for i in range(n_layers)], \
        [int(k[i]) for i in range(n_layers)]


def _sel_split(flat, B, filters, ks, D):
    out, off = [], 0
    for c, k in zip(filters, ks):
        out.append(flat[:, off:off + c * k * D].reshape(B, c, k, D))
        off += c * k * D
    return out


def extend(mock):
    def dctr_ccpm_bwd_workspace_floats(B, n_params):
        return 16

    def dctr_ccpm_fwd(E, ld_e, B, F, D, n_layers, width, filters, k, params, out, ld_out, sel, stream):
        mock.calls.append("ccpm_fwd:%d" % (0 if _arr(sel, (1,), dtype=np.uint8) is None else 1))
        if B == 0:
            return 0
        if n_layers > 4:
            return ENOSUP
        widths, filt, ks = _spec(n_layers, width, filters, k)
        if not fits(F, D, widths, filt, ks):
            return ENOSUP
        n_params = sum(c * ci * w + c for c, ci, w in zip(filt, [1] + filt[:-1], widths))
        n_out = filt[-1] * ks[-1] * D
        assert ld_e >= F * D and ld_out >= n_out
        y, sels, _ = forward(_arr(E, (B, F * D), ld_e).reshape(B, F, D), _arr(params, (n_params,)), widths, filt, ks)
        _arr(out, (B, n_out), ld_out)[:] = y.reshape(B, n_out)
        n_sel = sum(c * kk for c, kk in zip(filt, ks)) * D
        sv = _arr(sel, (B * n_sel,), dtype=np.uint8)
        if sv is not None:
            sv[:] = np.concatenate([s.reshape(B, -1) for s in sels], axis=1).reshape(-1)
        return 0

    def dctr_ccpm_bwd(E, ld_e, B, F, D, n_layers, width, filters, k, params, sel, g_out, ld_gout, gE, ld_ge, g_params, ws,
                      stream):
        mock.calls.append("ccpm_bwd")
        widths, filt, ks = _spec(n_layers, width, filters, k)
        n_params = sum(c * ci * w + c for c, ci, w in zip(filt, [1] + filt[:-1], widths))
        if B == 0:
            _arr(g_params, (n_params,))[:] = 0
            return 0
        if not fits(F, D, widths, filt, ks):
            return ENOSUP
        n_out = filt[-1] * ks[-1] * D
        n_sel = sum(c * kk for c, kk in zip(filt, ks)) * D
        assert ld_e >= F * D and ld_gout >= n_out and ld_ge >= F * D and _arr(ws, (1,)) is not None
        sv = _sel_split(_arr(sel, (B * n_sel,), dtype=np.uint8).reshape(B, n_sel), B, filt, ks, D)
        ge, gp = backward(_arr(E, (B, F * D), ld_e).reshape(B, F, D), _arr(params, (n_params,)), widths, filt, ks, sv,
                          _arr(g_out, (B, n_out), ld_gout).reshape(B, filt[-1], ks[-1], D))
        _arr(gE, (B, F * D), ld_ge)[:] = ge.reshape(B, F * D)
        _arr(g_params, (n_params,))[:] = gp
        return 0

    mock.dctr_ccpm_bwd_workspace_floats = dctr_ccpm_bwd_workspace_floats
    mock.dctr_ccpm_fwd = dctr_ccpm_fwd
    mock.dctr_ccpm_bwd = dctr_ccpm_bwd
    return mock
