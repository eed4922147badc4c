"""Stand-ins for what DIN adds to the C ABI (CPU tests only; see tests/mock_lib.py): ``dctr_din_attn_fwd / _bwd``, the
support and the workspace query, computed in numpy (float64 inside) from the formulas include/dctr.h documents, on the very
ctypes arguments the product code passes: segment addressing, lengths or mask, the packed parameter vector.

``extend(mock)`` attaches them to the object the ``mock`` fixture returns."""
import numpy as np

from mock_lib import _arr

EINVAL, ENOSUP = -1, -2
ACTS = ["linear", "relu", "sigmoid", "prelu", "dice"]
PAD = float(-2 ** 32 + 1)


def n_params(E, hidden, act):
    n, inn = 0, 4 * E
    for H in hidden:
        n += H * inn + H + (1 if act == "prelu" else 3 * H if act == "dice" else 0)
        inn = H
    return n + inn + 1


def unpack(params, E, hidden, act):
    """packed vector -> ([(W [H, in], b [H], extra)], dense w [H_L], dense b [1]); views, so a packed gradient can be
    filled through them"""
    out, off, inn = [], 0, 4 * E
    for H in hidden:
        W = params[off:off + H * inn].reshape(H, inn)
        off += H * inn
        b = params[off:off + H]
        off += H
        ne = 1 if act == "prelu" else 3 * H if act == "dice" else 0
        out.append((W, b, params[off:off + ne]))
        off += ne
        inn = H
    assert off + inn + 1 == params.size
    return out, params[off:off + inn], params[off + inn:]


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _act(act, z, extra):
    if act == "relu":
        return np.maximum(z, 0.0)
    if act == "sigmoid":
        return _sig(z)
    if act == "prelu":
        return np.where(z > 0, z, extra[0] * z)
    if act == "dice":
        H = z.shape[-1]
        al, s, t = extra[:H], extra[H:2 * H], extra[2 * H:]
        return z * (al + (1.0 - al) * _sig(s * z + t))
    return z


def forward(q, k, valid, params, hidden, act, softmax):
    """q [B, E], k [B, T, E], valid [B, T] bool -> (out [B, E], w [B, T], cache), float64"""
    q, k, params = np.asarray(q, np.float64), np.asarray(k, np.float64), np.asarray(params, np.float64)
    layers, wd, bd = unpack(params, q.shape[1], hidden, act)
    qq = np.broadcast_to(q[:, None, :], k.shape)
    a = np.concatenate([qq, k, qq - k, qq * k], axis=-1)
    zs, acts = [], [a]
    for W, b, extra in layers:
        z = a @ W.T + b
        a = _act(act, z, extra)
        zs.append(z)
        acts.append(a)
    s = a @ wd + bd[0]
    if softmax:
        sm = np.where(valid, s, PAD)
        e = np.exp(sm - sm.max(axis=1, keepdims=True))
        w = e / e.sum(axis=1, keepdims=True)
    else:
        w = np.where(valid, s, 0.0)
    return np.einsum("bt,bte->be", w, k), w, (q, k, zs, acts)


def backward(q, k, valid, params, hidden, act, softmax, gout):
    """-> (gq [B, E], gk [B, T, E], g_params packed), float64"""
    params = np.asarray(params, np.float64)
    _, w, (q, k, zs, acts) = forward(q, k, valid, params, hidden, act, softmax)
    E = q.shape[1]
    layers, wd, _ = unpack(params, E, hidden, act)
    gp = np.zeros_like(params)
    glayers, gwd, gbd = unpack(gp, E, hidden, act)
    g = np.asarray(gout, np.float64)
    gk = w[:, :, None] * g[:, None, :]
    dw = np.einsum("be,bte->bt", g, k)
    ds = w * (dw - (w * dw).sum(axis=1, keepdims=True)) if softmax else dw
    ds = np.where(valid, ds, 0.0)
    gwd[:] = np.einsum("bt,bth->h", ds, acts[-1])
    gbd[:] = ds.sum()
    dA = ds[:, :, None] * wd
    for l in range(len(layers) - 1, -1, -1):
        W, _, extra = layers[l]
        z, a = zs[l], acts[l + 1]
        if act == "relu":
            dz = dA * (z > 0)
        elif act == "sigmoid":
            dz = dA * a * (1.0 - a)
        elif act == "prelu":
            dz = dA * np.where(z > 0, 1.0, extra[0])
            glayers[l][2][:] = (dA * np.where(z > 0, 0.0, z)).sum()
        else:
            dz = dA
        glayers[l][0][:] = np.einsum("bth,bti->hi", dz, acts[l])
        glayers[l][1][:] = dz.sum(axis=(0, 1))
        dA = dz @ W
    d0, d1, d2, d3 = dA[..., :E], dA[..., E:2 * E], dA[..., 2 * E:3 * E], dA[..., 3 * E:]
    gq = (d0 + d2 + d3 * k).sum(axis=1)
    gk = gk + d1 - d2 + d3 * q[:, None, :]
    return gq, gk, gp


def supported(T, dims, hidden, act):
    return 1 <= T <= 128 and 1 <= len(dims) <= 4 and sum(dims) <= 64 and 1 <= len(hidden) <= 3 and \
        all(1 <= h <= 128 for h in hidden) and 0 <= act <= 4


def _read(ptr, ld, B, T, dims, offs, steps):
    """the segments of [B, ld] rows as [B, T, E] (T = 1, steps = None for a query)"""
    ext = max(o + (T - 1) * (st if steps is not None else 0) + d
              for o, d, st in zip(offs, dims, steps if steps is not None else [0] * len(dims)))
    assert ld >= ext
    rows = _arr(ptr, (B, ext), ld)
    parts = []
    for j, (o, d) in enumerate(zip(offs, dims)):
        st = steps[j] if steps is not None else 0
        parts.append(np.stack([rows[:, o + t * st:o + t * st + d] for t in range(T)], axis=1))
    return np.concatenate(parts, axis=-1), rows


def _write(rows, value, T, dims, offs, steps):
    e = 0
    for j, (o, d) in enumerate(zip(offs, dims)):
        st = steps[j] if steps is not None else 0
        for t in range(T):
            rows[:, o + t * st:o + t * st + d] = value[:, t, e:e + d]
        e += d


def _common(B, T, n_seg, dim, q_off, k_off, k_step, length, mask, n_layers, hidden):
    dims = [int(dim[j]) for j in range(n_seg)]
    qo, ko, ks = ([int(a[j]) for j in range(n_seg)] for a in (q_off, k_off, k_step))
    hid = [int(hidden[i]) for i in range(n_layers)]
    lv, mv = _arr(length, (B,), dtype=np.int32), _arr(mask, (B * T,), dtype=np.uint8)
    assert (lv is None) != (mv is None)
    valid = (np.arange(T)[None, :] < lv[:, None]) if lv is not None else mv.reshape(B, T) != 0
    return dims, qo, ko, ks, hid, valid


def extend(mock):
    def dctr_din_attn_supported(T, n_seg, dim, n_layers, hidden, act):
        return int(supported(T, [int(dim[j]) for j in range(n_seg)], [int(hidden[i]) for i in range(n_layers)], act))

    def dctr_din_attn_bwd_workspace_floats(B, n):
        return 16

    def dctr_din_attn_fwd(Q, ld_q, K, ld_k, B, T, n_seg, dim, q_off, k_off, k_step, length, mask, n_layers, hidden, act,
                          softmax, params, out, ld_out, weights, stream):
        mock.calls.append("din_fwd:%d" % (0 if _arr(weights, (1,)) is None else 1))
        if B == 0:
            return 0
        if not supported(T, [int(dim[j]) for j in range(n_seg)], [int(hidden[i]) for i in range(n_layers)], act):
            return ENOSUP
        dims, qo, ko, ks, hid, valid = _common(B, T, n_seg, dim, q_off, k_off, k_step, length, mask, n_layers, hidden)
        E = sum(dims)
        q, _ = _read(Q, ld_q, B, 1, dims, qo, None)
        k, _ = _read(K, ld_k, B, T, dims, ko, ks)
        p = _arr(params, (n_params(E, hid, ACTS[act]),))
        y, w, _ = forward(q[:, 0], k, valid, p, hid, ACTS[act], softmax)
        assert ld_out >= E
        _arr(out, (B, E), ld_out)[:] = y
        wv = _arr(weights, (B, T))
        if wv is not None:
            wv[:] = w
        return 0

    def dctr_din_attn_bwd(Q, ld_q, K, ld_k, B, T, n_seg, dim, q_off, k_off, k_step, length, mask, n_layers, hidden, act,
                          softmax, params, weights, g_out, ld_gout, gQ, ld_gq, gK, ld_gk, g_params, ws, stream):
        mock.calls.append("din_bwd")
        hid = [int(hidden[i]) for i in range(n_layers)]
        E = sum(int(dim[j]) for j in range(n_seg))
        if B == 0:
            _arr(g_params, (n_params(E, hid, ACTS[act]),))[:] = 0
            return 0
        if not supported(T, [int(dim[j]) for j in range(n_seg)], hid, act) or ACTS[act] == "dice":
            return ENOSUP
        dims, qo, ko, ks, hid, valid = _common(B, T, n_seg, dim, q_off, k_off, k_step, length, mask, n_layers, hidden)
        assert _arr(ws, (1,)) is not None and _arr(weights, (1,)) is not None and ld_gout >= E
        q, _ = _read(Q, ld_q, B, 1, dims, qo, None)
        k, _ = _read(K, ld_k, B, T, dims, ko, ks)
        p = _arr(params, (n_params(E, hid, ACTS[act]),))
        gq, gk, gp = backward(q[:, 0], k, valid, p, hid, ACTS[act], softmax, _arr(g_out, (B, E), ld_gout))
        _, qrows = _read(gQ, ld_gq, B, 1, dims, qo, None)
        _write(qrows, gq[:, None, :], 1, dims, qo, None)
        _, krows = _read(gK, ld_gk, B, T, dims, ko, ks)
        _write(krows, gk, T, dims, ko, ks)
        _arr(g_params, (p.size,))[:] = gp
        return 0

    mock.dctr_din_attn_supported = dctr_din_attn_supported
    mock.dctr_din_attn_bwd_workspace_floats = dctr_din_attn_bwd_workspace_floats
    mock.dctr_din_attn_fwd = dctr_din_attn_fwd
    mock.dctr_din_attn_bwd = dctr_din_attn_bwd
    return mock
