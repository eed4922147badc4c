"""Stand-ins for what DIEN adds to the C ABI (CPU tests only; see tests/mock_lib.py): ``dctr_gru_seq_fwd / _bwd``, the
support and the workspace query, computed in numpy (float64 inside) from the formulas include/dctr.h documents, on the
very ctypes arguments the product code passes: segment addressing, device lengths, the packed parameter vector.

``extend(mock)`` attaches them to the object the ``mock`` fixture returns."""
import numpy as np

from mock_lib import _arr

EINVAL, ENOSUP = -1, -2
GRU, AIGRU, AGRU, AUGRU = 0, 1, 2, 3


def n_params(H):
    return 6 * H * H + 6 * H


def unpack(p, H):
    """packed vector -> (W_ih [3H, H], W_hh [3H, H], b_ih [3H], b_hh [3H]); views"""
    a, b = 3 * H * H, 6 * H * H
    return p[:a].reshape(3 * H, H), p[a:b].reshape(3 * H, H), p[b:b + 3 * H], p[b + 3 * H:]


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def clamp(lens, T):
    return np.clip(np.asarray(lens, np.int64), 0, T)


def forward(x, att, lens, params, mode):
    """x [B, T, H], att [B, T] | None, lens [B] -> (states [B, T, H], last [B, H], cache), float64"""
    x, params = np.asarray(x, np.float64), np.asarray(params, np.float64)
    B, T, H = x.shape
    Wi, Wh, bi, bh = unpack(params, H)
    n = clamp(lens, T)
    a = np.asarray(att, np.float64) if att is not None else np.ones((B, T))
    states, h = np.zeros((B, T, H)), np.zeros((B, H))
    cache = []
    for t in range(T):
        on = (t < n)[:, None]
        xt = x[:, t] * a[:, t:t + 1] if mode == AIGRU else x[:, t]
        gi, gh = xt @ Wi.T + bi, h @ Wh.T + bh
        r, z = _sig(gi[:, :H] + gh[:, :H]), _sig(gi[:, H:2 * H] + gh[:, H:2 * H])
        hn = gh[:, 2 * H:]
        c = np.tanh(gi[:, 2 * H:] + r * hn)
        if mode in (GRU, AIGRU):
            new = (1 - z) * c + z * h
        else:
            u = a[:, t:t + 1] if mode == AGRU else a[:, t:t + 1] * z
            new = (1 - u) * h + u * c
        cache.append((xt, h, r, z, c, hn))
        h = np.where(on, new, h)
        states[:, t] = np.where(on, new, 0.0)
    return states, h, cache


def backward(x, att, lens, params, mode, g_states, g_last):
    """-> (gx [B, T, H], g_att [B, T], g_params), float64; zeros at t >= n"""
    x, params = np.asarray(x, np.float64), np.asarray(params, np.float64)
    B, T, H = x.shape
    Wi, Wh, _, _ = unpack(params, H)
    n = clamp(lens, T)
    a = np.asarray(att, np.float64) if att is not None else np.ones((B, T))
    _, _, cache = forward(x, att, lens, params, mode)
    gp = np.zeros_like(params)
    gWi, gWh, gbi, gbh = unpack(gp, H)
    gx, ga, dh = np.zeros((B, T, H)), np.zeros((B, T)), np.zeros((B, H))
    for t in range(T - 1, -1, -1):
        on = (t < n)[:, None]
        xt, hp, r, z, c, hn = cache[t]
        d = dh.copy()
        if g_states is not None:
            d = d + np.asarray(g_states, np.float64)[:, t]
        if g_last is not None:
            d = d + np.where((t == n - 1)[:, None], np.asarray(g_last, np.float64), 0.0)
        d = np.where(on, d, 0.0)
        at = a[:, t:t + 1]
        if mode in (GRU, AIGRU):
            dc, dz, dhd, da = d * (1 - z), d * (hp - c), d * z, 0.0
        elif mode == AGRU:
            dc, dz, dhd, da = d * at, 0.0 * d, d * (1 - at), (d * (c - hp)).sum(1)
        else:
            du = d * (c - hp)
            dc, dz, dhd, da = d * at * z, du * at, d * (1 - at * z), (du * z).sum(1)
        dpc = dc * (1 - c * c)
        dgi = np.concatenate([dpc * hn * r * (1 - r), dz * z * (1 - z), dpc], axis=1)
        dgh = np.concatenate([dgi[:, :2 * H], dpc * r], axis=1)
        gWi += dgi.T @ xt
        gWh += dgh.T @ hp
        gbi += dgi.sum(0)
        gbh += dgh.sum(0)
        dx = dgi @ Wi
        if mode == AIGRU:
            ga[:, t] = (dx * x[:, t]).sum(1)
            dx = dx * at
        else:
            ga[:, t] = da
        gx[:, t] = dx
        dh = np.where(on, dhd + dgh @ Wh, dh)
    return gx, ga, gp


def supported(T, dims, mode):
    return 1 <= T <= 128 and 1 <= len(dims) <= 4 and sum(dims) <= 64 and 0 <= mode <= 3


def _view(ptr, ld, B, T, dims, offs, steps):
    ext = max(o + (T - 1) * st + d for o, d, st in zip(offs, dims, steps))
    assert ld >= ext
    return _arr(ptr, (B, ext), ld)


def _read(rows, T, dims, offs, steps):
    return np.concatenate([np.stack([rows[:, o + t * st:o + t * st + d] for t in range(T)], axis=1)
                           for o, d, st in zip(offs, dims, steps)], axis=-1)


def _write(rows, value, T, dims, offs, steps):
    e = 0
    for o, d, st in zip(offs, dims, steps):
        for t in range(T):
            rows[:, o + t * st:o + t * st + d] = value[:, t, e:e + d]
        e += d


def extend(mock):
    def dctr_gru_seq_supported(T, n_seg, dim, mode):
        return int(supported(T, [int(dim[j]) for j in range(n_seg)], mode))

    def dctr_gru_seq_bwd_workspace_floats(B, H):
        return 16

    def _args(B, T, n_seg, dim, x_off, x_step, length, att, mode):
        dims = [int(dim[j]) for j in range(n_seg)]
        xo, xs = ([int(a[j]) for j in range(n_seg)] for a in (x_off, x_step))
        lens = _arr(length, (B,), dtype=np.int32)
        av = _arr(att, (B, T))
        assert lens is not None
        return dims, xo, xs, lens, (av if mode != GRU else None)

    def dctr_gru_seq_fwd(X, ld_x, B, T, n_seg, dim, x_off, x_step, length, att, mode, params, states, ld_states, last,
                         ld_last, gates, stream):
        mock.calls.append("gru_fwd:%d:%d" % (mode, 0 if _arr(gates, (1,)) is None else 1))
        if B == 0:
            return 0
        if not supported(T, [int(dim[j]) for j in range(n_seg)], mode):
            return ENOSUP
        dims, xo, xs, lens, av = _args(B, T, n_seg, dim, x_off, x_step, length, att, mode)
        if mode != GRU and av is None:
            return EINVAL
        H = sum(dims)
        x = _read(_view(X, ld_x, B, T, dims, xo, xs), T, dims, xo, xs)
        st, la, _ = forward(x, av, lens, _arr(params, (n_params(H),)), mode)
        sv, lv = _arr(states, (B, T * H), ld_states), _arr(last, (B, H), ld_last)
        assert sv is not None or lv is not None
        if sv is not None:
            assert ld_states >= T * H
            sv[:] = st.reshape(B, T * H)
        if lv is not None:
            lv[:] = la
        return 0

    def dctr_gru_seq_bwd(X, ld_x, B, T, n_seg, dim, x_off, x_step, length, att, mode, params, states, ld_states, gates,
                         g_states, ld_gstates, g_last, ld_glast, gX, ld_gx, g_att, g_params, ws, stream):
        mock.calls.append("gru_bwd:%d" % mode)
        H = sum(int(dim[j]) for j in range(n_seg))
        if B == 0:
            _arr(g_params, (n_params(H),))[:] = 0
            return 0
        if not supported(T, [int(dim[j]) for j in range(n_seg)], mode):
            return ENOSUP
        dims, xo, xs, lens, av = _args(B, T, n_seg, dim, x_off, x_step, length, att, mode)
        assert _arr(ws, (1,)) is not None and _arr(states, (1,)) is not None and _arr(gates, (1,)) is not None
        x = _read(_view(X, ld_x, B, T, dims, xo, xs), T, dims, xo, xs)
        gs, gl = _arr(g_states, (B, T * H), ld_gstates), _arr(g_last, (B, H), ld_glast)
        assert gs is not None or gl is not None
        gx, ga, gp = backward(x, av, lens, _arr(params, (n_params(H),)), mode,
                              gs.reshape(B, T, H) if gs is not None else None, gl)
        _write(_view(gX, ld_gx, B, T, dims, xo, xs), gx, T, dims, xo, xs)
        if mode != GRU:
            _arr(g_att, (B, T))[:] = ga
        _arr(g_params, (gp.size,))[:] = gp
        return 0

    mock.dctr_gru_seq_supported = dctr_gru_seq_supported
    mock.dctr_gru_seq_bwd_workspace_floats = dctr_gru_seq_bwd_workspace_floats
    mock.dctr_gru_seq_fwd = dctr_gru_seq_fwd
    mock.dctr_gru_seq_bwd = dctr_gru_seq_bwd
    return mock
