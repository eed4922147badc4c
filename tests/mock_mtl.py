"""Stand-ins for what the multi-task models add to the C ABI (CPU tests only; see tests/mock_lib.py): ``dctr_gate_mix_fwd /
_bwd`` and the two queries, computed in numpy (float64 inside) from the formulas include/dctr.h documents, on the very ctypes
arguments the product code passes: the array of ``dctr_gate_t`` descriptors, the tables of pool pointers and their leading
dimensions.  Includes the envelope, the ``B == 0`` rule and call recording (``gate_mix_fwd:<G>:<keep>``, ``gate_mix_bwd:<G>``).

``extend(mock)`` attaches them to the object the ``mock`` fixture returns."""
import ctypes

import numpy as np

from mock_lib import _arr

OK, EINVAL, ENOSUP = 0, -1, -2
MAX_GATES, MAX_MEMBERS, MAX_POOL, MAX_WIDTH = 8, 16, 32, 1152


def fits(P, dim, ns, Hs):
    """the envelope include/dctr.h states"""
    return 1 <= P <= MAX_POOL and 1 <= len(ns) <= MAX_GATES and 1 <= dim <= MAX_WIDTH and \
        all(1 <= n <= MAX_MEMBERS for n in ns) and all(1 <= H <= MAX_WIDTH for H in Hs)


def softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def forward(xs, h, W, members):
    """one gate: -> (out [B, dim], w [B, n]), float64"""
    w = softmax(np.asarray(h, np.float64) @ np.asarray(W, np.float64).T)
    out = sum(w[:, j:j + 1] * np.asarray(xs[e], np.float64) for j, e in enumerate(members))
    return out, w


def backward(xs, h, W, members, w, gout):
    """one gate: -> ({member: its share of g_x}, g_h, gW), float64"""
    w, gout = np.asarray(w, np.float64), np.asarray(gout, np.float64)
    s = np.stack([(gout * np.asarray(xs[e], np.float64)).sum(1) for e in members], axis=1)
    dz = w * (s - (w * s).sum(1, keepdims=True))
    gx = {}
    for j, e in enumerate(members):
        gx[e] = gx.get(e, 0.0) + w[:, j:j + 1] * gout
    return gx, dz @ np.asarray(W, np.float64), dz.T @ np.asarray(h, np.float64)


def _ptrs(p, n, ctype):
    addr = ctypes.cast(p, ctypes.c_void_p).value
    return list((ctype * n).from_address(addr))


def _gates(gates, G):
    return [gates[g] for g in range(G)]


def _shape_rc(P, dim, gs):
    if P <= 0 or dim <= 0 or not gs or any(q.n <= 0 or q.H <= 0 for q in gs[:MAX_GATES]):
        return EINVAL
    if P > MAX_POOL or len(gs) > MAX_GATES or not fits(P, dim, [q.n for q in gs], [q.H for q in gs]):
        return ENOSUP
    if any(not 0 <= q.member[j] < P for q in gs for j in range(q.n)):
        return EINVAL
    return OK


def extend(mock):
    def dctr_gate_mix_supported(P, dim, G, n, H):
        return 1 if fits(P, dim, [int(n[g]) for g in range(G)], [int(H[g]) for g in range(G)]) else 0

    def dctr_gate_mix_bwd_workspace_floats(B, G, n, ld_w):
        return 16

    def dctr_gate_mix_fwd(x, ld_x, P, dim, B, gates, G, stream):
        gs = _gates(gates, G) if 0 < G <= 64 else []
        mock.calls.append("gate_mix_fwd:%d:%d" % (G, 1 if (gs and gs[0].w) else 0))
        if B == 0:
            return OK
        rc = _shape_rc(P, dim, gs)
        if rc != OK:
            return rc
        lds = _ptrs(ld_x, P, ctypes.c_int64)
        xs = [_arr(p, (B, dim), ld) for p, ld in zip(_ptrs(x, P, ctypes.c_void_p), lds)]
        assert all(ld >= dim for ld in lds)
        results = []
        for q in gs:                      # (all gates first: an output may not alias an input)
            assert q.ld_h >= q.H and q.ld_w >= q.H and q.ld_out >= dim
            m = [q.member[j] for j in range(q.n)]
            results.append(forward(xs, _arr(q.h, (B, q.H), q.ld_h), _arr(q.W, (q.n, q.H), q.ld_w), m))
        for q, (out, w) in zip(gs, results):
            _arr(q.out, (B, dim), q.ld_out)[:] = out
            if q.w:
                _arr(q.w, (B, q.n))[:] = w
        return OK

    def dctr_gate_mix_bwd(x, ld_x, P, dim, B, gates, G, g_x, ld_gx, ws, stream):
        mock.calls.append("gate_mix_bwd:%d" % G)
        if B == 0:
            return OK
        gs = _gates(gates, G) if 0 < G <= 64 else []
        rc = _shape_rc(P, dim, gs)
        if rc != OK:
            return rc
        assert _arr(ws, (1,)) is not None
        xs = [_arr(p, (B, dim), ld) for p, ld in zip(_ptrs(x, P, ctypes.c_void_p), _ptrs(ld_x, P, ctypes.c_int64))]
        total = [np.zeros((B, dim)) for _ in range(P)]
        for q in gs:
            assert q.w and q.g_h and q.gW and q.ld_gh >= q.H
            gh, gW = _arr(q.g_h, (B, q.H), q.ld_gh), _arr(q.gW, (q.n, q.ld_w))
            if not q.g_out:
                gh[:] = 0
                gW[:] = 0
                continue
            assert q.ld_gout >= dim
            m = [q.member[j] for j in range(q.n)]
            gx, g_h, g_W = backward(xs, _arr(q.h, (B, q.H), q.ld_h), _arr(q.W, (q.n, q.H), q.ld_w), m, _arr(q.w, (B, q.n)),
                                    _arr(q.g_out, (B, dim), q.ld_gout))
            for e, v in gx.items():
                total[e] += v
            gh[:] = g_h
            gW[:] = 0
            gW[:, :q.H] = g_W
        for p, ld, v in zip(_ptrs(g_x, P, ctypes.c_void_p), _ptrs(ld_gx, P, ctypes.c_int64), total):
            _arr(p, (B, dim), ld)[:] = v
        return OK

    mock.dctr_gate_mix_supported = dctr_gate_mix_supported
    mock.dctr_gate_mix_bwd_workspace_floats = dctr_gate_mix_bwd_workspace_floats
    mock.dctr_gate_mix_fwd = dctr_gate_mix_fwd
    mock.dctr_gate_mix_bwd = dctr_gate_mix_bwd
    return mock
