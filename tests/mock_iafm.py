"""Stand-ins for what the input-aware FM models add to the C ABI (CPU tests only; see tests/mock_lib.py):

* ``dctr_iafm_fwd / _bwd``: the forward restates the formula include/dctr.h documents, in torch on the caller's host
  buffers; the backward is torch.autograd of that forward (as tests/mock_ops.py does) -- an independent check of the
  marshalling in deepctr_torch/_hip/ops/fm.py, not a second copy of the kernel's hand-derived gradients;
* ``dctr_embed_fwd / _update / _bwd`` for plans with DCTR_PLAN_WIDE_PER_FIELD: the deep side is left to the stand-in's own
  entry points (called without a wide buffer), the wide side is served per field here.  Plans without the bit go to the
  originals untouched.

``extend(mock)`` attaches them to the object the ``mock`` fixture returns."""
import ctypes

import numpy as np
import torch

from mock_lib import _arr, _tab, _st
from mock_ops import _grads, _t, _v

WIDE_PER_FIELD = 8
IAFM_SOFTMAX = 0


def _null(p):
    return p is None or not (p.value if isinstance(p, ctypes.c_void_p) else int(p))


def iafm_formula(E, Wl, n_wl, Z1, Z2, mode):
    """(m [B, F], y_lin [B], y_fm [B]) -- include/dctr.h, dctr_iafm_fwd."""
    B, F, D = E.shape
    m = F * torch.softmax(Z1, dim=1) if mode == IAFM_SOFTMAX else Z1 + Z2
    y_lin = torch.zeros(B, dtype=E.dtype)
    if Wl is not None:
        if n_wl:
            y_lin = y_lin + (m * Wl[:, :n_wl]).sum(1)
        y_lin = y_lin + Wl[:, n_wl]
    v = E * m.unsqueeze(-1)
    y_fm = 0.5 * (v.sum(1).pow(2) - v.pow(2).sum(1)).sum(1)
    return m, y_lin, y_fm


def extend(mock):
    orig_fwd, orig_update, orig_bwd = mock.dctr_embed_fwd, mock.dctr_embed_update, mock.dctr_embed_bwd

    def per_field(pref):
        return pref is not None and bool(pref._obj.flags & WIDE_PER_FIELD)

    # ---- the kernel pair -------------------------------------------------------------------------------------------
    def dctr_iafm_supported(F, D):
        return 1

    def dctr_iafm_fwd(E, ld_e, Wl, ld_w, n_wl, Z1, ld_z1, Z2, ld_z2, mode, B, F, D, m, ld_m, y_lin, y_fm, stream):
        mock.calls.append("iafm_fwd")
        assert ld_e >= F * D and (_null(Wl) or (n_wl in (0, F) and ld_w >= n_wl + 1))
        e = _t(E, B, F * D, ld_e).reshape(B, F, D)
        wl = None if _null(Wl) else _t(Wl, B, n_wl + 1, ld_w)
        z2 = None if _null(Z2) else _t(Z2, B, F, ld_z2)
        mm, yl, yf = iafm_formula(e, wl, n_wl, _t(Z1, B, F, ld_z1), z2, mode)
        _t(m, B, F, ld_m).copy_(mm)
        _v(y_lin, B).copy_(yl)
        _v(y_fm, B).copy_(yf)
        return 0

    def dctr_iafm_bwd(E, ld_e, Wl, ld_w, n_wl, m, ld_m, mode, B, F, D, g_lin, g_fm, gE, ld_ge, gWl, ld_gw, gZ, ld_gz,
                      stream):
        mock.calls.append("iafm_bwd")
        with torch.enable_grad():
            e = _t(E, B, F * D, ld_e).clone().requires_grad_(True)
            wl = None if _null(Wl) else _t(Wl, B, n_wl + 1, ld_w).clone().requires_grad_(True)
            # m is what the forward saved; a Z that reproduces it lets autograd differentiate the documented forward
            mm = _t(m, B, F, ld_m).clone()
            z = (torch.log(mm / F) if mode == IAFM_SOFTMAX else mm).requires_grad_(True)
            z2 = None if mode == IAFM_SOFTMAX else torch.zeros(B, F)
            _, yl, yf = iafm_formula(e.reshape(B, F, D), wl, n_wl, z, z2, mode)
            gl = torch.zeros(B) if _null(g_lin) else _v(g_lin, B)
            gf = torch.zeros(B) if _null(g_fm) else _v(g_fm, B)
            ge, gw, gz = _grads((yl * gl).sum() + (yf * gf).sum(), [e, wl, z], torch.ones(()))
        _t(gE, B, F * D, ld_ge).copy_(ge)
        if not _null(gWl):
            _t(gWl, B, n_wl + 1, ld_gw).copy_(gw)
        _t(gZ, B, F, ld_gz).copy_(gz)
        return 0

    # ---- the gather / update of a per-field-wide plan -----------------------------------------------------------------
    def dctr_embed_fwd(pref, X, ldx, B, out, ld_out, wide, ld_wide, fm, err, units, n_units, ids_t, parts_t, fm_s, ld_s,
                       stream):
        if not per_field(pref):
            return orig_fwd(pref, X, ldx, B, out, ld_out, wide, ld_wide, fm, err, units, n_units, ids_t, parts_t, fm_s,
                            ld_s, stream)
        if not _null(wide) and ld_wide < pref._obj.n_wide + 1:
            return -1          # (DCTR_EINVAL, include/dctr.h)
        rc = orig_fwd(pref, X, ldx, B, out, ld_out, None, 1, fm, err, units, n_units, ids_t, parts_t, fm_s, ld_s, stream)
        if rc or _null(wide) or B == 0:
            return rc
        c, deep, widef, dcols, wcols = mock._plan(pref)
        Xv = _arr(X, (B, c.n_xcols), ldx)
        W = _arr(wide, (B, c.n_wide + 1), ld_wide)
        for f, fd in enumerate(widef):
            W[:, f] = mock._gather(Xv, fd, _arr(err, (1,), dtype=np.int32))[:, 0]
        W[:, c.n_wide] = 0
        if wcols:
            ww = _arr(c.wdense_w, (len(wcols),))
            for j, col in enumerate(wcols):
                W[:, c.n_wide] += Xv[:, col] * ww[j]
        return 0

    def wide_rows(c, widef, Xv, gW):
        """per table of the wide side: (a field over it, row ids, gradient rows), the fields sharing it concatenated"""
        by_table = {}
        for f, fd in enumerate(widef):
            rows, g = mock._scatter(Xv, fd, np.ascontiguousarray(gW[:, f:f + 1]).astype(np.float32))
            ent = by_table.setdefault(fd.table, [fd, [], []])
            ent[1].append(np.asarray(rows).reshape(-1))
            ent[2].append(np.asarray(g, np.float32).reshape(-1, 1))
        return [(fd, np.concatenate(r), np.concatenate(g)) for fd, r, g in by_table.values()]

    def dctr_embed_update(pref, units, n_units, max_vocab, ids_t, parts_t, B, g_out, ld_g, out, ld_out, fm_s, ld_s, g_fm,
                          g_wide, ld_gw, opt, lr, eps, X, ld_x, g_wdense, wd_step, ws, ws_n, presorted, stream):
        if not per_field(pref):
            return orig_update(pref, units, n_units, max_vocab, ids_t, parts_t, B, g_out, ld_g, out, ld_out, fm_s, ld_s,
                               g_fm, g_wide, ld_gw, opt, lr, eps, X, ld_x, g_wdense, wd_step, ws, ws_n, presorted, stream)
        c, deep, widef, dcols, wcols = mock._plan(pref)
        work = []
        if not _null(g_wide):
            assert ld_gw >= c.n_wide + 1
            Xv = _arr(X, (B, c.n_xcols), ld_x)
            gW = _arr(g_wide, (B, c.n_wide + 1), ld_gw)
            work = wide_rows(c, widef, Xv, gW)          # (max pooling re-reads the tables: before anything moves)
        rc = orig_update(pref, units, n_units, max_vocab, ids_t, parts_t, B, g_out, ld_g, out, ld_out, fm_s, ld_s, g_fm,
                         None, 1, opt, lr, eps, X, ld_x, None, None, ws, ws_n, presorted, stream)
        if rc or _null(g_wide):
            return rc
        for fd, rows, g in work:
            uniq, inv = np.unique(rows, return_inverse=True)
            acc = np.zeros((len(uniq), 1), np.float32)
            np.add.at(acc, inv.reshape(-1), g)
            table = _tab(fd)
            if opt == 0:
                table[uniq] -= np.float32(lr) * acc
            elif opt == 1:
                st = _st(fd)
                st[uniq] += acc * acc
                table[uniq] -= np.float32(lr) * (acc / (np.sqrt(st[uniq]) + np.float32(eps)))
            else:
                _arr(fd.gacc, (fd.vocab, fd.dim))[uniq] += acc
        if not _null(g_wdense) and wcols:
            gd = gW[:, c.n_wide].astype(np.float64)
            _arr(g_wdense, (len(wcols),))[...] = [np.dot(gd, Xv[:, col]) for col in wcols]
            mock._dense_step(wd_step, g_wdense, len(wcols))
        return 0

    def dctr_embed_bwd(pref, X, ldx, B, g_out, ld_g, out, ld_out, g_fm, g_wide, mode, lr, stream):
        if not per_field(pref):
            return orig_bwd(pref, X, ldx, B, g_out, ld_g, out, ld_out, g_fm, g_wide, mode, lr, stream)
        c, deep, widef, dcols, wcols = mock._plan(pref)
        work = []
        if not _null(g_wide):
            Xv = _arr(X, (B, c.n_xcols), ldx)
            work = wide_rows(c, widef, Xv, _arr(g_wide, (B, c.n_wide + 1), c.n_wide + 1))
        rc = orig_bwd(pref, X, ldx, B, g_out, ld_g, out, ld_out, g_fm, None, mode, lr, stream)
        for fd, rows, g in work:
            dst = _arr(fd.gacc, (fd.vocab, fd.dim)) if mode == 0 else _tab(fd)
            np.add.at(dst, rows, g if mode == 0 else -np.float32(lr) * g)
        return rc

    mock.dctr_iafm_supported = dctr_iafm_supported
    mock.dctr_iafm_fwd = dctr_iafm_fwd
    mock.dctr_iafm_bwd = dctr_iafm_bwd
    mock.dctr_embed_fwd = dctr_embed_fwd
    mock.dctr_embed_update = dctr_embed_update
    mock.dctr_embed_bwd = dctr_embed_bwd
    return mock
