"""Stand-ins for what MLR adds to the C ABI (CPU tests only; see tests/mock_lib.py): ``dctr_mlr_supported``,
``dctr_mlr_fwd / _bwd`` and ``dctr_mlr_bwd_workspace_floats``, computed in float32 numpy from the formulas include/dctr.h
documents, on the very ctypes arguments the product code passes.  The plan is per-field-wide, so the gather and the update
of such plans come from tests/mock_iafm.py (the composed route and every table update go through them).

``extend(mock)`` attaches them to the object the ``mock`` fixture returns."""
import ctypes

import numpy as np

import mock_iafm
from mock_lib import _arr, _nul

EINVAL, ENOSUP = -1, -2
WIDE_PER_FIELD = 8
MAX_REGIONS = 16


def refusal(pref, mref):
    """0, DCTR_EINVAL or DCTR_ENOSUP -- csrc/mlr.hip check_mlr"""
    if pref is None or mref is None:
        return EINVAL
    c, m = pref._obj, mref._obj
    if c.n_deep != 0 or c.n_dense != 0 or c.dense_off >= 0 or c.wdense_w or c.out_chunks or not (c.flags & WIDE_PER_FIELD):
        return ENOSUP
    if not 2 <= m.n_regions <= MAX_REGIONS:
        return ENOSUP
    return 0


def heads(mref, n_wide):
    """(R, H, binary, head_of [n_wide], dense cols per head, dense weight arrays per head)"""
    m = mref._obj
    R, H = m.n_regions, m.n_regions + (1 if m.has_bias else 0)
    hof = _arr(ctypes.c_void_p(m.head_of), (n_wide,), dtype=np.int32) if n_wide else np.zeros(0, np.int32)
    off = _arr(ctypes.c_void_p(m.dense_off), (H + 1,), dtype=np.int32)
    assert off[0] == 0 and off[H] == m.n_dense and all(off[h] <= off[h + 1] for h in range(H))
    cols = _arr(ctypes.c_void_p(m.dense_cols), (m.n_dense,), dtype=np.int32) if m.n_dense else np.zeros(0, np.int32)
    wp = (ctypes.c_int64 * H).from_address(m.dense_w) if m.n_dense else [0] * H
    per_cols, per_w = [], []
    for h in range(H):
        n = int(off[h + 1] - off[h])
        per_cols.append([int(c) for c in cols[off[h]:off[h + 1]]])
        per_w.append(_arr(ctypes.c_void_p(wp[h]), (n,)) if n else None)
        assert n == 0 or wp[h], "head %d has dense columns and no weight" % h
    return R, H, m.task == 0, hof, per_cols, per_w


def mixture32(Z, R, has_bias, binary):
    from mlr_helpers import mixture
    return mixture(Z, R, has_bias, binary, dtype=np.float32)


def extend(mock):
    mock_iafm.extend(mock)

    def dctr_mlr_supported(pref, mref):
        return int(refusal(pref, mref) == 0)

    def dctr_mlr_fwd(pref, mref, X, ldx, B, y, z, ld_z, err, ids_t, parts_t, units, n_units, stream):
        mock.calls.append("mlr_fwd")
        rc = refusal(pref, mref)
        if rc:
            return rc
        c, _, widef, _, _ = mock._plan(pref)
        if _nul(X) or B < 0 or ldx < c.n_xcols:
            return EINVAL
        if B == 0:
            return 0
        R, H, binary, hof, dcols, dw = heads(mref, c.n_wide)
        if _nul(y) or _nul(z) or ld_z < H or (not _nul(ids_t) and (_nul(units) or n_units <= 0 or c.ext)) or \
                (not _nul(parts_t) and _nul(ids_t)):
            return EINVAL
        Xv = _arr(X, (B, c.n_xcols), ldx)
        errv = _arr(err, (1,), dtype=np.int32)
        Z = np.zeros((B, H), np.float32)
        for f, fd in enumerate(widef):
            assert 0 <= hof[f] < H and fd.dim == 1
            Z[:, hof[f]] += mock._gather(Xv, fd, errv)[:, 0]
        for h in range(H):
            for j, col in enumerate(dcols[h]):
                Z[:, h] += Xv[:, col] * dw[h][j]
        _arr(z, (B, H), ld_z)[...] = Z
        _arr(y, (B,))[...] = mixture32(Z, R, H > R, binary)[0]
        if not _nul(ids_t):
            mock.dctr_embed_ids(pref, units, n_units, X, ldx, B, ids_t, parts_t, stream)
            mock.calls.pop()
        if c.ext:      # a max-pooled field's arg-max bytes: where the gather puts them (the stand-in's own gather writes them)
            mock.dctr_embed_fwd(pref, X, ldx, B, None, 0, None, 1, None, None, None, 0, None, None, None, 0, stream)
            mock.calls.pop()
        return 0

    def dctr_mlr_bwd_workspace_floats(mref, B):
        return 0 if (mref is None or B <= 0) else (B + 63) // 64 * mref._obj.n_dense

    def dctr_mlr_bwd(pref, mref, X, ldx, B, g_y, z, ld_z, g_wide, ld_gw, g_dense, ws, stream):
        mock.calls.append("mlr_bwd")
        rc = refusal(pref, mref)
        if rc:
            return rc
        c = pref._obj
        if _nul(X) or B < 0 or ldx < c.n_xcols:
            return EINVAL
        if B == 0:
            return 0
        R, H, binary, hof, dcols, dw = heads(mref, c.n_wide)
        n_dense = mref._obj.n_dense
        if _nul(g_y) or _nul(z) or ld_z < H or (c.n_wide and (_nul(g_wide) or ld_gw < c.n_wide + 1)) or \
                (n_dense and (_nul(g_dense) or _nul(ws))):
            return EINVAL
        Xv = _arr(X, (B, c.n_xcols), ldx)
        gz = mixture32(_arr(z, (B, H), ld_z), R, H > R, binary)[1] * _arr(g_y, (B,))[:, None]
        if c.n_wide:
            G = _arr(g_wide, (B, c.n_wide + 1), ld_gw)
            G[:, :c.n_wide] = gz[:, hof]
            G[:, c.n_wide] = 0
        if n_dense:
            flat = [(h, col) for h in range(H) for col in dcols[h]]
            _arr(g_dense, (n_dense,))[...] = [np.dot(gz[:, h].astype(np.float64), Xv[:, col]) for h, col in flat]
        return 0

    mock.dctr_mlr_supported = dctr_mlr_supported
    mock.dctr_mlr_fwd = dctr_mlr_fwd
    mock.dctr_mlr_bwd_workspace_floats = dctr_mlr_bwd_workspace_floats
    mock.dctr_mlr_bwd = dctr_mlr_bwd
    return mock
