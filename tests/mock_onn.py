"""Stand-ins for what ONN adds to the C ABI (CPU tests only; see tests/mock_lib.py): ``dctr_pair_embed_fwd / _bwd``,
computed in numpy from the formulas include/dctr.h documents, on the very ctypes arguments the product code passes.  The
first-order logit is left to the stand-in's own ``dctr_embed_fwd`` (called without an output buffer), as the kernel shares
the gather's device code for it.

``extend(mock)`` attaches them to the object the ``mock`` fixture returns."""
import numpy as np

from mock_lib import _arr, _tab

ENOSUP = -2
WIDE_PER_FIELD = 8


def pair_rows(mock, Xv, deep, p, err=None):
    """(rows of emb1, rows of emb2) of pair p for every sample: [B, D] each; out-of-range ids read row 0."""
    f1, f2 = deep[2 * p], deep[2 * p + 1]
    return _tab(f1)[mock._rows(Xv, f1, err)], _tab(f2)[mock._rows(Xv, f2, err)]


def refused(c, deep):
    return bool(c.out_chunks) or bool(c.flags & WIDE_PER_FIELD) or c.n_deep % 2 == 1 or c.n_deep_fixed != c.n_deep or \
        len(set(f.dim for f in deep)) > 1 or any(f.len != 1 or f.pool != 0 for f in deep)


def extend(mock):
    def dctr_pair_embed_fwd(pref, X, ldx, B, out, ld_out, wide, ld_wide, err, stream):
        mock.calls.append("pair_embed_fwd")
        c, deep, widef, dcols, wcols = mock._plan(pref)
        if refused(c, deep):
            return ENOSUP
        P = c.n_deep // 2
        D = deep[0].dim if deep else 0
        Xv = _arr(X, (B, c.n_xcols), ldx)
        errv = _arr(err, (1,), dtype=np.int32)
        if P or dcols:
            assert ld_out >= P * D + len(dcols) and (not dcols or c.dense_off == P * D)
            O = _arr(out, (B, ld_out), ld_out)
            for p in range(P):
                assert deep[2 * p].out_off == 2 * p * D and deep[2 * p + 1].out_off == (2 * p + 1) * D
                a, b = pair_rows(mock, Xv, deep, p, errv)
                O[:, p * D:(p + 1) * D] = a * b
            for j, col in enumerate(dcols):
                O[:, c.dense_off + j] = Xv[:, col]
        if _arr(wide, (1,)) is not None:
            rc = mock.dctr_embed_fwd(pref, X, ldx, B, None, ld_out, wide, ld_wide, None, err, None, 0, None, None, None,
                                     0, stream)
            mock.calls.pop()          # (not a launch of its own: the kernel computes the logit itself)
            return rc
        return 0

    def dctr_pair_embed_bwd(pref, X, ldx, B, g_out, ld_g, g_rows, ld_rows, stream):
        mock.calls.append("pair_embed_bwd")
        c, deep, widef, dcols, wcols = mock._plan(pref)
        if refused(c, deep):
            return ENOSUP
        P = c.n_deep // 2
        if not P:
            return 0
        D = deep[0].dim
        assert ld_g >= P * D and ld_rows >= 2 * P * D
        Xv = _arr(X, (B, c.n_xcols), ldx)
        G = _arr(g_out, (B, ld_g), ld_g)
        R = _arr(g_rows, (B, ld_rows), ld_rows)
        for p in range(P):
            a, b = pair_rows(mock, Xv, deep, p)
            g = G[:, p * D:(p + 1) * D]
            o1, o2 = deep[2 * p].out_off, deep[2 * p + 1].out_off
            R[:, o1:o1 + D] = g * b
            R[:, o2:o2 + D] = g * a
        return 0

    mock.dctr_pair_embed_fwd = dctr_pair_embed_fwd
    mock.dctr_pair_embed_bwd = dctr_pair_embed_bwd
    return mock
