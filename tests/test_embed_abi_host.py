"""CPU: the C-ABI driver of the fused lookup and the sorted update (tests/embed_abi.py) over the stand-in library.  The
driver's float64 model is written from include/dctr.h and torch.optim, the stand-in's gather and update (tests/mock_lib.py)
from the kernels: two independent statements of the contract, held against each other on the very case list the device runs
(tests/test_gpu_embed_abi.py), with the same bounds -- integer outputs exact, the forward's copies bit for bit, every float
outside what the header says is written bit-identical (pad columns, guard bands, untouched rows, input buffers), refusals
that write nothing, floating-point results over max|ref| of the tensor.

The bounds (embed_abi.TOL) are the starting bounds of tests/interaction_abi.py -- OUT_TOL = 1e-5 for the forward's wide / fm /
fm_s, GRAD_TOL = 2e-5 for table / state / gacc / g_wdense / Linear.weight and its state.  A starting bound is kept only where
plain float32 numpy (``ref32``: the same statement as the float64 model, a row's duplicates summed once in sample order and
once in reverse) stays within a quarter of it at every case of the list; where it does not, the bound is four times the
largest deviation of ``ref32`` over the list (embed_abi.WIDENED) -- never anything a kernel returned.
``test_float32_stays_within_a_quarter_of_every_bound`` asserts both.  Largest max|ref32 - ref| / max|ref| over the list, per
(entry point, tensor), and the bound that follows:

    fwd     wide      3.588e-7   1e-5         update  g_wdense  7.437e-7   2e-5         bwd    table  2.054e-7   2e-5
    fwd     fm        2.236e-6   1e-5         update  wdense_w  7.946e-7   2e-5         bwd    gacc   2.102e-7   2e-5
    fwd     fm_s      1.871e-7   1e-5         update  wdense_s  1.523e-6   2e-5         apply  table  9.157e-8   2e-5
    update  table     1.763e-5   7.06e-5      update  state     9.170e-6   3.67e-5      apply  state  8.283e-8   2e-5
    update  gacc      5.145e-6   2.06e-5
  general units (pooled fields, shared tables):
    fwd-pooled  out   4.209e-7   1e-5         update-general  table  8.251e-6   3.305e-5      bwd-pooled    gacc   2.754e-7   2e-5
    fwd-pooled  wide  2.993e-7   1e-5         update-general  state  5.564e-6   2.23e-5      apply-pooled  table  7.360e-8   2e-5
    fwd-pooled  fm    2.010e-6   1e-5         update-general  gacc   3.091e-6   2e-5         apply-pooled  state  7.056e-8   2e-5
    fwd-pooled  fm_s  3.963e-7   1e-5

Five bounds are widened, all of dctr_embed_update: table, state and gacc of simple units pass a quarter of 2e-5 in the cases
that put 520 to 655 entries on one row (update-skew-*, update-routes-*-B16384), table and state of general units in
update-general-dim*-hot (about 2000 entries of a pooled history on one row), where float32 adds them one at a time.

The cases can fail: eighteen stand-ins with one seeded fault each make a named case raise (``FAULTS``).  Faults are seeded
in the stand-in only; nothing here touches a kernel or a device."""
import numpy as np
import pytest

import embed_abi as EA
import mock_iafm
from mock_lib import _arr, _nul

DEV = "cpu"
CASES = EA.case_list()
RAN = set()


@pytest.fixture()
def lib(mock):
    """the stand-in with the per-field-wide entry points of tests/mock_iafm.py on it"""
    return mock_iafm.extend(mock)


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_case_over_the_stand_in(lib, name):
    dict(CASES)[name](lib, DEV)
    RAN.add(name)


def test_case_ids_are_unique():
    """both files look a case up by its id: a repeated id would silently replace a case"""
    names = [n for n, _ in CASES]
    assert len(names) == len(set(names))


def test_float32_stays_within_a_quarter_of_every_bound(lib):
    """the rule that keeps a starting bound (module docstring): over the whole case list -- whatever of it has not run in this
    process yet runs here -- plain float32, in both summation orders, deviates from float64 by at most a quarter of the bound"""
    for name, fn in CASES:
        if name not in RAN:
            fn(lib, DEV)
            RAN.add(name)
    seen = set()
    for (entry, tensor), (_, ratio32) in sorted(EA.WORST.items()):
        print("float32 %-8s %-10s %.3e (bound %.2e)" % (entry, tensor, ratio32, EA.tol(entry, tensor)))
    for (entry, tensor), (_, ratio32) in sorted(EA.WORST.items()):
        assert ratio32 <= EA.tol(entry, tensor) / 4, "%s %s: plain float32 is %.3e off, more than a quarter of the bound %.2e" % (
            entry, tensor, ratio32, EA.tol(entry, tensor))
        if (entry, tensor) in EA.WIDENED:          # a widened bound is four times the measured deviation, not more
            assert EA.WIDENED[(entry, tensor)] <= 4.01 * ratio32 and ratio32 > EA.TOL[tensor] / 4, (entry, tensor, ratio32)
        seen.add(tensor)
    assert seen == set(EA.TOL), "tensors never compared: %s" % sorted(set(EA.TOL) - seen)


# ---- the checks bite -------------------------------------------------------------------------------------------------------
def _fails(lib, name):
    with pytest.raises(AssertionError) as info:
        with np.errstate(all="ignore"):
            dict(CASES)[name](lib, DEV)
    return str(info.value)


def _duplicates_applied_once(lib, mp):
    def bad(rows, G):
        uniq, last = np.unique(rows[::-1], return_index=True)
        return uniq, G[len(rows) - 1 - last].astype(np.float32)
    mp.setattr(lib, "_segment_sums", bad)


def _duplicates_applied_once_general(lib, mp):
    """general units: every row takes the gradient of its first entry only -- the update sees each id once"""
    def change(a):
        x = lib._ext(a["pref"])
        if x is None:
            return
        n = x[0].n_vcols * a["B"]
        ids = _arr(a["ids_t"], (n,), dtype=np.int32).reshape(x[0].n_vcols, a["B"])
        tags = _arr(a["parts_t"], (n,), dtype=np.uint16).reshape(x[0].n_vcols, a["B"])
        a["_tags"] = (tags, tags.copy())
        for vu in x[2]:
            if vu.j:
                continue
            seen = set()
            for c in range(vu.c0, vu.c0 + vu.n_slots):
                for b in range(a["B"]):
                    if tags[c, b] != 0xFFFF:
                        if int(ids[c, b]) in seen:
                            tags[c, b] = 0xFFFF
                        seen.add(int(ids[c, b]))

    def after(a):
        if "_tags" in a:
            a["_tags"][0][...] = a["_tags"][1]
    _wrap_update(lib, mp, change, after)


def _state_by_sum_of_squares(lib, mp):
    def bad(uniq, acc, rows, G):
        out = np.zeros_like(acc)
        np.add.at(out, np.searchsorted(uniq, rows), G * G)
        return out
    mp.setattr(lib, "_state_increment", bad)


def _out_of_range_to_last_row(lib, mp):
    def bad(ids, vocab):
        ids = np.asarray(ids, np.int64)
        return np.where((ids < 0) | (ids >= vocab), vocab - 1, ids)
    mp.setattr(lib, "_clamp_rows", bad)


def _ids_rounded(lib, mp):
    mp.setattr(lib, "_trunc_ids", lambda col: np.rint(col).astype(np.int32))


def _wrap_update(lib, mp, change=None, after=None):
    real = lib.dctr_embed_update
    names = ("pref units n_units max_vocab ids_t parts_t B g_out ld_g out ld_out fm_s ld_s g_fm g_wide ld_gw opt lr eps X ld_x "
             "g_wdense wd_step ws ws_n presorted stream").split()

    def bad(*args):
        a = dict(zip(names, args))
        if change is not None:
            change(a)
        rc = real(*[a[k] for k in names])
        if after is not None and rc == 0 and a["B"] > 0:
            after(a)
        return rc
    mp.setattr(lib, "dctr_embed_update", bad)


def _ld_gw_ignored(lib, mp):
    def change(a):
        if a["pref"] is not None and not a["pref"]._obj.flags & 8:
            a["ld_gw"] = 1
    _wrap_update(lib, mp, change)


def _ld_s_ignored(lib, mp):
    def change(a):
        if a["pref"] is not None and a["pref"]._obj.emb_dim > 0:
            a["ld_s"] = a["pref"]._obj.emb_dim
    _wrap_update(lib, mp, change)


def _fm_without_e(lib, mp):
    mp.setattr(lib, "_fm_term", lambda gF, S, e: gF[:, None] * S)


def _pad_column_written(lib, mp):
    def after(a):
        c, deep, widef, _, _ = lib._plan(a["pref"])
        for f in deep + widef:
            if f.ld > f.dim:
                _arr(f.table, (f.vocab, f.ld), f.ld)[0, 2 * f.dim] = 1.0          # (the first pad column of row 0's slab row)
                return
    _wrap_update(lib, mp, after=after)


def _whole_out_row_written(lib, mp):
    """the stand-in as it was before this driver: the whole [B, ld_out] row zeroed, padding included"""
    real = lib.dctr_embed_fwd

    def bad(pref, X, ldx, B, out, ld_out, *rest):
        if not _nul(out) and B > 0 and ld_out > 0 and ld_out % 4 == 0:
            _arr(out, (B, ld_out), ld_out)[...] = 0
        return real(pref, X, ldx, B, out, ld_out, *rest)
    mp.setattr(lib, "dctr_embed_fwd", bad)


def _wide_only_unit_skipped(lib, mp):
    mp.setattr(lib, "_unit_sides", lambda di, wi: (di, wi) if di >= 0 else (-1, -1))


def _accum_overwrites(lib, mp):
    def bad(gacc, uniq, acc):
        gacc[uniq] = acc
    mp.setattr(lib, "_accumulate", bad)


def _wdense_step_twice(lib, mp):
    real = lib._dense_step

    def bad(step, gptr, n):
        real(step, gptr, n)
        real(step, gptr, n)
    mp.setattr(lib, "_dense_step", bad)


def _tiny_where_zero(lib, mp):
    real = lib.dctr_embed_fwd

    def bad(pref, X, ldx, B, out, ld_out, wide, ld_wide, fm, *rest):
        rc = real(pref, X, ldx, B, out, ld_out, wide, ld_wide, fm, *rest)
        if rc == 0 and B > 0 and not _nul(fm):
            v = _arr(fm, (B,))
            v[v == 0] = 1e-30
        return rc
    mp.setattr(lib, "dctr_embed_fwd", bad)


def _last_maximum_wins(lib, mp):
    mp.setattr(lib, "_argmax", lambda v: v.shape[1] - 1 - v[:, ::-1].argmax(axis=1))


def _masked_position_is_an_entry(lib, mp):
    mp.setattr(lib, "_entry_valid", lambda valid: np.ones_like(valid))


def _mean_gradient_not_divided(lib, mp):
    """the update reads a divisor of 1 for every mean-pooled field (den_t itself is put back: it is an input)"""
    def change(a):
        x = lib._ext(a["pref"])
        if x is not None and x[0].n_den and x[0].den_t:
            den = _arr(x[0].den_t, (x[0].n_den * a["B"],))
            a["_den"] = (den, den.copy())
            den[...] = 1.0

    def after(a):
        if "_den" in a:
            a["_den"][0][...] = a["_den"][1]
    _wrap_update(lib, mp, change, after)


def _mean_divisor_without_epsilon(lib, mp):
    real = lib.dctr_embed_ids

    def bad(pref, units, n_units, X, ldx, B, ids_t, parts_t, stream):
        rc = real(pref, units, n_units, X, ldx, B, ids_t, parts_t, stream)
        x = lib._ext(pref)
        if rc == 0 and B > 0 and x is not None and x[0].n_den and x[0].den_t:
            den = _arr(x[0].den_t, (x[0].n_den * B,))
            den[den < 0.5] = 0.0
        return rc
    mp.setattr(lib, "dctr_embed_ids", bad)


# (the seeded fault, the case that must reject it, what its message says)
FAULTS = [
    ("max pooling: the last maximum wins", _last_maximum_wins, "lookup-pooled-dim4", r"amax differs from the contract"),
    ("a masked-out position counted as an entry", _masked_position_is_an_entry, "lookup-pooled-dim4",
     r"parts_t differs from the contract"),
    ("mean pooling's gradient not divided by the count", _mean_gradient_not_divided, "update-general-dim4-B17",
     r"table \d+ table: max\|d\|"),
    ("mean pooling's divisor without 1e-8", _mean_divisor_without_epsilon, "lookup-pooled-dim4", r"den_t differs from the contract"),
    ("duplicates of a row applied once, general units", _duplicates_applied_once_general, "update-general-dim4-B17",
     r"table \d+ table: max\|d\|"),
    ("duplicates of a row applied once", _duplicates_applied_once, "update-geometry-dim256-contiguous", r"table: max\|d\|"),
    ("Adagrad state stepped by the sum of squares", _state_by_sum_of_squares, "update-geometry-dim256-contiguous",
     r"adagrad .* (state|table): max\|d\|"),
    ("an out-of-range id sent to row vocab - 1", _out_of_range_to_last_row, "lookup-ids-contiguous",
     r"not the table row|int buffer parts"),
    ("ids rounded to nearest", _ids_rounded, "lookup-ids-contiguous", r"not the table row|int buffer ids|set err"),
    ("ld_gw ignored", _ld_gw_ignored, "update-geometry-dim4-interleaved", r"wide field \d+ table: max\|d\|"),
    ("ld_s ignored", _ld_s_ignored, "update-geometry-dim4-contiguous", r"deep field \d+ table: max\|d\|"),
    ("FM's backward with S instead of S - e", _fm_without_e, "update-geometry-dim4-contiguous", r"deep field \d+ table: max\|d\|"),
    ("a write into a slab's pad column", _pad_column_written, "update-geometry-dim4-interleaved",
     r"floats outside what the call writes changed"),
    ("the whole out row written", _whole_out_row_written, "lookup-vec4-dim4-contiguous",
     r"floats outside what the call writes changed"),
    ("a wide-only unit skipped", _wide_only_unit_skipped, "update-geometry-dim4-contiguous", r"wide field 1 table: max\|d\|"),
    ("ACCUM overwriting instead of adding", _accum_overwrites, "update-geometry-dim4-contiguous", r"accum .* gacc: max\|d\|"),
    ("wdense_step applied twice", _wdense_step_twice, "update-dense-half-1", r"wdense_(w|s): max\|d\|"),
    ("1e-30 where the reference is zero", _tiny_where_zero, "lookup-deep-fields-1", r"fm: nonzero where the reference is identically zero"),
]


@pytest.mark.parametrize("what,seed,case,message", FAULTS, ids=[f[0].replace(" ", "-") for f in FAULTS])
def test_a_seeded_fault_fails_its_case(lib, monkeypatch, what, seed, case, message):
    import re
    seed(lib, monkeypatch)
    msg = _fails(lib, case)
    assert re.search(message, msg), "%s: %s rejected it, but with %r" % (what, case, msg)


def test_the_unpatched_stand_in_passes_what_the_faults_fail(lib):
    for case in sorted(set(f[2] for f in FAULTS)):
        dict(CASES)[case](lib, DEV)
