"""CPU: the C-ABI driver of the lazy table update (tests/lazy_abi.py) over the stand-in library.  The driver's float64 model
is written from include/dctr.h and torch.optim, the stand-in's ``_lazy_pass`` (tests/mock_lib.py) from the kernel: two
independent statements of the contract, held against each other on the very case list the device runs
(tests/test_gpu_lazy_abi.py), with the same bounds -- stamps exact, untouched rows bit-identical, sentinels intact, refusals
that write nothing, order_ws written exactly when the header says so.  The stand-in is plain float32 numpy, so the state
bound (4 x what plain float32 loses, at least 4 ulps) is met by construction of the case, not by luck.

The cases can fail: four stand-ins with one seeded fault each -- the sweep's window shifted by one row, duplicates applied
twice, adam_ss clamped with n_bc, the catch-up replaying steps prev .. t-1 instead of prev+1 .. t -- make the list raise.
Faults are seeded in the stand-in only; nothing here touches a kernel or a device."""
import ctypes

import numpy as np
import pytest

import lazy_abi as LA
from mock_lib import _arr

DEV = "cpu"
CASES = LA.case_list()


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_case_over_the_stand_in(mock, name):
    dict(CASES)[name](mock, DEV)


def test_case_ids_are_unique():
    """both files look a case up by its id: a repeated id would silently replace a case"""
    names = [n for n, _ in CASES]
    assert len(names) == len(set(names))


def test_the_models_are_independent_of_the_tables(mock):
    """the float64 model takes Adam's scalars from the formulas: with a table entry changed the stand-in moves, the model
    does not, and the case fails"""
    c = LA.LazyCase(mock, DEV, "adam", [(6, 4, True, True, LA.LAM, LA.LAM)], t=20, gaps=[12])
    c.fa[c.tab[0] + 15] *= 2.0          # adam_ss[T - 1] at T = 16
    with pytest.raises(AssertionError, match=r"adam flush unit 0 (deep|wide) (w|s1|s2): max\|d\|"):
        c.flush()


# ---- the checks bite -------------------------------------------------------------------------------------------------------
def _fails(mock, names):
    """the named cases, run to the first that raises"""
    fns = dict(CASES)
    with pytest.raises(AssertionError) as info:
        with np.errstate(all="ignore"):
            for n in names:
                fns[n](mock, DEV)
    return str(info.value)


def _all_names(*prefixes):
    return [n for n, _ in CASES if n.startswith(prefixes)]


def test_a_sweep_window_shifted_by_one_row_fails(mock, monkeypatch):
    real = mock._sweep_rows

    def bad(t, K, vocab):
        rows = real(t, K, vocab) + 1
        return rows[rows < vocab]
    monkeypatch.setattr(mock, "_sweep_rows", bad)
    msg = _fails(mock, _all_names("sweep-"))
    assert "stamp of unit" in msg or "moved" in msg, msg


def _apply_duplicates_twice(mock, monkeypatch):
    from deepctr_torch._hip import lib as L
    real = mock.dctr_lazy_apply

    def bad(units, n_units, ids_t, B, step, opt, vec, max_dim, stream):
        rc = real(units, n_units, ids_t, B, step, opt, vec, max_dim, stream)
        if rc or B <= 0:
            return rc
        # the second claimant of a row finds the stamp at t again and applies step t + 1 once more
        arr = (L.LazyUnit * n_units).from_address(units.value)
        t = int(_arr(step, (1,), dtype=np.int32)[0])
        ids = _arr(ids_t, (n_units * B,), dtype=np.int32).reshape(n_units, B).copy()
        again = np.zeros_like(ids)
        for u in range(n_units):
            rows = np.where((ids[u] < 0) | (ids[u] >= arr[u].vocab), 0, ids[u])
            uniq, cnt = np.unique(rows, return_counts=True)
            dup = uniq[cnt > 1]
            if not dup.size:
                return rc
            _arr(arr[u].stamp, (arr[u].vocab,), dtype=np.int32)[dup[0]] = t
            again[u] = dup[0]
        return real(units, n_units, ctypes.c_void_p(again.ctypes.data), B, step, opt, vec, max_dim, stream)
    monkeypatch.setattr(mock, "dctr_lazy_apply", bad)


def test_duplicates_applied_twice_fail(mock, monkeypatch):
    _apply_duplicates_twice(mock, monkeypatch)
    msg = _fails(mock, _all_names("ids-adam", "ids-rmsprop"))
    assert "max|d|" in msg, msg


@pytest.mark.parametrize("name", ["ids-sgd-lam0.1-B17", "ids-sgd-lam0.1-B65"])
def test_duplicates_applied_twice_fail_under_sgd(mock, monkeypatch, name):
    """SGD keeps no state: only the weights can show the second step, and at lambda = 0.1 they do"""
    _apply_duplicates_twice(mock, monkeypatch)
    assert "sgd apply unit" in _fails(mock, [name])


@pytest.mark.parametrize("name", ["geometry-sgd-lam0.1-vec4-dim8", "geometry-sgd-lam0.1-vec1-dim5", "ids-sgd-lam0.1-B65",
                                  "sweep-sgd-lam0.1-K7", "long-gaps-sgd-lam0.1-from40"])
def test_a_catchup_that_loses_one_replayed_step_fails_under_sgd(mock, monkeypatch, name):
    """the stamps come out right and SGD has no state: the weights alone show one step too few"""
    from deepctr_torch._hip import lib as L
    real = mock.dctr_lazy_catchup

    def bad(units, n_units, ids_t, B, step, opt, vec, max_dim, order_ws, stream):
        if units and step and ids_t and B > 0:
            arr = (L.LazyUnit * n_units).from_address(units.value)
            t = int(_arr(step, (1,), dtype=np.int32)[0])
            ids = _arr(ids_t, (n_units * B,), dtype=np.int32).reshape(n_units, B)
            for u in range(n_units):
                rows = np.unique(np.where((ids[u] < 0) | (ids[u] >= arr[u].vocab), 0, ids[u]))
                stamp = _arr(arr[u].stamp, (arr[u].vocab,), dtype=np.int32)
                stamp[rows[stamp[rows] < t]] += 1
        return real(units, n_units, ids_t, B, step, opt, vec, max_dim, order_ws, stream)
    monkeypatch.setattr(mock, "dctr_lazy_catchup", bad)
    assert "sgd catchup unit" in _fails(mock, [name])


def test_adam_ss_clamped_with_n_bc_fails(mock, monkeypatch):
    real = mock._adam_scalars

    def bad(o, T):
        if not (o.adam_ss and o.adam_bc):
            return real(o, T)
        ss = _arr(ctypes.c_void_p(o.adam_ss), (o.n_bc,))          # (n_bc > n_ss: reads behind the table, into the sentinel band)
        bc = _arr(ctypes.c_void_p(o.adam_bc), (o.n_bc,))
        return ss[min(T, o.n_bc) - 1], bc[min(T, o.n_bc) - 1]
    monkeypatch.setattr(mock, "_adam_scalars", bad)
    names = [n for n in _all_names("adam-scalars-") if "-all-" in n or "-norbc-" in n]
    msg = _fails(mock, names)
    assert "max|d|" in msg or "not finite" in msg, msg
    for n in _all_names("adam-scalars-"):          # ... and only the cases that pass a table's end notice
        if "-none-" in n:
            dict(CASES)[n](mock, DEV)


def test_a_catchup_that_replays_steps_prev_to_t_minus_1_fails(mock, monkeypatch):
    from deepctr_torch._hip import lib as L
    real = mock.dctr_lazy_catchup

    def bad(units, n_units, ids_t, B, step, opt, vec, max_dim, order_ws, stream):
        if not units or not step or B <= 0:
            return real(units, n_units, ids_t, B, step, opt, vec, max_dim, order_ws, stream)
        # every step number one lower while the catch-up runs: the same rows, the same count of steps, numbered prev .. t-1
        arr = (L.LazyUnit * n_units).from_address(units.value)
        views = [_arr(step, (1,), dtype=np.int32)] + [_arr(un.stamp, (un.vocab,), dtype=np.int32) for un in arr]
        for v in views:
            v -= 1
        rc = real(units, n_units, ids_t, B, step, opt, vec, max_dim, order_ws, stream)
        for v in views:
            v += 1
        return rc
    monkeypatch.setattr(mock, "dctr_lazy_catchup", bad)
    msg = _fails(mock, _all_names("adam-scalars-fast-n_ss-6-all-catchup", "long-gaps-adam"))
    assert "max|d|" in msg or "not finite" in msg, msg


def test_the_unpatched_stand_in_passes_what_the_faults_fail(mock):
    for n in _all_names("sweep-adam", "ids-adam-B17", "adam-scalars-fast-n_ss-6-all", "geometry-adam-vec4-dim8"):
        dict(CASES)[n](mock, DEV)
