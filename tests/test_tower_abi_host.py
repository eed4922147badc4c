"""CPU: the C-ABI driver of the DNN tower and its fused train step (tests/tower_abi.py) over the stand-in library.  The
driver's float64 model is written from include/dctr.h, the stand-in's tower (tests/mock_lib.py) composes forward, head and
backward in float64 and rounds once: two statements of the contract held against each other on the very case list the device
runs (tests/test_gpu_tower_abi.py), with the same bounds -- guards, pad columns and NULL tensors' slots bit-identical,
gW's pad columns 0, both routes through the weight gradients the same bits, parameters and Adagrad state after the in-kernel
step.  Every check of a fixed bar also asserts that plain float32 numpy stays within a quarter of it at that case (the
driver's ``_verify``): running the list here is that rule, at every case.

The launcher's arithmetic restated in the driver (``launch_arm``, ``wgrad_plan``) is held to the figures the cases were
chosen by and, for the workspace sizes, to the real library (its size functions run on the host).

The cases can fail: sixteen stand-ins with one seeded fault each, each rejected by the case named beside it.  Faults are
seeded in the stand-in only; nothing here touches a kernel or a device."""
import ctypes

import numpy as np
import pytest

import tower_abi as TA
from mock_lib import _arr

DEV = "cpu"
CASES = TA.case_list()
NARROW = "fast2-keep-B37-K13-8"


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_case_over_the_stand_in(mock, name):
    dict(CASES)[name](mock, DEV)


def test_case_ids_are_unique():
    names = [n for n, _ in CASES]
    assert len(names) == len(set(names))


def test_every_arm_of_the_train_kernel_has_a_case():
    """(fast, bwd_off > 0) of mlp_train_body: the three fast values with the forward's image kept, fast 1 and 0 with the
    backward's tiles aliasing it (fast 2 cannot alias: every layer at most 256 wide leaves both images under 150 KB)"""
    arms = set((a[0], a[2]) for _, _, a in TA.GEOMETRY)
    assert arms == {(2, True), (1, True), (0, True), (1, False), (0, False)}
    kcs = set(a[1] for _, _, a in TA.GEOMETRY)
    assert kcs == {512, 256, 64}


def test_the_restated_launcher_gives_the_figures_the_cases_were_chosen_by():
    a = TA.launch_arm(500, (512, 64))
    assert (a["lds_f"], a["lds_b"], a["bwd_off"]) == (99840, 66560, 0) and a["lds_f"] + a["lds_b"] > 150 * 1024
    a = TA.launch_arm(1100, (1152, 64))
    assert (a["kc"], a["lds_f"], a["fast"], a["bwd_off"]) == (64, 153088, 0, 0) and 150 * 1024 - a["lds_f"] == 512
    a = TA.launch_arm(429, (1024, 512, 256))
    assert (a["kc"], a["fast"], a["bwd_off"]) == (256, 0, 0)
    a = TA.launch_arm(429, (256, 128))          # the tower of every model test
    assert (a["fast"], a["kc"]) == (1, 512) and a["bwd_off"] == a["lds_f"] // 4 > 0
    assert TA.launch_arm(754, (64, 32, 16))["fast"] == 0 and TA.launch_arm(754, (64, 32, 16))["bwd_off"] > 0
    assert TA.launch_arm(13, (8,))["fast"] == 2 and TA.launch_arm(13, (8,))["bwd_off"] > 0


def test_the_restated_wgrad_plan_gives_the_library_s_workspace_sizes():
    """the size functions read the descriptor's shapes only and run without a device (tests/test_tower_host_geometry.py)"""
    from deepctr_torch._hip import lib as L
    lib = L.lib()
    shapes = [(kw["B"], kw["K"], tuple(kw["hidden"])) for _, kw, _ in TA.GEOMETRY]
    shapes += [(200, 39, (256, 128)), (1000, 39, (256, 128)), (4096, 429, (256, 128)), (1024, 40, (130, 64))]
    for B, K, hidden in shapes:
        ks = [K] + list(hidden[:-1])
        ld_w = [TA.r4(k) + 4 for k in ks]
        for proj in (True, False):
            m = L.Mlp()
            m.n_layers = len(hidden)
            for l, (k, n) in enumerate(zip(ks, hidden)):
                e = m.layer[l]
                e.W, e.K, e.N, e.ld_w, e.ld_h, e.relu = 16, k, n, ld_w[l], TA.r4(n) + 4, 1
            m.w_out = 16 if proj else None
            p = TA.wgrad_plan(K, hidden, B, proj, ld_w)
            assert lib.dctr_mlp_bwd_workspace_floats(ctypes.byref(m), B) == p["bwd_ws"], (B, K, hidden, proj)
            assert lib.dctr_mlp_train_workspace_floats(ctypes.byref(m), B) == p["train_ws"], (B, K, hidden, proj)


# ---- the checks bite -------------------------------------------------------------------------------------------------------
def _fails(mock, name):
    with pytest.raises(AssertionError) as info:
        with np.errstate(all="ignore"):
            dict(CASES)[name](mock, DEV)
    return str(info.value)


def _layers(mref):
    m = mref._obj
    return m, [m.layer[l] for l in range(m.n_layers)]


def _after(monkeypatch, mock, name, post):
    """``post(*args)`` runs behind the stand-in's entry point ``name``"""
    real = getattr(mock, name)

    def bad(*a):
        rc = real(*a)
        if rc == 0 and a[3] > 0:
            post(*a)
        return rc
    monkeypatch.setattr(mock, name, bad)


def test_w_padding_multiplied_into_the_product_fails(mock, monkeypatch):
    def post(mref, x, ld_x, B, logit, stream):
        e = _layers(mref)[1][0]
        xf, Wf = _arr(x, (B, e.K + 1), ld_x), _arr(e.W, (e.N, e.K + 1), e.ld_w)
        _arr(e.h, (B, e.N), e.ld_h)[...] += 1e-6 * np.outer(xf[:, e.K], Wf[:, e.K])
    _after(monkeypatch, mock, "dctr_mlp_fwd", post)
    assert "('h', 0): max|d|" in _fails(mock, NARROW + "-fwd-bwd")


def test_an_ignored_ld_x_fails(mock, monkeypatch):
    real = mock.dctr_mlp_fwd
    monkeypatch.setattr(mock, "dctr_mlp_fwd", lambda mref, x, ld_x, *a: real(mref, x, mref._obj.layer[0].K, *a))
    assert "('h', 0): max|d|" in _fails(mock, NARROW + "-fwd-bwd")


def test_an_ignored_ld_h_fails(mock, monkeypatch):
    def post(mref, x, ld_x, B, logit, stream):
        e = _layers(mref)[1][0]
        _arr(e.h, (B, e.N), e.N)[...] = _arr(e.h, (B, e.N), e.ld_h).copy()
    _after(monkeypatch, mock, "dctr_mlp_fwd", post)
    msg = _fails(mock, NARROW + "-fwd-bwd")
    assert "outside what the call writes" in msg or "('h', 0)" in msg, msg


def test_gw_padding_left_unwritten_fails(mock, monkeypatch):
    real = mock.dctr_mlp_bwd

    def bad(mref, x, ld_x, B, *a):
        e = _layers(mref)[1][0]
        pad = _arr(e.gW + 4 * e.K, (e.N, e.ld_w - e.K), e.ld_w)
        keep = pad.copy()
        rc = real(mref, x, ld_x, B, *a)
        pad[...] = keep
        return rc
    monkeypatch.setattr(mock, "dctr_mlp_bwd", bad)
    assert "pad columns [K, ld_w) are not all 0" in _fails(mock, NARROW + "-fwd-bwd")


def test_a_relu_mask_of_greater_or_equal_fails(mock, monkeypatch):
    real = mock.dctr_mlp_bwd

    def bad(mref, x, ld_x, B, *a):
        e = _layers(mref)[1][0]
        h = _arr(e.h, (B, e.N), e.ld_h)
        keep = h.copy()
        h[h == 0] = 1e-30          # (h >= 0 lets the gradient through where the unit is off)
        rc = real(mref, x, ld_x, B, *a)
        h[...] = keep
        return rc
    monkeypatch.setattr(mock, "dctr_mlp_bwd", bad)
    assert "('dh', 0)" in _fails(mock, NARROW + "-fwd-bwd")


def test_the_last_ragged_tile_missing_from_gbias_fails(mock, monkeypatch):
    def post(mref, x, ld_x, B, *a):
        e = _layers(mref)[1][0]
        _arr(e.gbias, (e.N,))[...] -= _arr(e.dh, (B, e.N), e.ld_h)[B // 16 * 16:].sum(0)
    _after(monkeypatch, mock, "dctr_mlp_train_step", post)
    assert "('gbias', 0): max|d|" in _fails(mock, "rows-B17-train")
    dict(CASES)["rows-B16-train"](mock, DEV)          # (no ragged tile: the fault has nothing to drop)


def test_the_last_tile_s_partial_missing_from_the_loss_fails(mock, monkeypatch):
    def post(mref, x, ld_x, B, p0, p1, bias, y, y_pred, loss, *a):
        p, t = _arr(y_pred, (B,)).astype(np.float64)[B // 16 * 16:], _arr(y, (B,)).astype(np.float64)[B // 16 * 16:]
        li = -(t * np.maximum(np.log(p), -100) + (1 - t) * np.maximum(np.log(1 - p), -100))
        _arr(loss, (1,))[0] -= li.sum()
    _after(monkeypatch, mock, "dctr_mlp_train_step", post)
    assert "loss: max|d|" in _fails(mock, "rows-B33-train")


def test_an_ignored_part1_fails(mock, monkeypatch):
    real = mock.dctr_mlp_train_step
    monkeypatch.setattr(mock, "dctr_mlp_train_step", lambda mref, x, ld_x, B, p0, p1, *a: real(mref, x, ld_x, B, p0, None, *a))
    assert "y_pred: max|d|" in _fails(mock, NARROW + "-train")


def test_a_null_head_bias_read_as_y0_fails(mock, monkeypatch):
    real = mock.dctr_mlp_train_step

    def bad(mref, x, ld_x, B, p0, p1, bias, y, *a):
        return real(mref, x, ld_x, B, p0, p1, bias if bias is not None else y, y, *a)
    monkeypatch.setattr(mock, "dctr_mlp_train_step", bad)
    assert "y_pred: max|d|" in _fails(mock, "head-bias-null-train")
    dict(CASES)[NARROW + "-train"](mock, DEV)          # (a bias that is given is read as itself)


def test_g_w_out_from_the_pre_relu_top_layer_fails(mock, monkeypatch):
    def post(mref, x, ld_x, B, p0, p1, bias, y, y_pred, loss, g_logit, *a):
        m, (e,) = _layers(mref)
        pre = _arr(x, (B, e.K), ld_x).astype(np.float64) @ _arr(e.W, (e.N, e.K), e.ld_w).astype(np.float64).T \
            + _arr(e.bias, (e.N,))
        _arr(m.g_w_out, (e.N,))[...] = _arr(g_logit, (B,)).astype(np.float64) @ pre
    _after(monkeypatch, mock, "dctr_mlp_train_step", post)
    assert "g_w_out: max|d|" in _fails(mock, NARROW + "-train")


def test_an_optimizer_step_applied_twice_fails(mock, monkeypatch):
    real = mock._dense_step

    def bad(step, gptr, n):
        real(step, gptr, n)
        real(step, gptr, n)
    monkeypatch.setattr(mock, "_dense_step", bad)
    assert "param W: max|d|" in _fails(mock, NARROW + "-sgd")
    assert "max|d|" in _fails(mock, NARROW + "-adagrad")


def _state_of(step, gptr, n):
    s = step._obj
    addr = gptr.value if isinstance(gptr, ctypes.c_void_p) else int(gptr)
    return s, _arr(addr, (n,)), _arr(s.param_base + addr - s.grad_base, (n,)), \
        (_arr(s.state_base + addr - s.grad_base, (n,)) if s.kind == 1 else None)


def test_an_adagrad_state_that_is_not_updated_fails(mock, monkeypatch):
    real = mock._dense_step

    def bad(step, gptr, n):
        if step is None or not gptr:
            return
        st = _state_of(step, gptr, n)[3]
        keep = st.copy()
        real(step, gptr, n)
        st[...] = keep
    monkeypatch.setattr(mock, "_dense_step", bad)
    assert "state W: max|d|" in _fails(mock, NARROW + "-adagrad")


def test_adagrad_by_the_root_of_s_plus_eps_fails(mock, monkeypatch):
    def bad(step, gptr, n):
        if step is None or not gptr:
            return
        s, g, p, st = _state_of(step, gptr, n)
        st += g * g
        p -= np.float32(s.lr) * (g / np.sqrt(st + np.float32(s.eps)))
    monkeypatch.setattr(mock, "_dense_step", bad)
    assert "param W: max|d|" in _fails(mock, "adagrad-eps0.1")
    dict(CASES)[NARROW + "-adagrad"](mock, DEV)          # (at eps = 1e-10 the two formulas agree to 1e-9 of a step)


def test_a_gbias_written_although_bias_is_null_fails(mock, monkeypatch):
    def post(mref, x, ld_x, B, *a):
        for e in _layers(mref)[1]:
            if not e.bias:
                _arr(e.gbias, (e.N,))[...] = _arr(e.dh, (B, e.N), e.ld_h).sum(0)
    _after(monkeypatch, mock, "dctr_mlp_train_step", post)
    assert "outside what the call writes" in _fails(mock, "bias-null-layer1-train")


@pytest.mark.parametrize("entry,case", [("dctr_mlp_bwd", NARROW + "-fwd-bwd"), ("dctr_mlp_train_step", NARROW + "-train")])
def test_a_write_one_float_past_the_advertised_workspace_fails(mock, monkeypatch, entry, case):
    def post(mref, x, ld_x, B, *a):
        ws = a[-2] if entry == "dctr_mlp_bwd" else a[-4]
        fn = mock.dctr_mlp_bwd_workspace_floats if entry == "dctr_mlp_bwd" else mock.dctr_mlp_train_workspace_floats
        _arr(ws, (fn(mref, B) + 1,))[-1] = 0.0
    _after(monkeypatch, mock, entry, post)
    assert "outside what the call writes" in _fails(mock, case)


def test_1e_30_where_the_reference_is_exactly_zero_fails(mock, monkeypatch):
    def post(mref, x, ld_x, B, *a):
        e = _layers(mref)[1][0]
        dh = _arr(e.dh, (B, e.N), e.ld_h)
        dh[dh == 0] = 1e-30
    _after(monkeypatch, mock, "dctr_mlp_train_step", post)
    assert "not 0 where the float64 reference is exactly 0" in _fails(mock, NARROW + "-train")


def test_the_unpatched_stand_in_passes_what_the_faults_fail(mock):
    for n in (NARROW + "-fwd-bwd", NARROW + "-train", NARROW + "-sgd", NARROW + "-adagrad", "rows-B17-train", "rows-B33-train",
              "head-bias-null-train", "bias-null-layer1-train", "adagrad-eps0.1"):
        dict(CASES)[n](mock, DEV)
