"""CPU: the host bookkeeping of the Adam / RMSprop dense step of the autograd route (BaseModel._step_dense_multi ->
dctr_dense_opt_multi_reg + dctr_lazy_step_inc) over the numpy stand-in for the library.  The stand-in core of
tests/mock_lib.py has no ``dctr_dense_opt_multi_reg``; a subclass defined HERE adds it (and logs ``dctr_lazy_step_inc``
with the counter it advances), so both sides of the probe are pinned: with the entry point the step is items ->
dense_opt_multi_reg -> ONE lazy_step_inc on the dense counter and never ``optim.step()``; without it -- every existing
mock-based test -- ``optim.step()`` runs and the step is not replay-safe, exactly as before.  The kernels' arithmetic is
covered by tests/test_gpu_dense_multi_reg.py."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import build_model, load_golden, max_abs
from mock_lib import _arr, _make

DEV = "cpu"


def _reg_lib():
    Base = _make()

    class RegLib(Base):
        """the stand-in + the ABI-35 entry point, stated with the stand-in's own fp32 optimizer step"""

        def __init__(self):
            super(RegLib, self).__init__()
            self.reg_items = []          # per call: [(p, g, s1, s2, n, l2)]
            self.reg_steps = []          # per call: the step number the launch read

        def dctr_lazy_step_inc(self, step, stream):
            addr = step.value if isinstance(step, ctypes.c_void_p) else int(step)
            self.calls.append("lazy_step_inc:%d" % addr)
            return super(RegLib, self).dctr_lazy_step_inc(step, stream)

        def dctr_dense_opt_multi_reg(self, items, n_items, optref, step, stream):
            self.calls.append("dense_opt_multi_reg")
            if optref is None or not step or n_items < 0:
                return -1
            o = optref._obj
            if o.kind not in (0, 1, 2, 3):
                return -1
            T = int(_arr(step, (1,), dtype=np.int32)[0]) + 1
            row = []
            for i in range(n_items):
                it = items[i]
                row.append((it.p, it.g, it.s1, it.s2, it.n, it.l2))
                if it.n < 0 or (it.n and (not it.p or not it.g or (o.kind != 0 and not it.s1) or
                                          (o.kind == 2 and not it.s2))):
                    return -1
            self.reg_items.append(row)
            self.reg_steps.append(T)
            for (p, g, s1, s2, n, l2) in row:
                if not n:
                    continue
                P, G = _arr(ctypes.c_void_p(p), (n,)), _arr(ctypes.c_void_p(g), (n,))
                A = _arr(ctypes.c_void_p(s1), (n,)) if o.kind != 0 else None
                B = _arr(ctypes.c_void_p(s2), (n,)) if o.kind == 2 else None
                gt = G + (np.float32(2.0) * np.float32(l2)) * P if l2 else G
                ss, bc = self._adam_scalars(o, T) if o.kind == 2 else (0, 1)
                self._opt_step(o, gt, P, A, B, ss, bc)
            return 0
    return RegLib()


def _install(monkeypatch, lib):
    from deepctr_torch._hip import lib as L
    monkeypatch.setattr(L, "lib", lambda: lib)
    monkeypatch.setattr(L, "require_gpu", lambda t, what: None)
    monkeypatch.setattr(L, "stream_handle", lambda device=None: None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    return lib


@pytest.fixture
def reg(monkeypatch):
    return _install(monkeypatch, _reg_lib())


def _dcn(opt, l2=0.0):
    g = load_golden("lazy_dcn")
    m = build_model(g["spec"], DEV, l2=l2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    m.compile(opt, "binary_crossentropy", metrics=[])
    m.train()
    return g, m


def _steps(g, m, n, start=0):
    ex = g["extra"]
    out = []
    for i in range(start, start + n):
        out.append(float(m._train_step(torch.from_numpy(ex["lazy_X"][i]), torch.from_numpy(ex["lazy_y"][i]))[0]))
    return out


def _dense(m):
    tables = set(id(p) for p in m.model_plan().table_params)
    return [p for p in m.parameters() if id(p) not in tables]


def _no_optim_step(m, monkeypatch):
    hits = []
    monkeypatch.setattr(m.optim, "step", lambda *a, **k: hits.append(1))
    return hits


@pytest.mark.parametrize("opt,l2", [("adam", 0.0), ("adam", 1e-3), ("rmsprop", 0.0)])
def test_dcn_step_is_items_kernel_one_increment_and_no_optim_step(reg, monkeypatch, opt, l2):
    g, m = _dcn(opt, l2)
    hits = _no_optim_step(m, monkeypatch)
    _steps(g, m, 3)
    assert not hits, "optim.step() ran beside the kernel route"
    ck = m._dense_clock
    tag = "lazy_step_inc:%d" % ck["step"].data_ptr()
    assert reg.calls.count("dense_opt_multi_reg") == 3 and reg.calls.count(tag) == 3
    # per step: the kernel, then the increment of ITS counter, nothing of the dense step in between or after
    i = 0
    for _ in range(3):
        i = reg.calls.index("dense_opt_multi_reg", i)
        assert reg.calls[i + 1] == tag, reg.calls[i:i + 3]
        i += 2
    assert reg.reg_steps == [1, 2, 3]                       # read from the device counter, advanced once per step
    assert int(ck["step"][0]) == 3
    dense = _dense(m)
    keys = ("exp_avg", "exp_avg_sq") if opt == "adam" else ("square_avg",)
    want = {}
    for p in dense:
        st = m.optim.state[p]
        want[p.data_ptr()] = tuple(st[k].data_ptr() for k in keys)
    row = reg.reg_items[-1]
    assert sorted(it[0] for it in row) == sorted(want)        # every dense parameter, nothing else
    for (p, gp, s1, s2, n, lam) in row:
        assert (s1,) + ((s2,) if opt == "adam" else ()) == want[p]      # the optimizer's OWN state tensors
        assert gp and n > 0
    if l2:
        reg_ids = dict((q.data_ptr(), lam) for q, lam in m._fusable_l2().values())
        assert reg_ids and all(it[5] == np.float32(reg_ids.get(it[0], 0.0)) for it in row)     # (the struct's float)
    assert m._graph_safe_step()
    assert m.optim._opt_called


def test_state_step_follows_the_counter_on_flush_and_on_optimizer_state_dict(reg, monkeypatch):
    g, m = _dcn("adam")
    _steps(g, m, 3)
    dense = _dense(m)
    m._flush_lazy()
    assert all(float(m.optim.state[p]["step"]) == 3 for p in dense)
    _steps(g, m, 2, start=3)
    sd = m.optim.state_dict()                                  # the pre-hook, no model call
    n = 0
    for grp in m.optim.param_groups:
        for idx, p in zip(sd["param_groups"][m.optim.param_groups.index(grp)]["params"], grp["params"]):
            if any(p is q for q in dense):
                assert float(sd["state"][idx]["step"]) == 5
                n += 1
    assert n == len(dense)
    # ... and the trajectory is the one torch's own step gives from the same start (5e-5: the stand-in's fp32 order)
    from mock_lib import MockLib
    _install(monkeypatch, MockLib())
    g2, m2 = _dcn("adam")
    _steps(g2, m2, 5)
    a, b = m.state_dict(), m2.state_dict()
    for k in a:
        scale = max(1.0, float(b[k].abs().max()))
        assert max_abs(a[k].numpy(), b[k].numpy()) <= 5e-5 * scale, k


def test_a_parameter_without_gradient_ends_one_step_behind(reg):
    g, m = _dcn("adam")
    dense = _dense(m)
    frozen = dense[-1]
    _steps(g, m, 1)
    frozen.requires_grad_(False)
    ex = g["extra"]
    m._train_step(torch.from_numpy(ex["lazy_X"][1]), torch.from_numpy(ex["lazy_y"][1]))
    frozen.requires_grad_(True)
    m._train_step(torch.from_numpy(ex["lazy_X"][2]), torch.from_numpy(ex["lazy_y"][2]))
    m.optim.state_dict()
    for p in dense:
        assert float(m.optim.state[p]["step"]) == (2 if p is frozen else 3)


def test_switch_and_unmodified_stand_in_keep_the_torch_route(mock, monkeypatch):
    """``mock`` is the UNMODIFIED stand-in (tests/conftest.py): no dctr_dense_opt_multi_reg."""
    assert not hasattr(mock, "dctr_dense_opt_multi_reg")
    g, m = _dcn("adam")
    hits = []
    real = m.optim.step
    monkeypatch.setattr(m.optim, "step", lambda *a, **k: (hits.append(1), real(*a, **k))[1])
    _steps(g, m, 3)
    assert len(hits) == 3 and "dense_opt_multi_reg" not in mock.calls
    assert not m._graph_safe_step()
    assert all(float(m.optim.state[p]["step"]) == 3 for p in _dense(m))


def test_multi_adam_switch_leaves_only_sgd_and_adagrad_on_the_kernels(reg, monkeypatch):
    monkeypatch.setenv("DCTR_MULTI_ADAM", "0")
    g, m = _dcn("adam")
    hits = []
    real = m.optim.step
    monkeypatch.setattr(m.optim, "step", lambda *a, **k: (hits.append(1), real(*a, **k))[1])
    _steps(g, m, 2)
    assert len(hits) == 2 and "dense_opt_multi_reg" not in reg.calls and not m._graph_safe_step()
    g, m = _dcn("adagrad")
    _steps(g, m, 2)
    assert "dense_opt_multi" in reg.calls
