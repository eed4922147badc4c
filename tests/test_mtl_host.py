"""CPU: SharedBottom, ESMM, MMOE and PLE through the real Python stack over the stand-in for the library (tests/mock_lib.py,
extended by tests/mock_mtl.py with the gate-mix entry points), against the reference's golden values (tests/golden/mtl,
tools/golden/make_mtl_golden.py): per-task logits within 1e-5, every parameter gradient within 2e-5 x max|g_ref|, the 3-step
trajectories, the Adam runs on the lazy update.  Every fixture was accepted only with every ReLU input at least
``min_relu_margin`` away from 0, so no unit can be on in the reference and off here.  Plus what needs no library at all:
exports, the constructors' errors, ``state_dict`` keys and same-seed initial weights, the refusal of a distributed ``fit()``.
The kernels themselves are checked by tests/test_gpu_gate_mix_kernel.py, the models on the GPU by
tests/test_gpu_mtl_models.py."""
import json
import os

import numpy as np
import pytest
import torch

import mock_mtl
import mtl_helpers as H
from helpers import GOLDEN_DIR, golden_names, load_golden, max_abs

DEV = "cpu"
CONFIGS, METRICS = H.init_configs()


@pytest.fixture()
def mtl_mock(mock):
    return mock_mtl.extend(mock)


def gate_calls(mock, kind):
    return [c for c in mock.calls if c.startswith("gate_mix_" + kind)]


def n_gate_launches(spec):
    return {"MMOE": 1, "PLE": spec["kwargs"].get("num_levels", 2)}.get(spec["model"], 0)


# ---- no library needed ---------------------------------------------------------------------------------------------
def test_models_are_exported():
    import deepctr_torch.models as M
    from deepctr_torch.models import ESMM, MMOE, PLE, SharedBottom
    from deepctr_torch.models import multitask
    for name, cls in (("SharedBottom", SharedBottom), ("ESMM", ESMM), ("MMOE", MMOE), ("PLE", PLE)):
        assert getattr(M, name) is cls and name in M.__all__ and getattr(multitask, name) is cls
    assert multitask.__all__ == ["SharedBottom", "ESMM", "MMOE", "PLE"]


def test_fixture_set_and_margins():
    assert golden_names("mtl/") == sorted(H.ALL + ["init", "init_ple"])
    for name in H.ALL:
        path = os.path.join(GOLDEN_DIR, "mtl", name + ".npz")
        z = np.load(path, allow_pickle=False)
        assert float(z["min_relu_margin"]) >= H.RELU_MARGIN, name
        assert z["y"].ndim == 2 and z["y"].shape == z["y_pred"].shape == z["logit"].shape and z["y"].shape[0] <= 64
    for name in golden_names("mtl/"):
        assert os.path.getsize(os.path.join(GOLDEN_DIR, "mtl", name + ".npz")) < 1 << 20
    assert set(json.loads(str(load_golden("mtl/ple_112")["extra"]["grad_absent"]))) == {
        "shared_gate_dnn.1.linears.0.weight", "shared_gate_dnn.1.linears.0.bias", "shared_gate_dnn_final_layer.1.weight"}
    assert all(json.loads(str(load_golden("mtl/" + n)["extra"]["grad_absent"])) == [] for n in H.ALL if "ple" not in n)
    assert len(CONFIGS) == 14 and METRICS["binary,binary"] and METRICS["binary,regression"]


def test_constructor_errors():
    from deepctr_torch.inputs import SparseFeat
    from deepctr_torch.models import ESMM, MMOE, PLE, SharedBottom
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4)]
    for cls in (SharedBottom, MMOE, PLE):
        with pytest.raises(ValueError, match="num_tasks must be greater than 1"):
            cls(cols, task_types=("binary",), task_names=("ctr",))
        with pytest.raises(ValueError, match="dnn_feature_columns is null!"):
            cls([])
        with pytest.raises(ValueError, match="num_tasks must be equal to the length of task_types"):
            cls(cols, task_types=("binary",))
        with pytest.raises(ValueError, match="task must be binary or regression, multiclass is illegal"):
            cls(cols, task_types=("binary", "multiclass"))
    with pytest.raises(ValueError, match="num_tasks must be greater than 1!"):
        PLE(cols, task_types=("binary",), task_names=("ctr",))
    with pytest.raises(ValueError, match="num_experts must be greater than 1"):
        MMOE(cols, num_experts=1)
    with pytest.raises(ValueError, match="the length of task_names must be equal to 2"):
        ESMM(cols, task_types=("binary",) * 3, task_names=("a", "b", "c"))
    with pytest.raises(ValueError, match="dnn_feature_columns is null!"):
        ESMM([])
    with pytest.raises(ValueError, match="num_tasks must be equal to the length of task_types"):
        ESMM(cols, task_types=("binary",))
    with pytest.raises(ValueError, match="task must be binary in ESMM, regression is illegal"):
        ESMM(cols, task_types=("binary", "regression"))
    with pytest.raises(ValueError, match="should be the same gpu"):
        MMOE(cols, device="cpu", gpus=[1])


@pytest.mark.parametrize("c", CONFIGS, ids=H.config_id)
def test_same_seed_initial_weights_are_the_references(c):
    spec, params = c
    sd = H.build(spec, DEV, l2=None).state_dict()
    assert list(sd) == list(params)
    for k, v in params.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert np.array_equal(sd[k].numpy(), v), k


@pytest.mark.parametrize("name", H.ALL)
def test_state_dict_keys_are_the_fixtures(name):
    g = load_golden("mtl/" + name)
    sd = H.build(g["spec"], DEV).state_dict()
    assert list(sd) == list(g["params"])
    assert all(tuple(sd[k].shape) == v.shape for k, v in g["params"].items())


def test_ple_keeps_the_references_shared_expert_count(mtl_mock):
    """``shared_experts`` holds ``specific_expert_num`` modules per level whatever ``shared_expert_num`` says: with fewer
    shared experts the extra modules are idle, with more the forward fails where the reference's fails"""
    from deepctr_torch.inputs import SparseFeat
    from deepctr_torch.models import PLE
    cols = [SparseFeat("a", 5, 4), SparseFeat("b", 6, 4)]
    kw = dict(expert_dnn_hidden_units=(8,), gate_dnn_hidden_units=(), tower_dnn_hidden_units=())
    m = PLE(cols, shared_expert_num=1, specific_expert_num=2, **kw)
    assert [len(lv[0]) for lv in m.shared_experts] == [2, 2]
    assert tuple(m(torch.tensor([[1., 2.], [3., 4.]])).shape) == (2, 2)
    m = PLE(cols, shared_expert_num=2, specific_expert_num=1, **kw)
    assert [len(lv[0]) for lv in m.shared_experts] == [1, 1]
    with pytest.raises(IndexError):
        m(torch.tensor([[1., 2.], [3., 4.]]))


def test_distributed_fit_is_refused_before_any_process_group(monkeypatch):
    import torch.distributed as dist
    from deepctr_torch.inputs import SparseFeat
    from deepctr_torch.models import ESMM, MMOE, PLE, SharedBottom
    cols = [SparseFeat("a", 5, 4)]
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.delenv("DCTR_FIT_DISTRIBUTED", raising=False)

    def no_group(*a, **k):
        raise AssertionError("a process group was created")
    monkeypatch.setattr(dist, "init_process_group", no_group)
    for cls in (SharedBottom, ESMM, MMOE, PLE):
        m = cls(cols)
        m.compile("adam", ["binary_crossentropy"] * 2, metrics=[])
        with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
            m.fit({"a": np.arange(4) % 5}, np.zeros((4, 2)), batch_size=2, epochs=1, verbose=0)
    assert not dist.is_initialized()


# ---- the models over the stand-in ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.ALL)
def test_logits_match_reference(mtl_mock, name):
    g, m = H.loaded(name, DEV)
    m.train()          # (the fixtures hold the train-mode forward: BatchNorm on the batch's statistics)
    with torch.no_grad():
        logits, y = H.forward_logits(m, torch.from_numpy(g["X"]))
    m.model_plan().check_ids()
    assert tuple(y.shape) == g["y_pred"].shape
    assert max_abs(logits.numpy(), g["logit"]) <= H.LOGIT_TOL
    assert max_abs(y.numpy(), g["y_pred"]) <= H.LOGIT_TOL
    # one gate-mix forward per MMOE forward, one per PLE level; without grad mode no weights are kept
    assert gate_calls(mtl_mock, "fwd") == ["gate_mix_fwd:%d:0" % (m.num_tasks + (g["spec"]["model"] == "PLE"))] * \
        n_gate_launches(g["spec"])
    assert gate_calls(mtl_mock, "bwd") == []


@pytest.mark.parametrize("name", H.ALL)
def test_gradients_match_reference(mtl_mock, name):
    g, m = H.loaded(name, DEV)
    H.check_gradients(g, m, DEV)
    n = n_gate_launches(g["spec"])
    assert len(gate_calls(mtl_mock, "fwd")) == len(gate_calls(mtl_mock, "bwd")) == n
    assert all(c.endswith(":1") for c in gate_calls(mtl_mock, "fwd"))


def test_batchnorm_takes_the_module_route(mtl_mock):
    g, m = H.loaded("mmoe_bn", DEV)
    m.train()
    before = len(mtl_mock.calls)
    m(torch.from_numpy(g["X"]))
    calls = [str(c) for c in mtl_mock.calls[before:]]
    assert not any(c.startswith("mlp") for c in calls), calls
    assert len(gate_calls(mtl_mock, "fwd")) == 1


@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adagradp"])
@pytest.mark.parametrize("name", H.STEPS)
def test_training_trajectory_matches_reference(mtl_mock, name, opt):
    g, m = H.loaded(name, DEV)
    H.check_trajectory(g, m, DEV, opt)
    assert m.model_plan().update[0] == ("sgd" if opt == "sgd" else "adagrad")
    assert len(gate_calls(mtl_mock, "bwd")) == 3 * n_gate_launches(g["spec"])


@pytest.mark.parametrize("tag,l2", [("adam", None), ("adam0", 0.0)])
def test_lazy_adam_replays_reference_trajectory(mtl_mock, tag, l2):
    m = H.check_lazy(load_golden("mtl/lazy_mtl"), DEV, tag, l2)
    assert m.model_plan().update == ("lazy", "adam")


def _outputs_and_grads(g):
    m = H.build(g["spec"], DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    m.train()
    y = m(torch.from_numpy(g["X"]))
    loss = H.list_loss(g["spec"], y, torch.from_numpy(g["y"]))
    m.zero_grad()
    loss.backward()
    return m, y.detach().numpy(), {k: (None if p.grad is None else p.grad.numpy()) for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", ["mmoe", "mmoe_nogate", "ple_112", "ple_333_nogate", "ple_noshared"])
def test_switch_selects_the_torch_op_route_with_the_same_numbers(mtl_mock, monkeypatch, name):
    g = load_golden("mtl/" + name)
    _, y1, g1 = _outputs_and_grads(g)
    assert len(gate_calls(mtl_mock, "fwd")) == n_gate_launches(g["spec"])
    del mtl_mock.calls[:]
    monkeypatch.setenv("DCTR_GATE_MIX", "0")
    _, y0, g0 = _outputs_and_grads(g)
    assert gate_calls(mtl_mock, "fwd") == [] and gate_calls(mtl_mock, "bwd") == []
    assert max_abs(y1, y0) <= 1e-6
    for k, a in g1.items():
        assert (a is None) == (g0[k] is None), k
        if a is not None:
            assert max_abs(a, g0[k]) <= H.GRAD_TOL * float(np.max(np.abs(g0[k]))), k


def test_outside_the_envelope_runs_the_torch_ops(mtl_mock):
    """17 experts: more members than a gate descriptor lists -> the reference's formula as torch ops, same numbers as the
    reference's own expression"""
    from deepctr_torch._hip import ops
    torch.manual_seed(0)
    xs = [torch.randn(6, 5, requires_grad=True) for _ in range(17)]
    h, W = torch.randn(6, 4, requires_grad=True), torch.randn(17, 4, requires_grad=True)
    assert not ops.gate_mix_fused(xs, [h], [W], [tuple(range(17))])
    assert ops.gate_mix_fused(xs[:16], [h], [W[:16]], [tuple(range(16))])
    (out,) = ops.gate_mix(xs, [h], [W], [tuple(range(17))])
    ref = torch.matmul((h @ W.T).softmax(1).unsqueeze(1), torch.stack(xs, 1)).squeeze(1)
    assert gate_calls(mtl_mock, "fwd") == [] and torch.equal(out, ref)
    # a wrong member list or weight shape is an error of the caller, on either route
    with pytest.raises(ValueError, match="gate_mix"):
        ops.gate_mix(xs[:3], [h], [W[:3]], [(0, 1, 3)])
    with pytest.raises(ValueError, match="gate_mix"):
        ops.gate_mix(xs[:3], [h], [W[:2]], [(0, 1, 2)])


def test_gate_mix_reads_strided_views_in_place_and_returns_weight_gradients(mtl_mock):
    from deepctr_torch._hip import ops
    torch.manual_seed(1)
    bufs = [torch.randn(5, 8) for _ in range(3)]
    xs = [b[:, :6].requires_grad_() for b in bufs]                 # what tower(dnn, None, x) returns: hs[-1][:, :N]
    hb = torch.randn(5, 12)
    h = hb[:, :9].requires_grad_()
    Ws = [torch.randn(3, 9, requires_grad=True), torch.randn(2, 9, requires_grad=True)]
    seen = {}
    inner = mtl_mock.dctr_gate_mix_fwd

    def spy(x, ld_x, P, dim, B, gates, G, stream):
        seen["ld_x"] = [int(v) for v in mock_mtl._ptrs(ld_x, P, mock_mtl.ctypes.c_int64)]
        seen["x"] = [int(v) for v in mock_mtl._ptrs(x, P, mock_mtl.ctypes.c_void_p)]
        seen["ld_h"] = [int(gates[g].ld_h) for g in range(G)]
        return inner(x, ld_x, P, dim, B, gates, G, stream)
    mtl_mock.dctr_gate_mix_fwd = spy
    outs = ops.gate_mix(xs, [h, h], Ws, [(0, 1, 2), (2, 0)])
    assert seen["ld_x"] == [8, 8, 8] and seen["x"] == [b.data_ptr() for b in bufs] and seen["ld_h"] == [12, 12]
    refs = [torch.matmul((h @ W.T).softmax(1).unsqueeze(1), torch.stack([xs[e] for e in m], 1)).squeeze(1)
            for W, m in zip(Ws, [(0, 1, 2), (2, 0)])]
    gos = [torch.randn(5, 6), torch.randn(5, 6)]
    got = torch.autograd.grad(outs, xs + [h] + Ws, gos)
    want = torch.autograd.grad(refs, xs + [h] + Ws, gos)
    for o, r in zip(outs, refs):
        assert max_abs(o.detach().numpy(), r.detach().numpy()) <= 1e-6
    for a, b in zip(got, want):
        assert a.shape == b.shape and max_abs(a.numpy(), b.numpy()) <= 2e-5 * float(b.abs().max())
    # an unused output: None for that gate's input and weight, as autograd leaves them in the reference
    outs = ops.gate_mix(xs, [h.detach().requires_grad_(), hb[:, :9].clone().requires_grad_()], Ws, [(0, 1, 2), (2, 0)])
    grads = torch.autograd.grad([outs[0]], Ws, [gos[0]], allow_unused=True)
    assert grads[0] is not None and grads[1] is None


def test_empty_batch(mtl_mock):
    from deepctr_torch._hip import ops
    xs = [torch.zeros(0, 4, requires_grad=True) for _ in range(2)]
    W = torch.randn(2, 3, requires_grad=True)
    (out,) = ops.gate_mix(xs, [torch.zeros(0, 3)], [W], [(0, 1)])
    assert tuple(out.shape) == (0, 4)
    (gW,) = torch.autograd.grad([out], [W], [torch.zeros(0, 4)])
    assert float(gW.abs().max()) == 0.0


@pytest.mark.parametrize("name", ["sb_towers", "esmm", "mmoe", "ple_112"])
def test_whole_model_save_load_round_trip(mtl_mock, name, tmp_path):
    g, m = H.loaded(name, DEV)
    m.compile("adagrad", g["spec"]["losses"], metrics=[])
    m._train_step(torch.from_numpy(g["X"]), torch.from_numpy(g["y"]))
    m.eval()
    with torch.no_grad():
        before = m(torch.from_numpy(g["X"])).numpy()
    path = str(tmp_path / "model.h5")
    torch.save(m, path)
    again = torch.load(path, weights_only=False)
    assert type(again) is type(m) and list(again.state_dict()) == list(g["params"])
    again.eval()
    with torch.no_grad():
        assert np.array_equal(again(torch.from_numpy(g["X"])).numpy(), before)


@pytest.mark.parametrize("name", ["sb_towers", "esmm", "mmoe", "ple_112"])
def test_batch_of_one_keeps_its_shape(mtl_mock, name):
    g, m = H.loaded(name, DEV)
    m.eval()
    with torch.no_grad():
        X = torch.from_numpy(g["X"])
        one, all_ = m(X[:1]), m(X)
    assert tuple(one.shape) == (1, m.num_tasks) and max_abs(one.numpy(), all_[:1].numpy()) <= 1e-6


def test_stand_in_envelope_is_the_headers():
    src = open(os.path.join(os.path.dirname(GOLDEN_DIR), os.pardir, "include", "dctr.h")).read()
    for name, v in (("GATES", mock_mtl.MAX_GATES), ("MEMBERS", mock_mtl.MAX_MEMBERS), ("POOL", mock_mtl.MAX_POOL),
                    ("WIDTH", mock_mtl.MAX_WIDTH)):
        assert "#define DCTR_GATE_MAX_%s %d\n" % (name, v) in src
    from deepctr_torch._hip import lib as L
    assert (L.GATE_MAX_GATES, L.GATE_MAX_MEMBERS, L.GATE_MAX_POOL, L.GATE_MAX_WIDTH) == (8, 16, 32, 1152)
    assert mock_mtl.fits(32, 1152, [16] * 8, [1152] * 8) and not mock_mtl.fits(33, 8, [2], [8])
    assert not mock_mtl.fits(3, 1153, [2], [8]) and not mock_mtl.fits(3, 8, [17], [8]) and not mock_mtl.fits(3, 8, [2], [1153])
    assert not mock_mtl.fits(3, 8, [2] * 9, [8] * 9)
