"""CPU: DIEN through the real Python stack over the stand-in for the library (tests/mock_lib.py + mock_ops.py, extended by
tests/mock_din.py and tests/mock_dien.py with the attention and the recurrence entry points), against the reference's
golden values (tests/golden/dien, tools/golden/make_dien_golden.py): logits within 1e-5, the auxiliary loss, every
parameter gradient within 2e-5 x max|g_ref|, 3-step trajectories, the adam run, ``fit()``.  Plus what needs no library at
all: same-seed initial weights, state_dict keys, the constructors' errors, which route a call takes, the trainers'
refusal, the bound on T, and that the kernel test's inputs can be held by float32 arithmetic at all.  The kernels
themselves are checked by tests/test_gpu_gru_seq_kernel.py, the model on the GPU by tests/test_gpu_dien_models.py."""
import os

import numpy as np
import pytest
import torch

import dien_helpers as H
import mock_dien
import mock_din
from helpers import GOLDEN_DIR, feature_columns, golden_names, load_golden, max_abs

DEV = "cpu"


@pytest.fixture()
def dien_mock(mock):
    return mock_dien.extend(mock_din.extend(mock))


def _gru_calls(mock):
    return [c for c in mock.calls if c.startswith("gru_")]


def test_model_and_layers_are_exported():
    import deepctr_torch.layers as Ly
    import deepctr_torch.models as M
    from deepctr_torch.layers import AGRUCell, AUGRUCell, DynamicGRU
    from deepctr_torch.models import DIEN
    from deepctr_torch.models.dien import InterestEvolving, InterestExtractor  # noqa: F401
    assert M.DIEN is DIEN and "DIEN" in M.__all__
    assert Ly.AGRUCell is AGRUCell and Ly.AUGRUCell is AUGRUCell and Ly.DynamicGRU is DynamicGRU


def test_fixture_set():
    assert golden_names("dien/") == sorted(H.ALL + ["init"])
    for name in H.ALL + ["init"]:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, "dien", name + ".npz")) < 1 << 20
    from deepctr_torch.inputs import build_input_features
    for name in H.ALL:
        g = load_golden("dien/" + name)
        assert 16 <= g["X"].shape[0] <= 40
        fi = build_input_features(feature_columns(g["spec"]["dnn_columns"]))
        T = [c["maxlen"] for c in g["spec"]["dnn_columns"] if c["name"].startswith("hist_")][0]
        lens = g["X"][:, fi["seq_length"][0]]
        assert [int(v) for v in lens[:4]] == [0, 1, T - 1, T], name
        assert float(g["extra"]["min_relu_margin"]) >= 2e-6
        cols = dict((c["name"], c) for c in g["spec"]["dnn_columns"])
        for n_ in cols:                  # the negative history has ids of its own
            if n_.startswith("neg_hist_"):
                a, b = fi[n_], fi[n_[4:]]
                assert not np.array_equal(g["X"][:, a[0]:a[1]], g["X"][:, b[0]:b[1]])


# ---- the stand-in itself against float64 autograd of the cell loop ---------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("outputs", ["both", "states", "last"])
def test_stand_in_matches_float64_autograd(mode, outputs):
    c = dict(name="standin%d%s" % (mode, outputs), dims=(5,), T=6, B=9, mode=mode, lens=[0, 1, 5, 6, 9, -1, 3, 2, 6],
             outputs=outputs, layout="contig", ld_extra=0)
    a, ref = H.case_inputs(c), H._reference(c, torch.float64)
    att = a["att"] if mode else None
    st, la, _ = mock_dien.forward(a["x"], att, a["lens"], a["params"], mode)
    gx, ga, gp = mock_dien.backward(a["x"], att, a["lens"], a["params"], mode,
                                    a["g_states"] if outputs != "last" else None,
                                    a["g_last"] if outputs != "states" else None)
    assert max_abs(st, ref["states"]) <= 1e-12 and max_abs(la, ref["last"]) <= 1e-12
    assert max_abs(gx, ref["gx"]) <= 1e-11 and max_abs(gp, ref["g_params"]) <= 1e-11
    if mode:
        assert max_abs(ga, ref["g_att"]) <= 1e-11
    n = np.clip(a["lens"], 0, 6)
    pad = np.arange(6)[None, :] >= n[:, None]
    assert not st[pad].any() and not gx[pad].any() and not ga[pad].any()
    if mode == 2:
        assert not mock_dien.unpack(gp, 5)[0][5:10].any() and not mock_dien.unpack(gp, 5)[1][5:10].any()


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_kernel_case_inputs_are_within_float32s_reach(name):
    """every shape of tests/test_gpu_gru_seq_kernel.py: float32 torch within a quarter of each tolerance of float64"""
    dev = H.check_case_is_testable(name)
    print(name, dict((k, "%.2e/%.2g" % v) for k, v in dev.items()))


def test_product_torch_route_is_the_same_recurrence():
    from deepctr_torch.layers.sequence import gru_sequence_torch
    for name in ("h5_t7_m0", "h5_t7_m1", "h5_t7_m2", "h5_t7_m3"):
        c = H.CASES[name]
        a, ref = H.case_inputs(c), H.reference(name)
        p = torch.from_numpy(a["params"]).double()
        w = (p[:75].reshape(15, 5), p[75:150].reshape(15, 5), p[150:165], p[165:])
        st, la = gru_sequence_torch(torch.from_numpy(a["x"]).double(), torch.from_numpy(a["att"]).double(),
                                    torch.from_numpy(a["lens"]), *w, gru_type=["GRU", "AIGRU", "AGRU", "AUGRU"][c["mode"]])
        assert max_abs(st.numpy(), ref["states"]) <= 1e-12 and max_abs(la.numpy(), ref["last"]) <= 1e-12


# ---- the model over the stand-in -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.ALL)
def test_forward_matches_reference(dien_mock, name):
    g, m = H.loaded(name, DEV)
    H.check_forward(g, m, DEV)
    assert _gru_calls(dien_mock) == H.expected_calls(g, False)


@pytest.mark.parametrize("name", H.ALL)
def test_gradients_match_reference(dien_mock, name):
    g, m = H.loaded(name, DEV)
    H.check_gradients(g, m, DEV)
    assert _gru_calls(dien_mock) == H.expected_calls(g, True)


@pytest.mark.parametrize("name", H.STEPS)
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adagradp"])
def test_optimizer_trajectory(dien_mock, name, opt):
    g, m = H.loaded(name, DEV)
    H.check_trajectory(g, m, DEV, opt)
    assert not getattr(m, "_fused_step_ok", False)
    assert len([c for c in _gru_calls(dien_mock) if c.startswith("gru_bwd")]) == 6


def test_default_kwargs_adam_trajectory(dien_mock):
    g = load_golden("dien/dien_default_adam")
    m = H.build_dien(g["spec"], DEV, l2=1e-6)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    H.check_trajectory(g, m, DEV, "adam")


@pytest.mark.parametrize("tag,opt,l2,shuffle", [("plain", "adagrad", 0.0, False), ("shuffled", "adagrad", 0.0, True),
                                                ("default", "adam", 1e-5, True)])
def test_fit_history_and_predict(dien_mock, monkeypatch, tag, opt, l2, shuffle):
    monkeypatch.setenv("DCTR_FIT_GRAPH", "0")            # (no device to capture on; the GPU file runs both ways)
    g, m = H.loaded("fit_dien", DEV, l2=l2)
    H.check_fit(g, m, tag, opt, shuffle)


@pytest.mark.parametrize("name", H.ALL)
def test_state_dict_keys_are_the_references(name):
    g = load_golden("dien/" + name)
    assert list(H.build_dien(g["spec"], DEV).state_dict()) == list(g["params"])


def test_init_fixture_exists():
    assert len(H.init_configs()) == 9


@pytest.mark.parametrize("c", H.init_configs(),
                         ids=lambda c: "%s-%s" % (c[0]["kwargs"].get("gru_type", "default"), c[0]["kwargs"].get("use_negsampling")))
def test_same_seed_initial_weights_are_the_references(c):
    spec, params = c
    m = H.build_dien(spec, DEV, l2=1e-6)
    sd = m.state_dict()
    assert list(sd) == list(params)
    for k, v in params.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert np.array_equal(sd[k].numpy(), v), k
    named = [k for k, _ in m.named_parameters()]
    if spec["kwargs"].get("gru_type") == "AUGRU":           # the reference's tie: ONE Parameter behind both bias names
        assert "interest_evolution.interest_evolution.rnn.bias_ih" in named
        assert "interest_evolution.interest_evolution.rnn.bias_hh" not in named
        assert "interest_evolution.interest_evolution.rnn.bias_hh" in sd
        rnn = m.interest_evolution.interest_evolution.rnn
        assert rnn.bias_ih is rnn.bias_hh
    for key in ("interest_extractor.gru.weight_ih_l0", "interest_evolution.attention.local_att.dense.weight", "linear.weight"):
        assert key in sd
    if spec["kwargs"].get("use_negsampling"):
        assert "interest_extractor.auxiliary_net.linears.0.weight" in sd


def test_only_the_embeddings_are_regularised():
    g = load_golden("dien/dien_augru_neg")
    m = H.build_dien(dict(g["spec"], kwargs=dict(g["spec"]["kwargs"], l2_reg_dnn=0.5)), DEV, l2=1e-6)
    assert len(m.regularization_weight) == 2 and not getattr(m, "_fused_step_ok", False)
    assert m.model_plan().unpooled_columns == ("hist_item_id", "hist_cate_id", "neg_hist_item_id", "neg_hist_cate_id")


# ---- constructors and errors -----------------------------------------------------------------------------------------
def test_constructor_errors(dien_mock):
    from deepctr_torch.inputs import SparseFeat, VarLenSparseFeat
    from deepctr_torch.layers import DynamicGRU
    from deepctr_torch.models import DIEN
    from deepctr_torch.models.dien import InterestEvolving
    with pytest.raises(NotImplementedError, match="is not supported"):
        InterestEvolving(4, gru_type="LSTM")
    cols = [SparseFeat("item", 5, 4), VarLenSparseFeat(SparseFeat("hist_item", 5, 4, embedding_name="item"), 3)]
    with pytest.raises(NotImplementedError, match="is not supported"):
        DIEN(cols, ["item"], gru_type="nope")
    m = DIEN(cols, ["item"], dnn_hidden_units=(4,))
    with pytest.raises(ValueError, match="please add max length column"):
        m(torch.zeros(2, 4))
    with pytest.raises(NotImplementedError, match="only supports packed input"):
        DynamicGRU(4, 4)(torch.zeros(2, 3, 4), torch.zeros(2, 3))


def test_the_bound_on_T_is_named():
    from deepctr_torch.inputs import SparseFeat, VarLenSparseFeat
    from deepctr_torch.models import DIEN

    def cols(T, neg):
        out = [SparseFeat("item", 5, 4),
               VarLenSparseFeat(SparseFeat("hist_item", 5, 4, embedding_name="item"), T, length_name="seq_length")]
        if neg:
            out.append(VarLenSparseFeat(SparseFeat("neg_hist_item", 5, 4, embedding_name="item"), T, length_name="seq_length"))
        return out
    DIEN(cols(127, False), ["item"], dnn_hidden_units=(4,))
    DIEN(cols(63, True), ["item"], dnn_hidden_units=(4,), use_negsampling=True)
    with pytest.raises(ValueError, match="DCTR_MAX_UNIT_SLOTS = 128.*T <= 127.*T <= 63"):
        DIEN(cols(128, False), ["item"], dnn_hidden_units=(4,))
    with pytest.raises(ValueError, match="DCTR_MAX_UNIT_SLOTS = 128"):
        DIEN(cols(64, True), ["item"], dnn_hidden_units=(4,), use_negsampling=True)


# ---- the layers ------------------------------------------------------------------------------------------------------
_Q = [[1, 1, 1], [0.1, 0.2, 0.3]]
_K = [[[0.1, 0.2, 0.3], [1, 2, 3], [0.4, 0.2, 1], [0.0, 0.0, 0.0]], [[0.1, 0.2, 0.3], [1, 2, 3], [0.4, 0.2, 1], [0.5, 0.5, 0.5]]]


@pytest.mark.parametrize("gru_type", ["AIGRU", "AUGRU", "AGRU", "GRU"])
def test_interest_evolving_on_the_references_tensors(dien_mock, gru_type):
    """the reference's own layer test (2 x 4 x 3, lengths 3 and 4): the kernel route against the torch-op route"""
    from deepctr_torch.models.dien import InterestEvolving
    torch.manual_seed(0)
    layer = InterestEvolving(input_size=3, gru_type=gru_type, use_neg=False, init_std=0.5)
    q, k, n = torch.tensor(_Q), torch.tensor(_K), torch.tensor([3, 4])
    with torch.no_grad():
        out = layer(q, k, n)
    assert tuple(out.shape) == (2, 3)
    calls = _gru_calls(dien_mock)
    assert calls == ["gru_fwd:%d:0" % H.MODES[gru_type]]
    os.environ["DCTR_GRU_SEQ"] = "0"
    try:
        with torch.no_grad():
            plain = layer(q, k, n)
    finally:
        del os.environ["DCTR_GRU_SEQ"]
    assert _gru_calls(dien_mock) == calls and max_abs(out.numpy(), plain.numpy()) <= 1e-6


def test_dynamic_gru_on_packed_input_is_the_cell_loop():
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    from deepctr_torch.layers import DynamicGRU
    torch.manual_seed(2)
    for gt in ("AGRU", "AUGRU"):
        layer = DynamicGRU(4, 4, gru_type=gt).double()
        with torch.no_grad():
            layer.rnn.weight_ih.normal_(0, 0.5)
            layer.rnn.weight_hh.normal_(0, 0.5)
            layer.rnn.bias_hh.normal_(0, 0.1)
        x, a, n = torch.randn(5, 6, 4, dtype=torch.float64), torch.rand(5, 6, dtype=torch.float64), torch.tensor([6, 1, 3, 5, 2])
        out = layer(pack_padded_sequence(x, n, batch_first=True, enforce_sorted=False),
                    pack_padded_sequence(a, n, batch_first=True, enforce_sorted=False))
        states, _ = pad_packed_sequence(out, batch_first=True, padding_value=0.0, total_length=6)
        ref_states, ref_last = layer.fused(x, a, n, want_states=True, want_last=True)       # CPU tensors: torch ops
        states = states.detach()
        assert max_abs(states.numpy(), ref_states.detach().numpy()) <= 1e-12
        assert max_abs(states[torch.arange(5), n - 1].numpy(), ref_last.detach().numpy()) <= 1e-12
        p = torch.cat([layer.rnn.weight_ih.reshape(-1), layer.rnn.weight_hh.reshape(-1), layer.rnn.bias_ih, layer.rnn.bias_hh])
        st, _, _ = mock_dien.forward(x.numpy(), a.numpy(), n.numpy(), p.detach().numpy(), H.MODES[gt])
        assert max_abs(states.numpy(), st) <= 1e-12


def test_augru_tied_bias_gets_the_sum_of_both_halves(dien_mock):
    from deepctr_torch.layers import DynamicGRU
    torch.manual_seed(4)
    layer = DynamicGRU(3, 3, gru_type="AUGRU")
    with torch.no_grad():
        layer.rnn.weight_ih.normal_(0, 0.5)
        layer.rnn.weight_hh.normal_(0, 0.5)
        layer.rnn.bias_ih.normal_(0, 0.1)
    x, a, n = torch.randn(4, 5, 3), torch.rand(4, 5), torch.tensor([5, 0, 2, 7])
    _, last = layer.fused(x, a, n)
    g = torch.randn_like(last)
    (gb,) = torch.autograd.grad(last, [layer.rnn.bias_ih], g)
    assert _gru_calls(dien_mock) == ["gru_fwd:3:1", "gru_bwd:3"]
    p = torch.cat([layer.rnn.weight_ih.reshape(-1), layer.rnn.weight_hh.reshape(-1), layer.rnn.bias_ih, layer.rnn.bias_hh])
    _, _, gp = mock_dien.backward(x.numpy(), a.numpy(), n.numpy(), p.detach().numpy(), 3, None, g.numpy())
    assert max_abs(gb.numpy(), gp[54:63] + gp[63:72]) <= 1e-6


# ---- which route a call takes ----------------------------------------------------------------------------------------
def _layer_call(mock, T=3, Hd=4, dtype=torch.float32, gru_type="AGRU"):
    from deepctr_torch.layers import DynamicGRU
    if mock is not None:
        del mock.calls[:]
    layer = DynamicGRU(Hd, Hd, gru_type=gru_type).to(dtype)
    with torch.no_grad():
        layer.rnn.weight_ih.normal_(0, 0.3)
        layer.rnn.weight_hh.normal_(0, 0.3)
        out = layer.fused(torch.randn(2, T, Hd, dtype=dtype), torch.rand(2, T, dtype=dtype), torch.tensor([1, T]))[1]
    assert tuple(out.shape) == (2, Hd) and bool(torch.isfinite(out).all())
    return _gru_calls(mock) if mock is not None else None


def test_route_by_shape_dtype_and_switch(dien_mock, monkeypatch):
    assert _layer_call(dien_mock) == ["gru_fwd:2:0"]
    assert _layer_call(dien_mock, gru_type="AUGRU") == ["gru_fwd:3:0"]
    assert _layer_call(dien_mock, T=128, Hd=64) == ["gru_fwd:2:0"]
    assert _layer_call(dien_mock, T=129) == []                      # outside the envelope: torch ops
    assert _layer_call(dien_mock, Hd=65) == []
    assert _layer_call(dien_mock, dtype=torch.float64) == []
    monkeypatch.setenv("DCTR_GRU_SEQ", "0")
    assert _layer_call(dien_mock) == []


def test_cpu_tensors_run_the_torch_ops():
    _layer_call(None)                                               # no stand-in, no library: must not be needed
    g, m = H.loaded("dien_augru_neg", DEV)
    from deepctr_torch.models.dien import InterestExtractor
    ext = InterestExtractor(4, use_neg=True, init_std=0.3)
    k, nk = torch.randn(3, 5, 4), torch.randn(3, 5, 4)
    states, aux = ext(k, torch.tensor([0, 1, 4]), nk)
    assert tuple(states.shape) == (3, 5, 4) and not states[0].any() and not states[1, 1:].any() and float(aux.detach()) > 0


@pytest.mark.parametrize("name", ["dien_gru_neg", "dien_aigru_neg", "dien_agru_neg", "dien_augru_neg", "dien_gru"])
def test_all_zero_lengths_give_zero_hist_and_zero_auxiliary_loss(dien_mock, name):
    """the deliberate difference from the reference, which raises ValueError on such a batch: the interest states, the
    evolved interest (GRU: 1/T weights over states that are all 0) and the auxiliary loss are exactly 0, and the logit is
    that of the tower on ``[0, sparse embeddings, dense]``"""
    from deepctr_torch.inputs import build_input_features
    g, m = H.loaded(name, DEV)
    fi = build_input_features(feature_columns(g["spec"]["dnn_columns"]))
    X = g["X"].copy()
    X[:, fi["seq_length"][0]] = 0
    seen = {}
    h = m.interest_evolution.register_forward_hook(
        lambda mod, inp, out: seen.update(hist=out.detach().clone(), states=inp[1].detach().clone()))
    cap = {}
    h2 = m.out.register_forward_pre_hook(lambda mod, inp: cap.__setitem__("logit", inp[0].detach().clone()))
    m.train()
    with torch.no_grad():
        m(torch.from_numpy(X))
    h.remove()
    h2.remove()
    B = X.shape[0]
    assert tuple(seen["hist"].shape) == (B, 12) and tuple(seen["states"].shape) == (B, 4, 12)
    assert not seen["hist"].any() and not seen["states"].any()
    assert float(m.aux_loss) == 0.0
    # the logit against the stock modules on the tower input that hist = 0 implies
    plan = m.model_plan()
    with torch.no_grad():
        gathered, _, _ = m.fused_inputs(torch.from_numpy(X))
        sparse_w = sum(f.dim for f in plan.deep[:len(m.sparse_feature_columns)])
        x = torch.cat([torch.zeros(B, 12), gathered[:, :sparse_w],
                       gathered[:, plan.dense_off:plan.dense_off + len(plan.dense_cols)]], dim=-1)
        want = m.linear(m.dnn(x))
    assert max_abs(cap["logit"].numpy(), want.numpy()) <= 1e-6


# ---- multi-GPU trainers ----------------------------------------------------------------------------------------------
def test_multi_gpu_trainers_refuse(monkeypatch):
    import torch.distributed as dist
    from deepctr_torch import distributed_fit, parallel
    g = load_golden("dien/dien_augru")
    m = H.build_dien(g["spec"], DEV)
    m.compile("adagrad", "binary_crossentropy")
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    for cls in (parallel.DataParallelTrainer, parallel.ShardedTrainer):
        with pytest.raises(NotImplementedError, match="un-pooled behaviour sequences"):
            cls(m)
    with pytest.raises(NotImplementedError, match="un-pooled behaviour sequences"):
        distributed_fit.fit(m, torch.zeros(4, 6), torch.zeros(4), 2, 1, 0, 0, False, None, None, False, None)


def test_graph_replay_is_not_ruled_out_by_the_auxiliary_loss():
    g, m = H.loaded("dien_augru_neg", DEV)
    m.compile("adagrad", "binary_crossentropy")
    m.add_auxiliary_loss(torch.zeros(1), 0.5)
    from deepctr_torch.models import BaseModel
    assert not m._aux_is_default() and not BaseModel._graph_safe_step(m)
    m._graph_safe_step()
    assert not m._aux_is_default()                                  # the override leaves the flag as it found it


def test_a_forward_lets_go_of_the_previous_steps_auxiliary_graph(dien_mock):
    """``model.aux_loss`` outlives its step; were its graph still alive when the next forward builds its own, the parameters'
    AccumulateGrad nodes would be reused -- with the stream of the step that made them, which breaks a hipGraph capture"""
    g, m = H.loaded("dien_augru_neg", DEV)
    X = torch.from_numpy(g["X"])
    w = m.interest_extractor.auxiliary_net.linears[0].weight            # (used by the auxiliary net alone)

    def accumulator():
        return w.view_as(w).grad_fn.next_functions[0][0]
    m.train()
    m(X)
    assert m.aux_loss.grad_fn is not None
    accumulator().metadata["step"] = 1                                   # alive through model.aux_loss
    assert accumulator().metadata.get("step") == 1
    m(X)
    assert m.aux_loss.grad_fn is not None and "step" not in accumulator().metadata
