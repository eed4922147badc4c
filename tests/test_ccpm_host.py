"""CPU: CCPM through the real Python stack over the stand-in for the library (tests/mock_lib.py + mock_ops.py, extended by
tests/mock_ccpm.py with the conv kernel's entry points), against the reference's golden values (tests/golden/ccpm,
tools/golden/make_ccpm_golden.py): logits within 1e-5, every parameter gradient within 2e-5 x max|g_ref|, 3-step
trajectories, the regularised Adam run on the lazy update.  Every fixture was accepted only with a top-k margin
(``min_topk_gap``) far above fp32 rounding, so no selection can differ between the reference and the stand-in.  Plus what
needs no library at all: same-seed initial weights, state_dict keys, the constructor's errors, ``_kernel_fits``, the pooling
sizes.  The kernels themselves are checked by tests/test_gpu_ccpm_kernel.py, the model on the GPU by
tests/test_gpu_ccpm_models.py."""
import json
import os

import numpy as np
import pytest
import torch

import mock_ccpm
from helpers import GOLDEN_DIR, build_model, feature_columns, golden_names, load_golden, max_abs

DEV = "cpu"
LOGIT_TOL, GRAD_TOL, TRAJ_TOL = 1e-5, 2e-5, 2e-5
ALL = ["ccpm_two", "ccpm_three", "ccpm_criteo", "ccpm_f26", "ccpm_mixed", "ccpm_one_layer", "ccpm_three_layers",
       "ccpm_nolinear", "ccpm_bn", "lazy_ccpm", "fit_ccpm"]
STEPS = ["ccpm_two", "ccpm_criteo"]
MIN_GAP = 4e-6


@pytest.fixture()
def ccpm_mock(mock):
    return mock_ccpm.extend(mock)


def _loaded(name, l2=0.0):
    g = load_golden("ccpm/" + name)
    m = build_model(g["spec"], DEV, l2=l2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    return g, m


def grad_scale(key, grads, spec):
    """The gradient bound's scale: max|g_ref| of the parameter, no floor.  One exception, by reasoning and not by result: with
    ``dnn_use_bn`` a Linear bias sits directly in front of a BatchNorm in train mode, which subtracts the batch mean -- its
    exact gradient is 0 and the reference's own value (4.8e-7 here) is the rounding noise of a sum that cancels.  The terms
    of that sum are the rows of the same layer's weight gradient's factor, so that gradient's scale is used."""
    if spec["kwargs"].get("dnn_use_bn") and key.startswith("dnn.linears.") and key.endswith(".bias"):
        key = key[:-len("bias")] + "weight"
    return float(np.max(np.abs(grads[key])))


def test_model_and_layers_are_exported():
    import deepctr_torch.layers as Ly
    import deepctr_torch.models as M
    from deepctr_torch.layers import Conv2dSame, ConvLayer, KMaxPooling
    from deepctr_torch.models import CCPM
    assert M.CCPM is CCPM and "CCPM" in M.__all__
    assert Ly.ConvLayer is ConvLayer and Ly.KMaxPooling is KMaxPooling and Ly.Conv2dSame is Conv2dSame


def test_fixture_set_and_margins():
    assert golden_names("ccpm/") == sorted(ALL + ["init"])
    for name in ALL:
        z = np.load(os.path.join(GOLDEN_DIR, "ccpm", name + ".npz"), allow_pickle=False)
        assert float(z["min_topk_gap"]) >= MIN_GAP, name
        assert os.path.getsize(os.path.join(GOLDEN_DIR, "ccpm", name + ".npz")) < 1 << 20


# ---- the model over the stand-in -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_forward_matches_reference(ccpm_mock, name):
    g, m = _loaded(name)
    # (the fixtures hold the reference's train-mode forward: BatchNorm then normalises with the batch's statistics)
    m.train(bool(g["spec"]["kwargs"].get("dnn_use_bn")))
    cap = {}
    h = m.out.register_forward_pre_hook(lambda mod, inp: cap.__setitem__("logit", inp[0].detach()))
    with torch.no_grad():
        y = m(torch.from_numpy(g["X"]))
    h.remove()
    m.model_plan().check_ids()
    assert max_abs(cap["logit"].numpy(), g["logit"]) <= LOGIT_TOL
    assert max_abs(y.numpy(), g["y_pred"]) <= LOGIT_TOL
    assert ccpm_mock.calls.count("ccpm_fwd:0") == 1 and "ccpm_fwd:1" not in ccpm_mock.calls   # no selection buffer


@pytest.mark.parametrize("name", ALL)
def test_gradients_match_reference(ccpm_mock, name):
    g, m = _loaded(name)
    m.train()
    loss = torch.nn.functional.binary_cross_entropy(m(torch.from_numpy(g["X"])).squeeze(1), torch.from_numpy(g["y"]),
                                                    reduction="sum")
    m.zero_grad()
    loss.backward()
    assert abs(loss.item() - g["loss"]) <= 1e-4 * max(1.0, abs(g["loss"]))
    assert set(g["grads"]) == set(k for k, _ in m.named_parameters())
    for k, p in m.named_parameters():
        ref = g["grads"][k]
        got = p.grad.numpy() if p.grad is not None else np.zeros_like(ref)
        err = max_abs(got, ref)
        assert err <= GRAD_TOL * grad_scale(k, g["grads"], g["spec"]), "%s: max|d|=%.3e max|g_ref|=%.3g" % (
            k, err, np.max(np.abs(ref)))
    assert ccpm_mock.calls.count("ccpm_fwd:1") == 1 and ccpm_mock.calls.count("ccpm_bwd") == 1


@pytest.mark.parametrize("name", STEPS)
@pytest.mark.parametrize("opt", ["sgd", "adagrad", "adagradp"])
def test_in_kernel_optimizer_trajectory(ccpm_mock, name, opt):
    g, m = _loaded(name)
    m.compile("adagrad" if opt == "adagradp" else opt, "binary_crossentropy", metrics=[])
    if opt == "adagradp":
        for grp in m.optim.param_groups:
            for p in grp["params"]:
                m.optim.state[p]["sum"].fill_(0.05)
    m.train()
    losses = [float(m._train_step(torch.from_numpy(Xb), torch.from_numpy(yb))[0])
              for Xb, yb in zip(g["extra"]["X_steps"], g["extra"]["y_steps"])]
    plan = m.model_plan()
    assert plan.update[0] == ("sgd" if opt == "sgd" else "adagrad")
    assert "embed_update:%d" % (0 if opt == "sgd" else 1) in ccpm_mock.calls
    conv = set(id(p) for p in m.conv_layer.parameters())
    assert conv and not conv & set(id(p) for p in plan.table_params)      # the conv parameters: the dense optimizer's
    np.testing.assert_allclose(losses, g["extra"][opt + "3_loss"], rtol=2e-5)
    sd = m.state_dict()
    n = 0
    for k, v in g["extra"].items():
        if k.startswith(opt + "3/"):
            assert max_abs(sd[k[len(opt) + 2:]].numpy(), v) <= TRAJ_TOL, k
            n += 1
    assert n == len(sd)


def test_lazy_adam_replays_reference_trajectory(ccpm_mock):
    g, m = _loaded("lazy_ccpm", l2=1e-3)
    ex = g["extra"]
    m.compile("adam", "binary_crossentropy", metrics=[])
    m.train()
    assert m.model_plan().update == ("lazy", "adam")
    bce, tot = [], []
    for Xb, yb in zip(ex["lazy_X"], ex["lazy_y"]):
        loss, total, _ = m._train_step(torch.from_numpy(Xb), torch.from_numpy(yb))
        bce.append(float(loss))
        tot.append(float(total))
    np.testing.assert_allclose(bce, ex["lazy_adam_bce"], rtol=2e-5)
    np.testing.assert_allclose(tot, ex["lazy_adam_total"], rtol=2e-5)
    sd = m.state_dict()
    for k, v in ex.items():
        if k.startswith("lazy_adam/"):
            ref = np.asarray(v, np.float64)
            err = max_abs(sd[k[len("lazy_adam/"):]].numpy(), ref)
            assert err <= 2e-5 * max(1.0, float(np.max(np.abs(ref)))), k


@pytest.mark.parametrize("name", ALL)
def test_state_dict_keys_are_the_references(name):
    g = load_golden("ccpm/" + name)
    m = build_model(g["spec"], DEV)
    assert list(m.state_dict()) == list(g["params"])
    n = len(g["spec"]["kwargs"]["conv_filters"])
    assert [k for k in m.state_dict() if k.startswith("conv_layer.")] == \
        ["conv_layer.conv_layer.%d.%s" % (3 * i, s) for i in range(n) for s in ("weight", "bias")]


# ---- same-seed initial weights -------------------------------------------------------------------------------------
def _init_configs():
    path = os.path.join(GOLDEN_DIR, "ccpm", "init.npz")
    if not os.path.exists(path):
        return []
    z = np.load(path, allow_pickle=False)
    out = []
    for i, spec in enumerate(json.loads(str(z["configs"]))):
        pre = "%d/param/" % i
        out.append((spec, {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}))
    return out


def test_init_fixture_exists():
    assert len(_init_configs()) == 2


@pytest.mark.parametrize("c", _init_configs(), ids=lambda c: "%ds" % len(c[0]["dnn_columns"]))
def test_same_seed_initial_weights_are_the_references(c):
    from deepctr_torch.models import CCPM
    spec, params = c
    cols = feature_columns(spec["dnn_columns"])
    sd = CCPM(cols, cols, device="cpu", **spec["kwargs"]).state_dict()
    assert list(sd) == list(params)
    for k, v in params.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert np.array_equal(sd[k].numpy(), v), k


# ---- constructor and layers ----------------------------------------------------------------------------------------
def test_constructor_and_forward_errors(ccpm_mock):
    from deepctr_torch.inputs import DenseFeat, SparseFeat
    from deepctr_torch.models import CCPM
    a, b = SparseFeat("a", 5, 4), SparseFeat("b", 6, 4)
    with pytest.raises(ValueError, match="same element"):
        CCPM([a, b], [a, b], conv_kernel_width=(3, 2, 2), conv_filters=(2, 1))
    with pytest.raises(ValueError, match="DenseFeat is not supported"):
        CCPM([a, b], [a, b, DenseFeat("x", 1)])
    with pytest.raises(ValueError, match="must be same"):
        CCPM([a], [a, SparseFeat("c", 6, 8)])
    m = CCPM([a, b], [a, b], dnn_hidden_units=(4,))
    m._plan = None
    m.dnn_feature_columns = []
    with pytest.raises(ValueError, match="must have the embedding feature"):
        m(torch.zeros(3, 2))


def test_kmax_pooling_errors_and_values():
    from deepctr_torch.layers import KMaxPooling
    x = torch.tensor([[3., 1., 2., 5.], [0., 0., -1., 0.]])
    assert KMaxPooling(2, 1)(x).tolist() == [[5., 3.], [0., 0.]]
    with pytest.raises(ValueError, match="axis must be"):
        KMaxPooling(1, 2)(x)
    with pytest.raises(ValueError, match="k must be in"):
        KMaxPooling(5, 1)(x)
    with pytest.raises(ValueError, match="k must be in"):
        KMaxPooling(0, 1)(x)


@pytest.mark.parametrize("w", [1, 2, 3, 4, 6])
def test_conv2d_same_pads_like_the_formula(w):
    """cross-correlation over the rows with (w - 1) // 2 zero rows above and the rest below; the width axis untouched"""
    from deepctr_torch.layers import Conv2dSame
    torch.manual_seed(w)
    conv = Conv2dSame(2, 3, (w, 1)).double()
    x = torch.randn(2, 2, 5, 3, dtype=torch.float64)
    y = conv(x)
    assert tuple(y.shape) == (2, 3, 5, 3)
    top = (w - 1) // 2
    xp = torch.nn.functional.pad(x, [0, 0, top, w - 1 - top])
    ref = conv.bias[None, :, None, None] + sum(
        torch.einsum("oc,bcfd->bofd", conv.weight[:, :, t, 0], xp[:, :, t:t + 5]) for t in range(w))
    assert max_abs(y.detach().numpy(), ref.detach().numpy()) <= 1e-12


@pytest.mark.parametrize("n,widths,filters,ks", [
    (2, (3, 2), (2, 1), [1, 1]), (3, (3, 2), (2, 1), [1, 1]), (26, (6, 5), (4, 4), [13, 3]), (9, (6, 5), (4, 4), [4, 3]),
    (2, (1,), (1,), [2]), (5, (4,), (3,), [3]), (9, (3, 3, 2), (3, 2, 2), [8, 3, 3]), (26, (2, 2, 2), (2, 2, 2), [23, 8, 3])])
def test_conv_layer_pooling_sizes_follow_the_reference_formula(n, widths, filters, ks):
    from deepctr_torch.layers import ConvLayer, Conv2dSame, KMaxPooling
    layer = ConvLayer(n, widths, filters)
    mods = list(layer.conv_layer)
    assert len(mods) == 3 * len(filters)
    assert all(isinstance(mods[3 * i], Conv2dSame) and isinstance(mods[3 * i + 1], torch.nn.Tanh) and
               isinstance(mods[3 * i + 2], KMaxPooling) for i in range(len(filters)))
    assert [mods[3 * i + 2].k for i in range(len(filters))] == ks and layer.filed_shape == ks[-1]
    assert layer._spec() == (list(widths), list(filters), ks)
    assert [tuple(mods[3 * i].weight.shape) for i in range(len(filters))] == \
        [(c, ci, w, 1) for c, ci, w in zip(filters, (1,) + tuple(filters[:-1]), widths)]


@pytest.mark.parametrize("n,widths,filters", [(2, (3, 2), (2, 1)), (5, (4,), (3,)), (9, (3, 3, 2), (3, 2, 2))])
def test_conv_layer_output_shape_and_values(ccpm_mock, n, widths, filters):
    """the fused route (over the stand-in) equals the layer's own Sequential, and has the reference's output shape"""
    from deepctr_torch.layers import ConvLayer
    torch.manual_seed(3)
    layer = ConvLayer(n, widths, filters)
    x = torch.randn(7, 1, n, 4, requires_grad=True)
    y = layer(x)
    assert tuple(y.shape) == (7, filters[-1], layer.filed_shape, 4)
    assert ccpm_mock.calls == ["ccpm_fwd:1"]
    assert max_abs(y.detach().numpy(), layer.conv_layer(x).detach().numpy()) <= 1e-6
    g = torch.randn_like(y)
    got = torch.autograd.grad(y, [x] + list(layer.parameters()), g)
    ref = torch.autograd.grad(layer.conv_layer(x), [x] + list(layer.parameters()), g)
    for a, b in zip(got, ref):
        assert a.shape == b.shape and max_abs(a.numpy(), b.numpy()) <= 2e-5 * float(b.abs().max())


def test_kernel_fits():
    from deepctr_torch.layers import ConvLayer
    fits = ConvLayer._kernel_fits
    assert fits(26, 16, [6, 5], [4, 4], [13, 3])
    assert fits(2, 4, [3, 2], [2, 1], [1, 1]) and fits(64, 64, [16], [1], [3]) and fits(1, 1, [1], [1], [1])
    assert fits(9, 4, [3, 3, 2, 2], [3, 2, 2, 2], [8, 6, 3, 3])
    assert not fits(65, 16, [6, 5], [4, 4], [32, 3])                 # fields
    assert not fits(26, 65, [6, 5], [4, 4], [13, 3])                 # embedding size
    assert not fits(26, 16, [2] * 5, [2] * 5, [20, 15, 10, 5, 3])    # layers
    assert not fits(26, 16, [17, 5], [4, 4], [13, 3]) and not fits(26, 16, [6, 5], [17, 4], [13, 3])
    assert not fits(64, 64, [6, 5], [16, 16], [32, 3])               # the LDS image: 16 x 64 x 64 activations
    assert not fits(26, 16, [6, 5], [4, 4], [27, 3])                 # k beyond the rows of its input
    # the stand-in's envelope is the header's: both state the same budget
    for args in [(26, 16, [6, 5], [4, 4], [13, 3]), (64, 64, [6, 5], [16, 16], [32, 3]), (64, 64, [16], [1], [3]),
                 (64, 32, [6, 5], [4, 4], [32, 3]), (64, 64, [6, 5], [4, 4], [32, 3])]:
        assert fits(*args) == mock_ccpm.fits(*args), args


def test_shapes_outside_the_kernel_run_the_sequential(ccpm_mock):
    from deepctr_torch.layers import ConvLayer
    torch.manual_seed(0)
    layer = ConvLayer(70, (6, 5), (4, 4))
    y = layer(torch.randn(3, 1, 70, 4))
    assert tuple(y.shape) == (3, 4, 3, 4) and ccpm_mock.calls == []


@pytest.mark.parametrize("widths,filters", [((3,), (1,)), ((3, 2), (2, 2))])
def test_tie_rule_through_the_layer(ccpm_mock, widths, filters):
    """E = 0 (and no bias below the last layer, so that the zero padding does not show): every column of every layer is
    constant.  Through ``ConvLayer`` over the stand-in: the selection handed to the backward is rows 0..k-1 in order, and
    the input gradient is that of a pooling which takes exactly those rows."""
    from deepctr_torch.layers import ConvLayer, Conv2dSame
    torch.manual_seed(2)
    layer = ConvLayer(5, widths, filters)
    convs = [m for m in layer.conv_layer if isinstance(m, Conv2dSame)]
    with torch.no_grad():
        for c in convs[:-1]:
            c.bias.zero_()
        convs[-1].bias.fill_(0.1)
    ks = layer._spec()[2]
    seen = {}
    inner = ccpm_mock.dctr_ccpm_bwd

    def spy(*a):
        n_sel = sum(c * k for c, k in zip(filters, ks)) * 3
        seen["sel"] = mock_ccpm._arr(a[10], (2 * n_sel,), dtype=np.uint8).reshape(2, n_sel).copy()
        return inner(*a)
    ccpm_mock.dctr_ccpm_bwd = spy
    x = torch.zeros(2, 1, 5, 3, requires_grad=True)
    y = layer(x)
    assert ccpm_mock.calls == ["ccpm_fwd:1"]
    go = torch.ones_like(y)
    (gx,) = torch.autograd.grad(y, [x], go)
    want = np.concatenate([np.broadcast_to(np.arange(k)[None, None, :, None], (2, c, k, 3)).reshape(2, -1)
                           for c, k in zip(filters, ks)], axis=1)
    assert np.array_equal(seen["sel"], want)
    # the same stack with the pooling replaced by "take rows 0..k-1", as torch ops
    x2 = torch.zeros(2, 1, 5, 3, requires_grad=True)
    h = x2
    for c, k in zip(convs, ks):
        h = torch.tanh(c(h))[:, :, :k]
    (gref,) = torch.autograd.grad(h, [x2], go)
    assert max_abs(y.detach().numpy(), h.detach().numpy()) <= 1e-7
    assert float(gref.abs().max()) > 0 and max_abs(gx.numpy(), gref.numpy()) <= 2e-5 * float(gref.abs().max())


def test_other_dtypes_run_the_sequential(ccpm_mock):
    """the kernel is float32 only: a double input (and double weights) takes the layer's own modules, gradients included"""
    from deepctr_torch.layers import ConvLayer
    torch.manual_seed(0)
    layer = ConvLayer(5, (3, 2), (2, 2)).double()
    x = torch.randn(3, 1, 5, 4, dtype=torch.float64, requires_grad=True)
    y = layer(x)
    assert y.dtype == torch.float64 and tuple(y.shape) == (3, 2, 2, 4) and ccpm_mock.calls == []
    (g,) = torch.autograd.grad(y.sum(), [x])
    assert g.dtype == torch.float64


def test_pool_sizes_helper_is_exported():
    from deepctr_torch.layers import ccpm_pool_sizes
    assert ccpm_pool_sizes(26, 2) == [13, 3] and ccpm_pool_sizes(2, 2) == [1, 1] and ccpm_pool_sizes(9, 3) == [8, 3, 3]
    assert ccpm_pool_sizes(2, 1) == [2] and ccpm_pool_sizes(5, 0) == []
