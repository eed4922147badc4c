"""CPU: IFM and DIFM through the real Python stack over the stand-in for the library (tests/mock_lib.py + mock_ops.py,
extended by tests/mock_iafm.py with the input-aware FM pair and the per-field-wide gather / update), against the reference's
golden forward values, per-parameter gradients, 3-step SGD / Adagrad trajectories and the 8-step regularised Adam run
(tests/golden/iafm).  Pins, without a GPU: the per-field wide buffer and its gradient through EmbedFunction (sorted update,
general units, the two-pass lazy route), IAFMFunction's marshalling, the models' wiring.  The kernels are checked by
tests/test_gpu_iafm_*.py and tests/test_gpu_wide_per_field.py."""
import numpy as np
import pytest
import torch

import mock_iafm
from helpers import build_model, load_golden, max_abs

DEV = "cpu"
NAMES = ["ifm_criteo", "ifm_mixed", "difm_criteo"]


@pytest.fixture()
def iafm_mock(mock):
    return mock_iafm.extend(mock)


def _loaded(name, l2=0.0):
    g = load_golden("iafm/" + name)
    m = build_model(g["spec"], DEV, l2=l2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    return g, m


@pytest.mark.parametrize("name", NAMES + ["ifm_one_field", "ifm_nolinear", "ifm_dense_linear_only", "difm_mixed", "difm_d6"])
def test_forward_matches_reference(iafm_mock, name):
    g, m = _loaded(name)
    m.eval()
    with torch.no_grad():
        y = m(torch.from_numpy(g["X"]))
    assert max_abs(y.numpy(), g["y_pred"]) <= 2e-5
    m.model_plan().check_ids()
    assert iafm_mock.calls.count("embed_fwd") == 1 and iafm_mock.calls.count("iafm_fwd") == 1


@pytest.mark.parametrize("name", NAMES + ["ifm_one_field", "ifm_nolinear", "ifm_dense_linear_only", "difm_mixed", "difm_d6"])
def test_dense_gradients_match_reference(iafm_mock, name):
    g, m = _loaded(name)
    m.train()
    loss = torch.nn.functional.binary_cross_entropy(m(torch.from_numpy(g["X"])).squeeze(1), torch.from_numpy(g["y"]),
                                                    reduction="sum")
    m.zero_grad()
    loss.backward()
    assert abs(loss.item() - g["loss"]) <= 1e-4 * max(1.0, abs(g["loss"]))
    for k, p in m.named_parameters():
        ref = g["grads"][k]
        got = p.grad.numpy() if p.grad is not None else np.zeros_like(ref)
        assert max_abs(got, ref) <= 2e-5 * max(1.0, float(np.max(np.abs(ref)))), k
    assert iafm_mock.calls.count("iafm_bwd") == 1


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_in_kernel_optimizer_trajectory(iafm_mock, name, opt):
    g, m = _loaded(name)
    m.compile(opt, "binary_crossentropy", metrics=[])
    m.train()
    losses = [float(m._train_step(torch.from_numpy(Xb), torch.from_numpy(yb))[0])
              for Xb, yb in zip(g["extra"]["X_steps"], g["extra"]["y_steps"])]
    plan = m.model_plan()
    assert plan.wide_per_field and plan.update[0] == opt and plan.unit_path
    assert "embed_update:%d" % (0 if opt == "sgd" else 1) in iafm_mock.calls
    assert not any(c.startswith("embed_bwd") for c in iafm_mock.calls)
    np.testing.assert_allclose(losses, g["extra"][opt + "3_loss"], rtol=5e-5)
    sd = m.state_dict()
    for k, v in g["extra"].items():
        if k.startswith(opt + "3/"):
            assert max_abs(sd[k[len(opt) + 2:]].numpy(), v) <= 1e-4, k
    for d in (m.embedding_dict, m.linear_model.embedding_dict):
        assert not d.__dict__.get("_dctr_plans")


def test_lazy_adam_replays_reference_trajectory(iafm_mock):
    """The reference's default kind of training on the exact lazy update: ids -> catch-up -> gather -> update(ACCUM) with the
    per-field wide gradient -> apply (the stand-in's dctr_embed_update_lazy answers DCTR_ENOSUP: the two-pass route)."""
    g, m = _loaded("lazy_ifm", l2=1e-3)
    ex = g["extra"]
    m.compile("adam", "binary_crossentropy", metrics=[])
    m.train()
    assert m.model_plan().update == ("lazy", "adam")
    bce, tot = [], []
    for Xb, yb in zip(ex["lazy_X"], ex["lazy_y"]):
        loss, total, _ = m._train_step(torch.from_numpy(Xb), torch.from_numpy(yb))
        bce.append(float(loss))
        tot.append(float(total))
    assert "embed_update:2" in iafm_mock.calls and "lazy_apply" in iafm_mock.calls
    np.testing.assert_allclose(bce, ex["lazy_adam_bce"], rtol=5e-5)
    np.testing.assert_allclose(tot, ex["lazy_adam_total"], rtol=5e-5)
    sd = m.state_dict()
    for k, v in ex.items():
        if k.startswith("lazy_adam/"):
            ref = np.asarray(v, np.float64)
            err = max_abs(sd[k[len("lazy_adam/"):]].numpy(), ref)
            assert err <= 5e-5 * max(1.0, float(np.max(np.abs(ref)))), k


def test_linear_forward_with_a_refine_weight_still_works(iafm_mock):
    """``Linear.forward(X, sparse_feat_refine_weight=...)`` called directly keeps its secondary-plan route."""
    g, m = _loaded("ifm_criteo")
    X = torch.from_numpy(g["X"])
    F = m.sparse_feat_num
    refine = torch.rand(X.shape[0], F)
    got = m.linear_model(X, sparse_feat_refine_weight=refine)
    lm = m.linear_model
    cols = [c for c in g["spec"]["linear_columns"] if c["kind"] == "sparse"]
    want = sum(lm.embedding_dict[c["name"]].weight[X[:, m.feature_index[c["name"]][0]].long()] * refine[:, i:i + 1]
               for i, c in enumerate(cols))
    dense = torch.cat([X[:, m.feature_index[c["name"]][0]:m.feature_index[c["name"]][1]]
                       for c in g["spec"]["linear_columns"] if c["kind"] == "dense"], 1)
    want = want + dense @ lm.weight
    assert max_abs(got.detach().numpy(), want.detach().numpy()) <= 1e-6
