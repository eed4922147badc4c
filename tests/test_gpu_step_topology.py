"""The autograd-assembled fused train step (DCTR_STEP_ENGINE=0: dctr_embed_fwd + dctr_mlp_train_step + ..., the update on the
pre-pass's side stream) against the numpy oracle.  tests/test_gpu_step_engine.py compares the step engine with this step bit
for bit; this file anchors both to the reference's arithmetic.

A small vocabulary on purpose: most rows are touched by consecutive steps, i.e. the gather of step n+1 reads what the
update of step n wrote a few microseconds earlier."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F_SPARSE, N_DENSE, DIM, B = 26, 13, 16, 4096


def _data(vocab, n_batches):
    gen = torch.Generator().manual_seed(7)
    n = B * n_batches
    ids = torch.randint(0, vocab, (n, F_SPARSE), generator=gen)
    X = torch.cat([ids.float(), torch.rand(n, N_DENSE, generator=gen)], dim=1).to(DEV)
    y = torch.randint(0, 2, (n,), generator=gen).float().to(DEV)
    return X, y


@pytest.mark.parametrize("opt", ["adagrad", "sgd"])
def test_default_topology_follows_the_oracle_trajectory(opt):
    """What the bit-comparisons of tests/test_gpu_step_engine.py are anchored to: six steps against the numpy oracle's fp64 train
    step (oracle/np_oracle.py Oracle.train_step: the reference's dense update, pinned to its 3-step goldens) on a small
    vocabulary -- every parameter within 2e-5 (Adagrad: 2e-4 of the elements may sit on the other side of a sign of a ~1e-9
    gradient, as in tests/test_gpu_models.py)."""
    import numpy as np
    from np_oracle import Oracle
    vocab, Bs, steps = 500, 512, 6
    os.environ["DCTR_STEP_ENGINE"] = "0"
    try:
        # (init_std 0.05, not the default 1e-4: with 1e-4 weights the embedding gradients are ~1e-9 -- at Adagrad's eps of
        # 1e-10 -- and g / (|g| + eps) of an fp32 and an fp64 evaluation differ by percents: the AFM case of test_gpu_models)
        from deepctr_torch.inputs import DenseFeat, SparseFeat
        from deepctr_torch.models import DeepFM
        fcols = [SparseFeat("C%d" % (i + 1), vocab, DIM) for i in range(F_SPARSE)] + \
                [DenseFeat("I%d" % (i + 1), 1) for i in range(N_DENSE)]
        m = DeepFM(fcols, fcols, dnn_hidden_units=(256, 128), l2_reg_linear=0, l2_reg_embedding=0, dnn_dropout=0, seed=1024,
                   init_std=0.05, device=DEV)
        m.compile(opt, "binary_crossentropy", metrics=[])
        m.train()
        X, y = _data(vocab, 1)
        spec = {"model": "DeepFM", "kwargs": {"dnn_hidden_units": [256, 128]},
                "linear_columns": None, "dnn_columns": None}
        cols = [{"kind": "sparse", "name": "C%d" % (i + 1), "vocab": vocab, "dim": DIM, "embedding_name": "C%d" % (i + 1)}
                for i in range(F_SPARSE)] + [{"kind": "dense", "name": "I%d" % (i + 1), "dimension": 1} for i in range(N_DENSE)]
        spec["linear_columns"] = spec["dnn_columns"] = cols
        o = Oracle(spec, {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, dtype=np.float64)
        st = None
        for i in range(steps):
            xb, yb = X[i * Bs:(i + 1) * Bs], y[i * Bs:(i + 1) * Bs]
            loss = m._train_step(xb, yb)[0]
            lo, st = o.train_step(xb.cpu().numpy(), yb.cpu().numpy(), optimizer=opt, lr=0.01, eps=1e-10, state=st)
            assert abs(float(loss) - lo) <= 2e-5 * max(1.0, abs(lo))
        sd = m.state_dict()
        for k, v in o.P.items():
            d = np.abs(sd[k].double().cpu().numpy() - np.asarray(v).reshape(tuple(sd[k].shape)))
            if opt == "sgd":
                assert float(d.max()) <= 2e-5 * max(1.0, float(np.abs(v).max())), k
            else:
                assert float((d > 2e-5).mean()) <= 2e-4 and float(d.max()) <= 0.2, "%s: %.3e" % (k, d.max())
    finally:
        os.environ.pop("DCTR_STEP_ENGINE", None)
