"""What the AFN tests share (tests/test_afn_host.py on the stand-in, tests/test_gpu_afn_models.py on the GPU): the fixture
list and the bounds, which come from the fixtures' own float64 runs (tools/golden/make_afn_golden.py).

AFN's gradients are ill-conditioned -- 1/x of the log, exp, batch statistics over small batches: the float32 reference
deviates from its float64 self by up to 3.4e-5 x max|g| on these fixtures, more than the flat 2e-5 every other family is
held to.  So a gradient is compared with the FLOAT64 reference, within max(2e-5, 4 x the float32 reference's own deviation
from it), per parameter; trajectories likewise per ``state_dict`` entry."""
import numpy as np
import torch

from helpers import build_model, load_golden, max_abs

LOGIT_TOL, GRAD_TOL, TRAJ_TOL = 1e-5, 2e-5, 2e-5
ALL = ["afn_two", "afn_three", "afn_criteo", "afn_f26", "afn_nolinear", "afn_sigmoid", "afn_varlen", "fit_afn"]
STEPS = ["afn_two", "afn_criteo"]
LOGIT_DEV, GRAD_DEV = 2.5e-6, 5e-5          # the generator's acceptance margins


def loaded(name, device, l2=0.0):
    g = load_golden("afn/" + name)
    m = build_model(g["spec"], device, l2=l2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    return g, m


def scale_key(key):
    """The parameter whose gradient gives the bound's scale: the parameter itself, except -- by reasoning, not by result --
    where the exact gradient is zero or shares its terms with a neighbour's:

    * ``afn_dnn.linears.<i>.bias`` sits directly in front of a train-mode BatchNorm, which subtracts the batch mean: its
      exact gradient is 0, the reference's value is the rounding noise of a sum that cancels, and the terms of that sum are
      those of the same layer's weight gradient (the rule tests/test_gpu_ccpm_models.py::grad_scale states);
    * ``ltl.bn.1.bias`` adds a constant per embedding channel to the input of ``afn_dnn.linears.0``, whose BatchNorm
      subtracts it again: exactly 0 as well, its terms are those of ``ltl.bn.1.weight``'s sum;
    * ``afn_dnn.bn.<i>.bias`` sums the same per-sample gradients as ``afn_dnn.bn.<i>.weight`` (there weighted by the
      normalised activations, which are O(1)), so it is held to that scale."""
    if key.startswith("afn_dnn.") and key.endswith(".bias"):
        return key[:-len("bias")] + "weight"
    if key == "ltl.bn.1.bias":
        return "ltl.bn.1.weight"
    return key


def grad_bounds(g):
    """{key: (float64 gradient, bound)}: max(2e-5, 4 x the float32 reference's recorded deviation) x the scale"""
    ex, out = g["extra"], {}
    for k, g32 in g["grads"].items():
        g64 = ex["ref64/grad/" + k]
        scale = float(np.max(np.abs(ex["ref64/grad/" + scale_key(k)])))
        dev = max_abs(g32, g64) / scale if scale > 0 else 0.0
        out[k] = (g64, max(GRAD_TOL, 4.0 * dev) * scale)
    return out


def check_gradients(g, grads, tag):
    """``grads``: {key: numpy gradient}.  -> the worst error / bound (printed by the callers)"""
    bounds = grad_bounds(g)
    assert set(bounds) == set(grads)
    worst = 0.0
    for k, (g64, bound) in bounds.items():
        err = max_abs(grads[k], g64)
        if bound > 0:
            worst = max(worst, err / bound)
        assert err <= bound, "%s %s: max|d|=%.3e bound %.3e" % (tag, k, err, bound)
    return worst


def check_trajectory(g, opt, sd, tag):
    """every ``state_dict`` entry against the float64 trajectory, within max(2e-5, 4 x the float32 reference trajectory's
    own deviation from it); the step counters exactly"""
    ex, n, worst = g["extra"], 0, 0.0
    pre64, pre32 = "ref64/%s3/" % opt, "%s3/" % opt
    for k, v64 in ex.items():
        if not k.startswith(pre64):
            continue
        key = k[len(pre64):]
        got = sd[key].cpu().numpy()
        n += 1
        if key.endswith("num_batches_tracked"):
            assert int(got) == int(v64) == int(ex[pre32 + key]), key
            continue
        bound = max(TRAJ_TOL, 4.0 * max_abs(ex[pre32 + key], v64))
        err = max_abs(got, v64)
        worst = max(worst, err / bound)
        assert err <= bound, "%s %s: max|d|=%.3e bound %.3e" % (tag, key, err, bound)
    assert n == len(sd)
    return worst


def run_steps(g, m, opt, device):
    """``run_case``'s 3-step runs: they start from the state AFTER its first train-mode forward on the fixture's batch (the
    running statistics have moved once), with Adagrad's accumulators preset for ``adagradp``.  -> the three losses"""
    m.train()
    with torch.no_grad():
        m(torch.from_numpy(g["X"]).to(device))
    m.compile("adagrad" if opt == "adagradp" else opt, "binary_crossentropy", metrics=[])
    if opt == "adagradp":
        for grp in m.optim.param_groups:
            for p in grp["params"]:
                m.optim.state[p]["sum"].fill_(0.05)
    m.train()
    losses = []
    for Xb, yb in zip(g["extra"]["X_steps"], g["extra"]["y_steps"]):
        loss = m._train_step(torch.from_numpy(Xb).to(device), torch.from_numpy(yb).to(device))[0]
        losses.append(float(loss))
    return losses
