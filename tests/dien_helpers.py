"""What tests/test_dien_host.py, tests/test_gpu_dien_models.py and tests/test_gpu_gru_seq_kernel.py share: the fixture
names, the model builder and the checks against a fixture (tests/golden/dien, tools/golden/make_dien_golden.py), and the
kernel cases with their float64 reference.

Kernel inputs are chosen so that the reference arithmetic itself can hold the tolerances: weight std 0.25 for H >= 32 and
0.5 below, bias std 0.1, inputs N(0, 1), att uniform in (0, 1).  ``check_case_is_testable`` asserts on the CPU that the
float32 torch restatement of the recurrence stays within a quarter of each tolerance of the float64 one."""
import functools
import json
import os

import numpy as np
import torch

from helpers import GOLDEN_DIR, feature_columns, load_golden, max_abs

LOGIT_TOL, GRAD_TOL, TRAJ_TOL = 1e-5, 2e-5, 2e-5
OUT_TOL = 1e-5
TYPES = ["gru", "aigru", "agru", "augru"]
PLAIN = ["dien_" + t for t in TYPES]
NEGS = ["dien_%s_neg" % t for t in TYPES]
ALL = PLAIN + NEGS + ["dien_one", "dien_t50", "dien_extra_varlen", "dien_nosoftmax_sigmoid", "dien_default_adam", "fit_dien"]
STEPS = ["dien_gru", "dien_augru"]
MODES = {"GRU": 0, "AIGRU": 1, "AGRU": 2, "AUGRU": 3}


def build_dien(spec, device, l2=0.0):
    from deepctr_torch.models import DIEN
    return DIEN(feature_columns(spec["dnn_columns"]), spec["history_feature_list"], l2_reg_embedding=l2, device=device,
                **spec["kwargs"])


def loaded(name, device, l2=0.0):
    g = load_golden("dien/" + name)
    m = build_dien(g["spec"], device, l2=l2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()})
    return g, m


def gru_type(g):
    return g["spec"]["kwargs"].get("gru_type", "GRU")


def expected_calls(g, grad):
    """the recurrence launches of one forward (and backward) in mock_dien's notation"""
    gt, k = gru_type(g), int(bool(grad))
    fwd = ["gru_fwd:0:%d" % k] + (["gru_fwd:0:%d" % k] if gt == "GRU" else ["gru_fwd:%d:%d" % (MODES[gt], k)])
    bwd = (["gru_bwd:0", "gru_bwd:0"] if gt == "GRU" else ["gru_bwd:%d" % MODES[gt], "gru_bwd:0"]) if grad else []
    return fwd + bwd


def init_configs():
    path = os.path.join(GOLDEN_DIR, "dien", "init.npz")
    if not os.path.exists(path):
        return []
    z = np.load(path, allow_pickle=False)
    out = []
    for i, spec in enumerate(json.loads(str(z["configs"]))):
        pre = "%d/param/" % i
        out.append((spec, {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}))
    return out


def check_forward(g, m, device):
    m.train()
    cap = {}
    h = m.out.register_forward_pre_hook(lambda mod, inp: cap.__setitem__("logit", inp[0].detach()))
    with torch.no_grad():
        y = m(torch.from_numpy(g["X"]).to(device))
    h.remove()
    m.model_plan().check_ids()
    e1, e2 = max_abs(cap["logit"].cpu().numpy(), g["logit"]), max_abs(y.cpu().numpy(), g["y_pred"])
    aux, ref = m.aux_loss.detach().cpu().numpy().reshape(-1), g["extra"]["aux_loss"].reshape(-1)
    print("logit %.3e y_pred %.3e aux %.6f (ref %.6f)" % (e1, e2, float(aux[0]), float(ref[0])))
    assert e1 <= LOGIT_TOL and e2 <= LOGIT_TOL
    assert abs(float(aux[0]) - float(ref[0])) <= 1e-5 * max(1.0, abs(float(ref[0])))


def grad_scale(key, grads, spec):
    """The gradient bound's scale: max|g_ref| of the parameter, no floor.  One exception, by reasoning and not by result
    (din_helpers.grad_scale has the argument): under ``att_weight_normalization`` -- DIEN's default -- the scores pass
    through a softmax, the exact gradient of the attention's ``dense.bias`` is 0, the reference's own value is the
    rounding noise of a sum that cancels, and ``dense.weight``'s scale is used."""
    if spec["kwargs"].get("att_weight_normalization", True) and key.endswith("attention.local_att.dense.bias"):
        key = key[:-len("bias")] + "weight"
    return float(np.max(np.abs(grads[key])))


def check_gradients(g, m, device):
    """the gradients of BCE(sum) + aux_loss, the objective the fixture differentiated"""
    m.train()
    y = m(torch.from_numpy(g["X"]).to(device)).squeeze(1)
    loss = torch.nn.functional.binary_cross_entropy(y, torch.from_numpy(g["y"]).to(device), reduction="sum")
    m.zero_grad()
    (loss + m.aux_loss).sum().backward()
    assert abs(loss.item() - g["loss"]) <= 1e-4 * max(1.0, abs(g["loss"]))
    assert set(g["grads"]) == set(k for k, _ in m.named_parameters())
    for k, p in m.named_parameters():
        ref = g["grads"][k]
        got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        err, scale = max_abs(got, ref), grad_scale(k, g["grads"], g["spec"])
        print("%-60s max|d|=%.3e max|g_ref|=%.3g" % (k, err, scale))
        assert err <= GRAD_TOL * scale, "%s: max|d|=%.3e max|g_ref|=%.3g" % (k, err, scale)


NOISE = 1e-5


def noise_mask(key, g):
    """Elements of an attention-net parameter whose gradient in the fixture is at rounding-noise level, or None.

    Under ``att_weight_normalization`` a sample's scores pass through a softmax, which ignores a shift of all of them.  The
    exact gradient is therefore 0 for ``dense.bias`` and for whatever only shifts a sample's scores together (the bias of a
    unit that is active at every position, its weights on query-only inputs): what either implementation computes there is
    the rounding noise of a sum that cancels.  Adam's first steps are ``lr * g / (|g| + eps)``: such an element moves by up
    to lr per step in the direction the noise happens to have, in the reference as here, and it moves nothing else (the
    shift it causes cancels in the softmax).  An element counts as noise when the fixture's own float32 gradient of it is
    below NOISE = 1e-5 of the largest in its tensor (``dense.bias``: of ``dense.weight``'s): about 170 float32 roundings of
    that largest term, what a cancelling sum over the batch's positions leaves.  Every other element has a real gradient
    and is held to TRAJ_TOL."""
    if not g["spec"]["kwargs"].get("att_weight_normalization", True) or ".attention.local_att." not in key:
        return None
    ref = np.abs(g["grads"][key])
    return ref <= NOISE * grad_scale(key, g["grads"], g["spec"])


def check_trajectory(g, m, device, opt, lr=1e-3, steps=3):
    """3 steps of the model's own train step against ``<opt>3/<key>`` and ``<opt>3_loss``: every element within TRAJ_TOL;
    in the adam run the elements ``noise_mask`` names within ``steps * lr``, all that can be said of them"""
    m.compile("adagrad" if opt == "adagradp" else opt, "binary_crossentropy", metrics=[])
    if opt == "adagradp":
        for grp in m.optim.param_groups:
            for p in grp["params"]:
                m.optim.state[p]["sum"].fill_(0.05)
    m.train()
    ex = g["extra"]
    losses = [float(m._train_step(torch.from_numpy(Xb).to(device), torch.from_numpy(yb).to(device))[0])
              for Xb, yb in zip(ex["X_steps"], ex["y_steps"])]
    np.testing.assert_allclose(losses, ex[opt + "3_loss"], rtol=2e-5)
    sd = m.state_dict()
    n, bad = 0, []
    for k, v in ex.items():
        if k.startswith(opt + "3/"):
            key = k[len(opt) + 2:]
            d = np.abs(sd[key].cpu().numpy().astype(np.float64) - v)
            mask = noise_mask(key, g) if (opt == "adam" and key in g["grads"]) else None
            if mask is not None and mask.any():
                print("%-70s %.3e (and %d noise elements: %.3e)" % (k, d[~mask].max() if (~mask).any() else 0.0,
                                                                    int(mask.sum()), d[mask].max()))
                if d[mask].max() > steps * lr * (1 + 1e-3):
                    bad.append("%s (noise elements): %.3e" % (k, d[mask].max()))
                d = d[~mask]
            else:
                print("%-70s %.3e" % (k, d.max() if d.size else 0.0))
            if d.size and d.max() > TRAJ_TOL:
                bad.append("%s: %.3e" % (k, d.max()))
            n += 1
    assert not bad, bad
    assert n == len(sd)


def fit_inputs(g):
    from deepctr_torch.inputs import build_input_features
    fi = build_input_features(feature_columns(g["spec"]["dnn_columns"]))
    X = g["extra"]["fit_X"]
    return {n: (X[:, lo] if hi - lo == 1 else X[:, lo:hi]) for n, (lo, hi) in fi.items()}


def check_fit(g, m, tag, opt, shuffle):
    ex = g["extra"]
    m.compile(opt, "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    x = fit_inputs(g)
    torch.manual_seed(777)
    hist = m.fit(x, ex["fit_y"], batch_size=64, epochs=3, verbose=2, validation_split=0.25, shuffle=shuffle)
    ref = {k[len("fit_%s_hist/" % tag):]: v for k, v in ex.items() if k.startswith("fit_%s_hist/" % tag)}
    assert set(hist.history) == set(ref)
    for k, v in ref.items():
        if k.endswith("auc"):
            np.testing.assert_allclose(hist.history[k], v, atol=5e-3, err_msg=k)
        else:
            np.testing.assert_allclose(hist.history[k], v, rtol=2e-4, err_msg=k)
    pred = m.predict(x, batch_size=50)
    assert pred.dtype == np.float64 and pred.shape == ex["fit_%s_pred" % tag].shape
    assert max_abs(pred, ex["fit_%s_pred" % tag]) <= 5e-5
    return hist


# ---- the recurrence itself: cases of the kernel test and their float64 reference ---------------------------------------
def recurrence(x, att, n, params, mode):
    """The formulas of include/dctr.h as a cell loop in torch, in the dtype of its operands: x [B, T, H], att [B, T] | None,
    n [B] (already clamped), params packed -> (states [B, T, H], last [B, H])"""
    B, T, H = x.shape
    Wi, Wh = params[:3 * H * H].reshape(3 * H, H), params[3 * H * H:6 * H * H].reshape(3 * H, H)
    bi, bh = params[6 * H * H:6 * H * H + 3 * H], params[6 * H * H + 3 * H:]
    h = x.new_zeros((B, H))
    zero, out = h, []
    for t in range(T):
        a = att[:, t:t + 1] if att is not None else None
        xt = x[:, t] * a if mode == 1 else x[:, t]
        gi, gh = xt @ Wi.t() + bi, h @ Wh.t() + bh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        c = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        if mode in (0, 1):
            new = (1 - z) * c + z * h
        elif mode == 2:
            new = (1 - a) * h + a * c
        else:
            u = a * z
            new = (1 - u) * h + u * c
        on = (t < n).reshape(-1, 1)
        h = torch.where(on, new, h)
        out.append(torch.where(on, new, zero))
    return torch.stack(out, dim=1), h


# name -> (dims, T, B, mode, lens | None (drawn from -1..T+3), outputs, layout)
CASES = {}


def _case(name, dims, T, B, mode, lens=None, outputs="both", layout="contig", ld_extra=0):
    CASES[name] = dict(name=name, dims=tuple(dims), T=T, B=B, mode=mode, lens=lens, outputs=outputs, layout=layout,
                       ld_extra=ld_extra)


for _m in range(4):
    _case("one_m%d" % _m, (1,), 1, 1, _m, lens=[1])
    _case("h5_t7_m%d" % _m, (5,), 7, 11, _m)
    # the model's in-row layout: segments 8 + 4 read in place from a wider row, ld_x > width
    _case("row12_t4_m%d" % _m, (8, 4), 4, 9, _m, lens=[-1, 0, 1, 3, 3, 4, 7, 2, 4], layout="row")
    _case("h33_t50_m%d" % _m, (33,), 50, 20, _m)
_case("h64_t1", (64,), 1, 7, 1, lens=[1, 0, 1, 4, -2, 1, 1])
_case("h32_t50", (32,), 50, 40, 3)
_case("corner_m0", (64,), 128, 48, 0)
_case("corner_m3", (64,), 128, 48, 3)
# H = 12 runs 16 (forward) / 32 (backward) samples per tile: a whole tile of length 0 next to one of length T
_case("tilezero", (12,), 6, 70, 3, lens=[0] * 32 + [6] * 2 + [0] * 30 + [3, 6, 1, 0, 6, 2])
_case("allzero", (12,), 6, 35, 2, lens=[0, -1, 0, 0, -5] * 7)
_case("b4100", (12,), 6, 4100, 3)
# H = 33 runs 8 samples per backward tile: 513 tiles over 512 workgroups, so workgroup 0 takes a second tile
_case("tiles513", (33,), 3, 4100, 3)
for _o in ("states", "last"):
    _case("row12_%s_m0" % _o, (8, 4), 4, 9, 0, lens=[-1, 0, 1, 3, 3, 4, 7, 2, 4], outputs=_o, layout="row")
    _case("row12_%s_m3" % _o, (8, 4), 4, 9, 3, lens=[-1, 0, 1, 3, 3, 4, 7, 2, 4], outputs=_o, layout="row")
_case("strided_states", (5,), 7, 11, 3, ld_extra=5)


def case_inputs(c):
    """numpy operands of a case (float32 / int32), deterministic per name"""
    rng = np.random.RandomState(sum(map(ord, c["name"])))
    dims, T, B = c["dims"], c["T"], c["B"]
    H = sum(dims)
    wstd = 0.25 if H >= 32 else 0.5
    params = np.concatenate([rng.normal(0, wstd, 6 * H * H), rng.normal(0, 0.1, 6 * H)]).astype(np.float32)
    x = rng.normal(0, 1, (B, T, H)).astype(np.float32)
    att = rng.uniform(0.02, 0.98, (B, T)).astype(np.float32)
    lens = np.asarray(c["lens"], np.int32) if c["lens"] is not None else rng.randint(-1, T + 4, B).astype(np.int32)
    assert lens.shape == (B,)
    return dict(params=params, x=x, att=att, lens=lens, g_states=rng.normal(0, 1, (B, T, H)).astype(np.float32),
                g_last=rng.normal(0, 1, (B, H)).astype(np.float32))


def _reference(c, dtype):
    a = case_inputs(c)
    T = c["T"]
    x = torch.from_numpy(a["x"]).to(dtype).requires_grad_(True)
    att = torch.from_numpy(a["att"]).to(dtype).requires_grad_(True)
    params = torch.from_numpy(a["params"]).to(dtype).requires_grad_(True)
    n = torch.from_numpy(np.clip(a["lens"].astype(np.int64), 0, T))
    states, last = recurrence(x, att if c["mode"] else None, n, params, c["mode"])
    obj = 0
    if c["outputs"] in ("both", "states"):
        obj = obj + (states * torch.from_numpy(a["g_states"]).to(dtype)).sum()
    if c["outputs"] in ("both", "last"):
        obj = obj + (last * torch.from_numpy(a["g_last"]).to(dtype)).sum()
    gx, ga, gp = torch.autograd.grad(obj, [x, att, params], allow_unused=True)
    z = lambda g, like: (g if g is not None else torch.zeros_like(like)).detach().numpy().astype(np.float64)  # noqa: E731
    return dict(states=states.detach().numpy().astype(np.float64), last=last.detach().numpy().astype(np.float64),
                gx=z(gx, x), g_att=z(ga, att), g_params=z(gp, params))


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 values of a case: computed once, shared, never written to"""
    r = _reference(CASES[name], torch.float64)
    for v in r.values():
        v.setflags(write=False)
    return r


BOUNDS = dict(states=OUT_TOL, last=OUT_TOL, gx=GRAD_TOL, g_att=GRAD_TOL, g_params=GRAD_TOL)


def deviations(got, ref):
    """{tensor: (max|got - ref|, max|ref|)}"""
    return dict((k, (max_abs(np.asarray(got[k], np.float64), ref[k]), float(np.max(np.abs(ref[k]))) if ref[k].size else 0.0))
                for k in BOUNDS if k in got and got[k] is not None)


def check_case_is_testable(name):
    """float32 torch against float64 torch: within a QUARTER of each tolerance, so the tolerance tests the kernel and not
    the arithmetic"""
    dev = deviations(_reference(CASES[name], torch.float32), reference(name))
    for k, (err, scale) in dev.items():
        assert err <= 0.25 * BOUNDS[k] * scale, "%s %s: fp32 torch deviates %.3e from float64 at scale %.3g" % (
            name, k, err, scale)
    return dev
