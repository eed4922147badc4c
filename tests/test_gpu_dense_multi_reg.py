"""GPU: dctr_dense_opt_multi_reg (csrc/head.hip) -- the multi-tensor Adam / RMSprop step with a device-side step count --
through the C ABI: against a float64 restatement of the step kept in this file, against torch.optim.Adam / RMSprop on
the same device tensors, the counter protocol (read, not advanced), a hipGraph replay of kernel + increment, and the
argument checks.

The bar (the AFN rule of this project: no exact bar for Adam is derivable, so torch's own step sets the margin): per
tensor, the kernel's deviation from the float64 step may be at most 4 x the deviation of torch's own float32 step from
float64 on the same inputs, with a floor of one ulp of the tensor's largest magnitude.  Every step is judged from the
float32 values it started from, so the figures are single-step roundings, not drift."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

DEV = "cuda:0"
LR, EPS, B1, B2, ALPHA, L2 = 1e-3, 1e-8, 0.9, 0.999, 0.99, 1e-3
SHAPES = [(1,), (3,), (7, 5), (4097,), (128, 65), (1000,)] + [(17 + i,) for i in range(54)]   # 60 tensors: two launches
PAD = 8         # floats of NaN in front of and behind every view
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "adam_autograd_step.json")


def _numel(s):
    return int(np.prod(s))


def _offs(i, what):
    """every third parameter / state view starts 4 bytes off 16-byte alignment, every fourth gradient: some tensors take
    the vector path, some the per-element path because of one operand only"""
    if what == "g":
        return 1 if i % 4 == 0 else 0
    return 1 if i % 3 == 0 else 0


def _inputs(seed, start, device):
    """-> (params, states1, states2, grads[3]) as float32 numpy arrays; fixed by the seed.  Gradients scaled 0.1 / 1 /
    10; magnitudes below 1e-6 are pushed out to 1e-6 (RMSprop from a zero accumulator moves by lr * g / (|g|/10 + eps):
    well conditioned only away from eps).  start != 0: the second moment preset to 0.05, the first to small values."""
    r = np.random.RandomState(seed)
    P = [r.randn(*s).astype(np.float32) for s in SHAPES]
    G = []
    for k in range(3):
        row = []
        for s in SHAPES:
            g = (r.randn(*s) * 10.0 ** (k - 1)).astype(np.float32)
            g = np.where(np.abs(g) < 1e-6, np.float32(1e-6), g).astype(np.float32)
            row.append(g)
        G.append(row)
    if start:
        S1 = [(0.01 * r.randn(*s)).astype(np.float32) for s in SHAPES]
        S2 = [np.full(s, 0.05, np.float32) for s in SHAPES]
    else:
        S1 = [np.zeros(s, np.float32) for s in SHAPES]
        S2 = [np.zeros(s, np.float32) for s in SHAPES]
    return P, S1, S2, G


def step64(kind, p, g, s1, s2, T, l2):
    """ONE optimizer step in float64 from float32 inputs (torch.optim.Adam / RMSprop, no weight_decay; the L2 term
    lambda * sum(p^2) enters as 2 lambda p): -> (p, s1, s2)."""
    p, g = p.astype(np.float64), g.astype(np.float64)
    g = g + 2.0 * l2 * p
    if kind == "adam":
        m = B1 * s1.astype(np.float64) + (1.0 - B1) * g
        v = B2 * s2.astype(np.float64) + (1.0 - B2) * g * g
        p = p - (LR / (1.0 - B1 ** T)) * m / (np.sqrt(v) / np.sqrt(1.0 - B2 ** T) + EPS)
        return p, m, v
    v = ALPHA * s1.astype(np.float64) + (1.0 - ALPHA) * g * g
    p = p - LR * g / (np.sqrt(v) + EPS)
    return p, v, None


def _torch_optim(kind, params):
    if kind == "adam":
        return torch.optim.Adam(params, lr=LR, betas=(B1, B2), eps=EPS)
    return torch.optim.RMSprop(params, lr=LR, alpha=ALPHA, eps=EPS)


def _torch_run(kind, with_l2, start, device):
    """torch's own float32 trajectory on ``device`` and, per step and tensor, its deviation from the float64 step taken
    from the float32 values the step started from: -> dev[step][i] = (d_param, d_s1, d_s2), finite flag."""
    P, S1, S2, G = _inputs(11, start, device)
    ref = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(device)) for p in P]
    optim = _torch_optim(kind, ref)
    keys = ("exp_avg", "exp_avg_sq") if kind == "adam" else ("square_avg",)
    for i, r in enumerate(ref):              # the state as a loaded checkpoint leaves it
        st = optim.state[r]
        st["step"] = torch.tensor(float(start))
        st[keys[0]] = torch.from_numpy((S1[i] if kind == "adam" else S2[i]).copy()).to(device)
        if kind == "adam":
            st[keys[1]] = torch.from_numpy(S2[i].copy()).to(device)
    devs, finite = [], True
    for k in range(3):
        before = [(r.detach().cpu().numpy().copy(),) + tuple(optim.state[r][key].cpu().numpy().copy() for key in keys)
                  for r in ref]
        for i, r in enumerate(ref):
            g = torch.from_numpy(G[k][i]).to(device)
            l2 = L2 if (with_l2 and i % 2 == 0) else 0.0
            # what autograd leaves in .grad for loss + lambda * sum(p^2): the main gradient plus 2 lambda p
            r.grad = g + (2.0 * l2) * r.detach() if l2 else g.clone()
        optim.step()
        row = []
        for i, r in enumerate(ref):
            l2 = L2 if (with_l2 and i % 2 == 0) else 0.0
            b = before[i]
            p64, a64, b64 = step64(kind, b[0], G[k][i], b[1], b[2] if kind == "adam" else None, start + k + 1, l2)
            got = [r.detach().cpu().numpy()] + [optim.state[r][key].cpu().numpy() for key in keys]
            finite = finite and all(np.isfinite(x).all() for x in got)
            d = [float(np.max(np.abs(got[0].astype(np.float64) - p64))),
                 float(np.max(np.abs(got[1].astype(np.float64) - a64)))]
            d.append(float(np.max(np.abs(got[2].astype(np.float64) - b64))) if kind == "adam" else 0.0)
            row.append(tuple(d))
        devs.append(row)
    return devs, finite


def _ulp(x):
    return float(np.spacing(np.float32(max(float(np.max(np.abs(x))), 1e-30))))


class _Views(object):
    """p / g / s1 / s2 of every tensor as views into NaN-filled base buffers"""

    def __init__(self, kind, start, seed=11):
        self.kind = kind
        P, S1, S2, G = _inputs(seed, start, DEV)
        self.G = G
        self.base = {}
        self.v = {}
        init = {"p": P, "s1": S1 if kind == "adam" else S2, "s2": S2, "g": G[0]}
        for what in ("p", "g", "s1", "s2"):
            self.base[what], self.v[what] = [], []
            for i, s in enumerate(SHAPES):
                n, off = _numel(s), PAD + _offs(i, what)
                b = torch.full((n + 2 * PAD + 1,), float("nan"), device=DEV)
                view = b[off:off + n].view(s)
                view.copy_(torch.from_numpy(init[what][i]))
                self.base[what].append(b)
                self.v[what].append(view)

    def set_grads(self, k):
        for i, view in enumerate(self.v["g"]):
            view.copy_(torch.from_numpy(self.G[k][i]))

    def items(self, L, with_l2, lo=0, hi=None):
        idx = list(range(len(SHAPES)))[lo:hi]
        items = (L.DenseItem2 * len(idx))()
        for j, i in enumerate(idx):
            items[j].p, items[j].g = self.v["p"][i].data_ptr(), self.v["g"][i].data_ptr()
            items[j].s1 = self.v["s1"][i].data_ptr()
            items[j].s2 = self.v["s2"][i].data_ptr() if self.kind == "adam" else None
            items[j].n = _numel(SHAPES[i])
            items[j].l2 = L2 if (with_l2 and i % 2 == 0) else 0.0
        return items

    def snapshot(self):
        return [tuple(self.v[w][i].cpu().numpy().copy() for w in ("p", "s1", "s2")) for i in range(len(SHAPES))]

    def bits(self):
        return [b.clone() for w in ("p", "s1", "s2") for b in self.base[w]]

    def nans_in_place(self):
        for what in ("p", "g", "s1", "s2"):
            for i, (b, s) in enumerate(zip(self.base[what], SHAPES)):
                n, off = _numel(s), PAD + _offs(i, what)
                if not (torch.isnan(b[:off]).all() and torch.isnan(b[off + n:]).all()):
                    return False
                if what != "g" and not (what == "s2" and self.kind != "adam") and not torch.isfinite(b[off:off + n]).all():
                    return False
        return True


def _opt(L, kind):
    from deepctr_torch._hip.plan import LazyState
    o = L.LazyOpt()
    keep = None
    if kind == "adam":
        o.kind, o.lr, o.eps, o.beta1, o.beta2 = L.LAZY_ADAM, LR, EPS, B1, B2
        o.beta1_c, o.beta2_c = 1 - B1, 1 - B2
        ss, bc, _ = LazyState.adam_tables(LR, B1, B2)
        keep = (torch.from_numpy(ss).to(DEV), torch.from_numpy(bc).to(DEV))
        o.adam_ss, o.n_ss, o.adam_bc, o.n_bc = keep[0].data_ptr(), keep[0].numel(), keep[1].data_ptr(), keep[1].numel()
    else:
        o.kind, o.lr, o.eps, o.beta1, o.beta2 = L.LAZY_RMSPROP, LR, EPS, 1 - ALPHA, ALPHA
    return o, keep


def _call(L, items, n, o, step, stream=None):
    return L.lib().dctr_dense_opt_multi_reg(items, n, ctypes.byref(o) if o is not None else None,
                                            ctypes.c_void_p(step.data_ptr()) if step is not None else None,
                                            stream if stream is not None else L.stream_handle(DEV))


def _inc(L, step, stream=None):
    L.check(L.lib().dctr_lazy_step_inc(ctypes.c_void_p(step.data_ptr()), stream if stream is not None else L.stream_handle(DEV)))


_TORCH_CPU = {}


def _cpu_margin(kind, with_l2, start):
    key = (kind, with_l2, start)
    if key not in _TORCH_CPU:
        _TORCH_CPU[key] = _torch_run(kind, with_l2, start, "cpu")
    return _TORCH_CPU[key]


@pytest.mark.parametrize("start", [0, 7])
@pytest.mark.parametrize("with_l2", [False, True])
@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_inputs_keep_torch_itself_within_1e5_of_float64(kind, with_l2, start):
    """CPU: the chosen inputs are well conditioned -- torch's own float32 step stays finite and within 1e-5 of the
    float64 step on every tensor, so its deviation is a usable margin for the GPU cases below."""
    devs, finite = _cpu_margin(kind, with_l2, start)
    assert finite
    worst = max(max(d) for row in devs for d in row)
    assert worst <= 1e-5, "torch's float32 step is %.3e from float64" % worst


def _record(tag, value):
    """the largest ratio seen on the GPU goes into profiles/adam_autograd_step.json when DCTR_WRITE_PROFILE is set"""
    if os.environ.get("DCTR_WRITE_PROFILE", "0") != "1":
        return
    doc = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as f:
            doc = json.load(f)
    doc.setdefault("abi_test_ratios", {})[tag] = value
    with open(PROFILE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)


@pytest.mark.gpu
@pytest.mark.parametrize("start", [0, 7])
@pytest.mark.parametrize("with_l2", [False, True])
@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_three_steps_against_float64_and_torch(kind, with_l2, start):
    from deepctr_torch._hip import lib as L
    tdev, finite = _torch_run(kind, with_l2, start, DEV)
    assert finite
    V = _Views(kind, start)
    o, keep = _opt(L, kind)
    step = torch.full((1,), start, dtype=torch.int32, device=DEV)
    items = V.items(L, with_l2)
    worst_ratio, floor_decided = 0.0, 0
    names = ("param", "s1", "s2") if kind == "adam" else ("param", "s1")
    for k in range(3):
        V.set_grads(k)
        before = V.snapshot()
        L.check(_call(L, items, len(SHAPES), o, step), "dctr_dense_opt_multi_reg")
        assert int(step.item()) == start + k               # read, not advanced
        _inc(L, step)
        assert int(step.item()) == start + k + 1
        after = V.snapshot()
        for i in range(len(SHAPES)):
            l2 = L2 if (with_l2 and i % 2 == 0) else 0.0
            b = before[i]
            want = step64(kind, b[0], V.G[k][i], b[1], b[2] if kind == "adam" else None, start + k + 1, l2)
            for j, name in enumerate(names):
                got = after[i][j]
                assert np.isfinite(got).all()
                d = float(np.max(np.abs(got.astype(np.float64) - want[j])))
                ulp = _ulp(want[j])
                bar = max(4.0 * tdev[k][i][j], ulp)
                print("%s l2=%d start=%d step %d tensor %d %s: kernel %.3e torch %.3e ulp %.3e" %
                      (kind, with_l2, start, k, i, name, d, tdev[k][i][j], ulp))
                assert d <= bar, "%s step %d tensor %d %s: |kernel - f64| %.3e > max(4 x %.3e, ulp %.3e)" % (
                    kind, k, i, name, d, tdev[k][i][j], ulp)
                if tdev[k][i][j] > 0:
                    worst_ratio = max(worst_ratio, d / tdev[k][i][j])
                if d > 4.0 * tdev[k][i][j]:
                    floor_decided += 1
    assert V.nans_in_place(), "something was written outside the views"
    _record("%s_l2%d_start%d" % (kind, int(with_l2), start), {"max_ratio_kernel_over_torch": worst_ratio,
                                                           "cases_decided_by_the_ulp_floor": floor_decided})


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_counter_is_read_not_advanced_and_calls_repeat_bit_for_bit(kind):
    from deepctr_torch._hip import lib as L
    o, keep = _opt(L, kind)
    A, B = _Views(kind, 7), _Views(kind, 7)
    step = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    L.check(_call(L, A.items(L, True), len(SHAPES), o, step))
    assert int(step.item()) == 7
    L.check(_call(L, B.items(L, True), len(SHAPES), o, step))       # same step number: same bits
    assert int(step.item()) == 7
    for x, y in zip(A.bits(), B.bits()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    _inc(L, step)
    assert int(step.item()) == 8
    # the two launches of the 60-tensor list read ONE step number: tensor 59 (second launch) equals what the same tensor
    # gets as a one-item list at the same counter
    C = _Views(kind, 7)
    step.fill_(7)
    L.check(_call(L, C.items(L, True, 59, 60), 1, o, step))
    assert torch.equal(C.v["p"][59], A.v["p"][59]) and torch.equal(C.v["s1"][59], A.v["s1"][59])
    if kind == "adam":
        # ... and the step number matters: at another count the parameters differ (bias correction)
        D = _Views(kind, 7)
        step.fill_(0)
        L.check(_call(L, D.items(L, True, 59, 60), 1, o, step))
        assert not torch.equal(D.v["p"][59], A.v["p"][59])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_graph_replay_equals_eager_steps(kind):
    """ONE captured step (kernel + increment), replayed 5 times with fresh gradients copied into the static gradient
    views, against 5 eager calls: bit-equal parameters and state.  With beta1 = 0.9 a frozen step number would change the
    first step sizes by tens of percent."""
    from deepctr_torch._hip import lib as L
    o, keep = _opt(L, kind)
    E, R = _Views(kind, 0), _Views(kind, 0)
    r = np.random.RandomState(5)
    fresh = [[torch.from_numpy(np.where(np.abs(g) < 1e-6, 1e-6, g).astype(np.float32)).to(DEV)
              for g in [r.randn(*s).astype(np.float32) for s in SHAPES]] for _ in range(5)]
    step_e = torch.zeros((1,), dtype=torch.int32, device=DEV)
    step_r = torch.zeros((1,), dtype=torch.int32, device=DEV)
    items_e, items_r = E.items(L, True), R.items(L, True)
    for k in range(5):
        for view, g in zip(E.v["g"], fresh[k]):
            view.copy_(g)
        L.check(_call(L, items_e, len(SHAPES), o, step_e))
        _inc(L, step_e)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.graph(graph, stream=side):
        h = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
        L.check(_call(L, items_r, len(SHAPES), o, step_r, h))
        _inc(L, step_r, h)
    for k in range(5):
        for view, g in zip(R.v["g"], fresh[k]):
            view.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert int(step_r.item()) == int(step_e.item()) == 5
    for x, y in zip(E.bits(), R.bits()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert R.nans_in_place()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["adam", "rmsprop", "adagrad"])
def test_argument_checks_refuse_and_touch_nothing(kind):
    from deepctr_torch._hip import lib as L
    k2 = "rmsprop" if kind == "adagrad" else kind
    o, keep = _opt(L, k2)
    if kind == "adagrad":
        o.kind = L.LAZY_ADAGRAD
    V = _Views(k2, 7)
    step = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    before = V.bits()
    n = len(SHAPES)

    def refused(rc):
        assert rc == L.EINVAL, rc
        torch.cuda.synchronize()
        for x, y in zip(before, V.bits()):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "a refused call wrote something"
        assert int(step.item()) == 7

    refused(_call(L, V.items(L, True), n, None, step))
    refused(_call(L, V.items(L, True), n, o, None))
    bad = L.LazyOpt()
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(o), ctypes.sizeof(o))
    bad.kind = 9
    refused(_call(L, V.items(L, True), n, bad, step))
    refused(L.lib().dctr_dense_opt_multi_reg(None, 3, ctypes.byref(o), ctypes.c_void_p(step.data_ptr()), L.stream_handle(DEV)))
    refused(_call(L, V.items(L, True), -1, o, step))
    fields = ["p", "g", "s1"] + (["s2"] if kind == "adam" else [])
    for f in fields:
        for at in (0, 55):             # in the first launch's part of the list and in the second's: nothing runs either way
            items = V.items(L, True)
            setattr(items[at], f, None)
            refused(_call(L, items, n, o, step))
    items = V.items(L, True)
    items[50].n = -1
    refused(_call(L, items, n, o, step))
    # nothing to do is fine: an empty list, a list of empty tensors (their pointers may be NULL)
    assert _call(L, V.items(L, True), 0, o, step) == 0
    assert L.lib().dctr_dense_opt_multi_reg(None, 0, ctypes.byref(o), ctypes.c_void_p(step.data_ptr()), L.stream_handle(DEV)) == 0
    items = V.items(L, True, 0, 3)
    for j in range(3):
        items[j].n = 0
        items[j].p = items[j].g = items[j].s1 = items[j].s2 = None
    assert _call(L, items, 3, o, step) == 0
    torch.cuda.synchronize()
    for x, y in zip(before, V.bits()):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    if kind != "adam":
        # a kind without a second moment ignores s2
        items = V.items(L, True)
        for j in range(n):
            items[j].s2 = None
        assert _call(L, items, n, o, step) == 0
        torch.cuda.synchronize()
        assert V.nans_in_place()
