"""Driver for the DNN tower and its fused train step THROUGH THE C ABI (include/dctr.h: dctr_mlp_fwd, dctr_mlp_bwd,
dctr_mlp_train_step, dctr_mlp_train_wgrad and the two workspace sizes), shared by tests/test_tower_abi_host.py (over the
stand-in library, on the CPU) and tests/test_gpu_tower_abi.py (on the device).  Not a test file.

A ``TowerCase`` builds ``dctr_mlp_t`` by hand and owns ONE float32 arena (tests/lazy_abi.py's, the sentinel 777 of
tests/interaction_abi.py in front of, behind and between all buffers):

  three flat slabs   parameters | gradients | Adagrad state, one layout: W_l [N, ld_w] with ld_w = r4(K_l) + 4, bias_l,
                     w_out, the head's bias -- what ``dctr_dense_step_t``'s grad_base / param_base / state_base address.  W's
                     pad columns [K_l, ld_w) hold 777 (finite, non-zero: what the header permits), the gradient slab is all
                     777 before a call.
  x                  ld_x = r4(K) + 4, 777 in [K, ld_x);  h, dh: ld_h = r4(N) + 4;  gx: ld_gx = r4(K) + 4;  g without w_out:
                     ld_g = r4(N) + 4;  part0, part1, y, y_pred, g_logit, loss, logit: all outputs pre-filled with 777.
  workspace          exactly the advertised floats (``bwd`` cases: dctr_mlp_bwd_workspace_floats, ``train`` cases:
                     dctr_mlp_train_workspace_floats), NaN inside, a guard behind.
  two models         include/dctr.h's contract in float64 (``ref``) and the same statement in plain float32 numpy (``ref32``):
                     tower forward, the head of the dctr_bce_head comment (logs clamped at -100, the 1e-12 floor), backward,
                     weight gradients, SGD / Adagrad as the dctr_dense_step_t comment states them.

After every call ``_verify`` asserts
  (a) every float of the arena outside what the header says the call writes keeps its bits: guards, inputs, the pad columns
      of x / W (also inside the parameter and state slabs after an optimizer step), a gbias whose layer has bias == NULL, h / dh
      columns [r4(N), ld_h), gx columns from round_up(K, 64), the float behind the workspace;
  (b) gW[:, K_l:ld_w) is exactly 0; gx columns [K, round_up(K, 32)) are exactly 0; h / dh columns [N, r4(N)) and gx columns
      [round_up(K, 32), round_up(K, 64)) hold 0 or what they held (include/dctr.h);
  (c) tower outputs and gradients within 1e-5 x max(1, max|ref|) (tests/test_gpu_mlp.py, tests/test_gpu_wgrad_assignment.py),
      y_pred 1e-6, g_logit 2e-6, loss 1e-5 x max(1, |ref|) (tests/test_gpu_mlp.py's head bars); plain float32 stays within a
      quarter of each of these at the same case, or the case is not comparable;
  (d) parameters and Adagrad state after the in-kernel step relative to max|ref| of the tensor within max(4 x the deviation
      of plain float32 at the same case, 4 float32 ulps) -- tests/lazy_abi.py's rule: two for the device's root / division
      against IEEE's, two for another valid summation order;
  (e) where the float64 reference is exactly zero (a relu-masked gradient, a dead unit's weight gradient, a saturated row's
      g_logit) the result is exactly zero.

Relu coin flips: a row is risky when a float64 pre-activation lies within 1e-5 x max(1, max|pre|) of zero (any layer).
dctr_mlp_bwd gives such rows g = 0; the train step gives them part0 (part1 when part0 is absent) = +40 and y = 1: p rounds
to 1, q = 0, g_logit and the loss term are exactly 0 by the head's formula.  One unmarked row has -40 and y = 0 (the 1e-12
floor under q).  At most a quarter of the rows may be risky (asserted when the inputs are prepared, from the float64 forward
alone); nothing is dropped from any comparison.

``launch_arm`` / ``wgrad_plan`` restate the launcher's host arithmetic; every case asserts the arm it was chosen for.
``WORST`` collects max|d| / scale per quantity, the kernel's and plain float32's."""
import ctypes

import numpy as np
import torch

from interaction_abi import GUARD, SENT
from lazy_abi import ULP, _Arena, _bits

F32 = np.float32
TOL, TOL_YPRED, TOL_GLOGIT, TOL_LOSS = 1e-5, 1e-6, 2e-6, 1e-5
RISK = 1e-5
SGD, ADAGRAD = 0, 1
LR = 1e-3          # (BCE summed over the batch: at 0.01 three SGD steps of a 64-row batch already leave the basin)
WORST = {}          # quantity -> [kernel ratio, float32 ratio]
SENT_BITS = int(np.array([SENT], F32).view(np.int32)[0])


def r4(n):
    return (n + 3) // 4 * 4


def _ru(x, m):
    return (x + m - 1) // m * m


# ---- the launcher's host arithmetic, restated (csrc/mlp.hip, csrc/tower_tiles.hpp) -----------------------------------------
KTM, KPAD, KKC, LDS_LIMIT = 16, 8, 512, 150 * 1024          # tower_tiles.hpp: kTM, kPad, kKC; the launchers' 150 KB


def launch_arm(K, hidden):
    """what dctr_mlp_train_step computes before it launches k_mlp_train: ``fast`` (tower_fast), ``kc`` (pick_kc), ``bwd_off``
    (0: the backward's gradient tiles alias the forward's LDS image) and the LDS sizes in bytes"""
    widths = list(hidden)
    ks = [K] + widths[:-1]
    K0p = _ru(K, 16)
    rsh = _ru(max(widths), 16) + KPAD                                # a.rsh = round_up(max_width(m), 16) + kPad
    kc = KKC                                                         # pick_kc
    while kc > 64 and KTM * (min(K0p, kc) + KPAD + 2 * rsh) * 4 > LDS_LIMIT:
        kc >>= 1
    rsx = min(K0p, kc) + KPAD                                        # a.rsx
    if K0p > kc or K0p > 512 or max(widths) > 512 or max(ks) > 512:  # tower_fast
        fast = 0
    else:
        fast = 1 if max(ks) > 256 else 2
    rsd = _ru(max(widths + ks[1:]), 64) + KPAD                       # bwd_stride
    lds_f, lds_b = KTM * (rsx + 2 * rsh) * 4, KTM * 2 * rsd * 4
    bwd_off = lds_f // 4 if lds_f + lds_b <= LDS_LIMIT else 0        # "both images fit"
    lds = lds_f + lds_b if bwd_off else max(lds_f, lds_b)
    assert lds <= LDS_LIMIT, "the launcher refuses this tower (DCTR_ENOSUP)"
    return dict(fast=fast, kc=kc, bwd_off=bwd_off, lds_f=lds_f, lds_b=lds_b, lds=lds)


def wgrad_plan(K, hidden, B, proj, ld_w):
    """plan_wgrad: S batch slices of ``bs`` rows, one slab of partials per slice"""
    ks = [K] + list(hidden[:-1])
    tiles = sum(((n + 63) // 64) * ((k + 63) // 64) for n, k in zip(hidden, ks))
    S, best = 1, -1
    for s in range(1, min(16, B // 64 if B >= 64 else 1) + 1):
        rounds = (tiles * s + (1 if proj else 0) + 255) // 256
        cost = rounds * ((B + s - 1) // s + 150)
        if best < 0 or cost < best:
            best, S = cost, s
    S = max(1, min(S, B // 64, 16))
    bs = _ru((B + S - 1) // S, 8)
    slab = sum(n * ld + r4(n) for n, ld in zip(hidden, ld_w)) + (r4(hidden[-1]) if proj else 0)
    return dict(S=S, bs=bs, slab=slab, bwd_ws=slab * S, train_ws=slab * S + 2 * ((B + KTM - 1) // KTM))


# ---- the contract, in one dtype ------------------------------------------------------------------------------------------
class Model(object):
    """include/dctr.h's tower, head, backward and dense optimizer step on numpy arrays of ``dt``"""

    def __init__(self, dt, W, bias, w_out, hbias, state, relu, kind, lr, eps):
        self.dt, self.relu, self.kind = dt, relu, kind
        c = lambda a: None if a is None else np.array(a, dt)          # noqa: E731
        self.W, self.bias, self.w_out, self.hbias = [c(w) for w in W], [c(b) for b in bias], c(w_out), c(hbias)
        self.state = dict((k, c(v)) for k, v in state.items())
        self.lr, self.eps = dt(F32(lr)), dt(F32(eps))

    def forward(self, x):
        h, pres, hs = np.array(x, self.dt), [], []
        for W, b, relu in zip(self.W, self.bias, self.relu):
            pre = h @ W.T
            if b is not None:
                pre = pre + b
            h = np.maximum(pre, 0) if relu else pre
            pres.append(pre)
            hs.append(h)
        return pres, hs, (h @ self.w_out if self.w_out is not None else None)

    def head(self, tower, p0, p1, use_bias, y):
        dt = self.dt
        z = np.zeros(len(y), dt)          # ((part0 + part1) + tower) + bias
        for p in (p0, p1):
            if p is not None:
                z = z + np.array(p, dt)
        z = z + tower
        if use_bias:
            z = z + self.hbias[0]
        t = np.array(y, dt)
        with np.errstate(divide="ignore", over="ignore"):
            p = dt(1) / (dt(1) + np.exp(-z))
            lp, l1p = np.maximum(np.log(p), dt(-100)), np.maximum(np.log(dt(1) - p), dt(-100))
        li = (t - dt(1)) * l1p - t * lp
        q = (dt(1) - p) * p
        gz = (p - t) / np.maximum(q, dt(1e-12)) * q
        return dict(z=z, y_pred=p, loss=li.sum(dtype=dt), g_logit=gz, g_bias=gz.sum(dtype=dt))

    def backward(self, x, hs, g):
        """g: [B] d loss / d logit (with w_out) or [B, N] d loss / d h_L"""
        out = {}
        g = np.array(g, self.dt)
        if self.w_out is not None:
            gh = np.outer(g, self.w_out)
            out["g_w_out"] = g @ hs[-1]
        else:
            gh = g
        for l in reversed(range(len(self.W))):
            if self.relu[l]:
                gh = np.where(hs[l] > 0, gh, 0).astype(self.dt)
            inp = np.array(x, self.dt) if l == 0 else hs[l - 1]
            out[("dh", l)], out[("gW", l)], out[("gbias", l)] = gh, gh.T @ inp, gh.sum(0)
            gh = gh @ self.W[l]
        out["gx"] = gh
        return out

    def param(self, key):
        """("W", l) | ("bias", l) | "w_out" | "hbias" -> the array"""
        return {"W": self.W, "bias": self.bias}[key[0]][key[1]] if isinstance(key, tuple) else getattr(self, key)

    def step(self, key, g):
        """dctr_dense_step_t: SGD p -= lr g; Adagrad s += g g, p -= lr g / (sqrt(s) + eps)"""
        p = self.param(key)
        g = np.asarray(g, self.dt).reshape(p.shape)
        if self.kind == ADAGRAD:
            s = self.state[key]
            s += g * g
            p -= self.lr * (g / (np.sqrt(s) + self.eps))
        else:
            p -= self.lr * g


def _state_key(key):
    return ("s",) + key if isinstance(key, tuple) else "s_" + key


def _grad_key(key):
    """the name of a parameter's gradient"""
    return ({"W": "gW", "bias": "gbias"}[key[0]], key[1]) if isinstance(key, tuple) else {"w_out": "g_w_out", "hbias": "g_bias"}[key]


class TowerCase(object):
    """see the module docstring.  ``mode``: "bwd" (dctr_mlp_fwd + dctr_mlp_bwd) or "train".  ``relu``: one flag or one per
    layer; ``no_bias`` / ``no_gW``: layers whose bias / gW is NULL; ``parts``: (part0 given, part1 given); ``x_pad``: what x's columns [K, ld_x) hold instead of 777."""

    def __init__(self, lib, dev, mode, B, K, hidden, relu=1, proj=True, no_bias=(), no_gW=(), gx=True, parts=(True, True),
                 head_bias=True, g_bias=True, opt=None, eps=1e-10, seed=0, x_pad=None):
        from deepctr_torch._hip import lib as L
        assert mode in ("bwd", "train") and (proj or mode == "bwd")
        self.L, self.lib, self.dev, self.mode = L, lib, torch.device(dev), mode
        self.B, self.K, self.hidden, self.proj = B, K, list(hidden), proj
        self.relu = [int(relu)] * len(hidden) if np.isscalar(relu) else [int(r) for r in relu]
        self.no_bias, self.no_gW, self.has_gx = set(no_bias), set(no_gW), gx
        self.parts, self.head_bias, self.has_g_bias, self.opt, self.eps = parts, head_bias, g_bias, opt, eps
        self.stream = L.stream_handle(self.dev)
        self.real = isinstance(lib, ctypes.CDLL)
        rng = self.rng = np.random.RandomState(seed)
        nl, ks = len(hidden), [K] + list(hidden[:-1])
        self.ks, self.ld_w, self.ld_h = ks, [r4(k) + 4 for k in ks], [r4(n) + 4 for n in hidden]
        self.ld_x = self.ld_gx = r4(K) + 4
        ntop = hidden[-1]
        self.ld_g = r4(ntop) + 4

        # ---- the slab layout: float offsets of every parameter inside a slab (the same in all three)
        off, lay = 0, {}
        for l, (n, ld) in enumerate(zip(hidden, self.ld_w)):
            lay[("W", l)] = off
            off += n * ld + GUARD
            lay[("bias", l)] = off
            off += r4(n) + GUARD
        lay["w_out"] = off
        off += r4(ntop) + GUARD
        lay["hbias"] = off
        off += 4
        fa = _Arena(np.float32, F32(SENT))
        self.base = dict((s, fa.alloc(1, off)[0]) for s in ("param", "grad", "state"))
        ix = self.ix = {}
        pad = self.pad = {}

        def rows(base, nr, nc, ld):
            return base + np.arange(nr)[:, None] * ld + np.arange(nc)[None, :]
        for slab, names in (("param", ("W", "bias", "w_out", "hbias")), ("grad", ("gW", "gbias", "g_w_out", "g_bias")),
                            ("state", ("s", "s", "s_w_out", "s_hbias"))):
            b0 = self.base[slab]
            for l, (n, k, ld) in enumerate(zip(hidden, ks, self.ld_w)):
                kw = (names[0], "W", l) if slab == "state" else (names[0], l)
                kb = (names[1], "bias", l) if slab == "state" else (names[1], l)
                ix[kw] = rows(b0 + lay[("W", l)], n, k, ld)
                pad[kw] = rows(b0 + lay[("W", l)] + k, n, ld - k, ld)
                ix[kb] = b0 + lay[("bias", l)] + np.arange(n)
            ix[names[2]] = b0 + lay["w_out"] + np.arange(ntop)
            ix[names[3]] = b0 + lay["hbias"] + np.arange(1)

        def buf(name, nr, nc, ld):
            base, _ = fa.alloc(nr, nc, ld)
            ix[name] = rows(base, nr, nc, ld)
            pad[name] = rows(base + nc, nr, ld - nc, ld)
            return base
        buf("x", B, K, self.ld_x)
        for l, (n, ld) in enumerate(zip(hidden, self.ld_h)):
            buf(("h", l), B, n, ld)
            buf(("dh", l), B, n, ld)
        buf("gx", B, K, self.ld_gx)
        for name in ("part0", "part1", "y", "y_pred", "g_logit", "logit"):
            ix[name] = fa.alloc(1, B)[1][0]
        ix["loss"] = fa.alloc(1, 1)[1][0]
        if proj:
            ix["g"] = fa.alloc(1, B)[1][0]
        else:
            buf("g", B, ntop, self.ld_g)

        # ---- the descriptor's shapes first: the workspace size is read from the library
        d = self.desc = L.Mlp()
        d.n_layers = nl
        for l in range(nl):
            e = d.layer[l]
            e.K, e.N, e.ld_w, e.ld_h, e.relu = ks[l], hidden[l], self.ld_w[l], self.ld_h[l], self.relu[l]
            e.W = 16          # (the size functions read shapes only; the real addresses follow)
        d.w_out = 16 if proj else None
        self.plan = wgrad_plan(K, hidden, max(B, 1), proj, self.ld_w)
        fn = lib.dctr_mlp_bwd_workspace_floats if mode == "bwd" else lib.dctr_mlp_train_workspace_floats
        self.n_ws = int(fn(ctypes.byref(d), B))
        if self.real and B > 0:
            assert self.n_ws == self.plan[mode + "_ws"], "workspace: the library says %d floats, plan_wgrad restated %d" % (
                self.n_ws, self.plan[mode + "_ws"])
        ix["ws"] = fa.alloc(1, max(self.n_ws, 1))[1][0][:self.n_ws]

        # ---- contents
        host = fa.build()
        self.x = rng.randn(B, K).astype(F32)
        W, bias = [], []
        for l, (n, k) in enumerate(zip(hidden, ks)):
            W.append((rng.randn(n, k) * np.sqrt((2.0 if self.relu[l] else 1.0) / k)).astype(F32))
            bias.append(None if l in self.no_bias else (rng.randn(n) * 0.1).astype(F32))
        w_out = (rng.randn(ntop) * 0.5 / np.sqrt(ntop)).astype(F32) if proj else None
        hbias = np.array([0.3], F32)
        state = {}
        # Adagrad state: a floor of 0.05 .. 0.15 here (starting from 0 the first step is lr * sign(g), which turns the sign of
        # a gradient element within rounding of 0 into a whole lr) + ``_seed_state``'s history
        for l in range(nl):
            state[("W", l)] = rng.uniform(0.05, 0.15, W[l].shape).astype(F32)
            state[("bias", l)] = None if bias[l] is None else rng.uniform(0.05, 0.15, hidden[l]).astype(F32)
        state["w_out"] = rng.uniform(0.05, 0.15, ntop).astype(F32) if proj else None
        state["hbias"] = np.array([0.1], F32)
        self.p0 = (rng.randn(B) * 0.5).astype(F32)
        self.p1 = (rng.randn(B) * 0.5).astype(F32)
        self.y = rng.randint(0, 2, B).astype(F32)
        self.y[0] = 1          # (a NULL head bias or an absent part read as y[0] must show)
        self.g = (rng.randn(B) * 0.1).astype(F32) if proj else (rng.randn(B, ntop) * 0.1).astype(F32)
        host[ix["x"]] = self.x
        if x_pad is not None:          # (include/dctr.h: x's row padding never enters a product)
            host[pad["x"]] = x_pad
        for l in range(nl):
            host[ix[("W", l)]] = W[l]
            host[ix[("s", "W", l)]] = state[("W", l)]
            if bias[l] is not None:
                host[ix[("bias", l)]] = bias[l]
                host[ix[("s", "bias", l)]] = state[("bias", l)]
        if proj:
            host[ix["w_out"]], host[ix["s_w_out"]] = w_out, state["w_out"]
        host[ix["hbias"]], host[ix["s_hbias"]] = hbias, state["hbias"]
        host[ix["ws"]] = np.nan
        self.fa = torch.from_numpy(host).to(self.dev)
        kind = {None: SGD, "sgd": SGD, "adagrad": ADAGRAD}[opt]
        self.ref = Model(np.float64, W, bias, w_out, hbias, state, self.relu, kind, LR, eps)
        self.ref32 = Model(np.float32, W, bias, w_out, hbias, state, self.relu, kind, LR, eps)

        # ---- the descriptor's pointers
        P = self.addr
        for l in range(nl):
            e = d.layer[l]
            e.W, e.h, e.dh = P(ix[("W", l)]), P(ix[("h", l)]), P(ix[("dh", l)])
            e.bias = None if l in self.no_bias else P(ix[("bias", l)])
            e.gW = None if l in self.no_gW else P(ix[("gW", l)])
            e.gbias = P(ix[("gbias", l)])          # (given even where bias is NULL: the launcher must not pass it on)
        if proj:
            d.w_out, d.g_w_out = P(ix["w_out"]), P(ix["g_w_out"])
        self.step = None
        if opt is not None:
            s = self.step = L.DenseStep()
            s.kind, s.lr, s.eps = kind, LR, eps
            s.grad_base, s.param_base = P(self.base["grad"]), P(self.base["param"])
            s.state_base = P(self.base["state"]) if kind == ADAGRAD else None
        self.risky = np.zeros(B, bool)
        self.sync()
        if opt == "adagrad":
            self._seed_state()

    def _seed_state(self):
        """state += 10 g0^2, g0 the float64 gradient at the initial parameters: the sum of squares after ten earlier steps on
        this batch, as tests/lazy_abi.py seeds its states (stamp x g0^2).  A state made of this run's three squares alone turns
        the state's bound into one on the gradient itself -- 4 ulps of s are 2 ulps of g, where the gradient's own bar is
        1e-5: the first device run of the 12-layer case sat there (4.83e-7 of max|s| against the floor of 4.77e-7, the
        gradient being 2 ulps off float64 after 24 matrix products; plain float32 drew 1.1e-7)."""
        self.prepare_train()
        exp = self._expect(self.ref)
        for k in self.params():
            g = np.asarray(exp[_grad_key(k)], np.float64)
            s0 = (self.ref.state[k] + 10.0 * g.reshape(self.ref.state[k].shape) ** 2).astype(F32)
            for m in (self.ref, self.ref32):
                m.state[k][...] = s0
            self.put(_state_key(k), s0)

    # ---- plumbing ------------------------------------------------------------------------------------------------------
    def addr(self, idx):
        return self.fa.data_ptr() + 4 * int(np.asarray(idx).ravel()[0] if np.ndim(idx) else idx)

    def ptr(self, name):
        return ctypes.c_void_p(self.addr(self.ix[name]) if self.ix[name].size else self.fa.data_ptr())

    def sync(self):
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)

    def snapshot(self):
        self.sync()
        return self.fa.cpu().numpy().copy()

    def put(self, name, values):
        if self.ix[name].size:
            self.fa[torch.from_numpy(self.ix[name].ravel()).to(self.dev)] = \
                torch.from_numpy(np.ascontiguousarray(values, F32).ravel()).to(self.dev)
        self.sync()

    def step_ref(self):
        return ctypes.byref(self.step) if self.step is not None else None

    def params(self):
        """keys of the parameters the optimizer step reaches: those whose gradient has a destination"""
        out = []
        for l in range(len(self.hidden)):
            if l not in self.no_gW:
                out.append(("W", l))
            if l not in self.no_bias:
                out.append(("bias", l))
        if self.proj:
            out.append("w_out")
        if self.mode == "train" and self.has_g_bias:
            out.append("hbias")
        return out

    # ---- the inputs of one call ----------------------------------------------------------------------------------------
    def _risk(self):
        pres, _, logit = self.ref.forward(self.x)
        risky = np.zeros(self.B, bool)
        for pre in pres:
            if pre.size:
                risky |= (np.abs(pre) < RISK * max(1.0, float(np.abs(pre).max()))).any(axis=1)
        assert 4 * int(risky.sum()) <= max(self.B, 1), "%d of %d rows are risky: pick another seed" % (risky.sum(), self.B)
        self.risky = risky
        return logit

    def prepare_bwd(self):
        self._risk()
        g = self.g.copy()
        g[self.risky] = 0
        self.g_now = g
        self.put("g", g)

    def prepare_train(self):
        """part0 / part1 / y of this step: +40 | y = 1 on the risky rows, -40 | y = 0 on one unmarked row"""
        logit = self._risk()
        p0, p1, y = self.p0.copy(), self.p1.copy(), self.y.copy()
        sat = p0 if self.parts[0] else p1
        if self.parts[0] or self.parts[1]:
            rows = np.flatnonzero(self.risky)
            p0[rows], p1[rows], y[rows] = 0, 0, 1
            sat[rows] = 40
            free = np.flatnonzero(~self.risky)
            if self.B >= 4 and free.size:          # (a middle row: the batch's last row is the ragged tile's, it keeps its gradient)
                mid = free[free.size // 2]
                p0[mid], p1[mid], y[mid] = 0, 0, 0
                sat[mid] = -40
            z = logit[rows] + 40 + (0.3 if self.head_bias else 0.0)
            assert not rows.size or z.min() > 37, "a risky row's logit does not saturate the float64 sigmoid"
        else:
            assert not self.risky.any(), "without part0 / part1 no row can be neutralised: pick a seed without risky rows"
        # every other row stays where the float32 sigmoid has bits left on both sides (|z| < 12: p and 1 - p above 6e-6)
        z = logit + (p0 if self.parts[0] else 0) + (p1 if self.parts[1] else 0) + (0.3 if self.head_bias else 0.0)
        plain = np.abs(np.where(self.parts[0], p0, p1)) != 40 if (self.parts[0] or self.parts[1]) else np.ones(self.B, bool)
        assert not plain.any() or np.abs(z[plain]).max() < 12, "an unmarked row's logit saturates the float32 sigmoid"
        self.p0_now = p0 if self.parts[0] else None
        self.p1_now = p1 if self.parts[1] else None
        self.y_now = y
        self.put("part0", p0)
        self.put("part1", p1)
        self.put("y", y)

    # ---- the entry points ----------------------------------------------------------------------------------------------
    def call_fwd(self, B=None):
        rc = self.lib.dctr_mlp_fwd(ctypes.byref(self.desc), self.ptr("x"), self.ld_x, self.B if B is None else B,
                                   self.ptr("logit") if self.proj else None, self.stream)
        self.sync()
        return rc

    def call_bwd(self, B=None):
        rc = self.lib.dctr_mlp_bwd(ctypes.byref(self.desc), self.ptr("x"), self.ld_x, self.B if B is None else B,
                                   self.ptr("g"), 0 if self.proj else self.ld_g, self.ptr("gx") if self.has_gx else None,
                                   self.ld_gx if self.has_gx else 0, self.ptr("ws"), self.stream)
        self.sync()
        return rc

    def call_train(self, defer, B=None):
        rc = self.lib.dctr_mlp_train_step(
            ctypes.byref(self.desc), self.ptr("x"), self.ld_x, self.B if B is None else B,
            self.ptr("part0") if self.parts[0] else None, self.ptr("part1") if self.parts[1] else None,
            self.ptr("hbias") if self.head_bias else None, self.ptr("y"), self.ptr("y_pred"), self.ptr("loss"),
            self.ptr("g_logit"), self.ptr("g_bias") if self.has_g_bias else None, self.ptr("gx") if self.has_gx else None,
            self.ld_gx if self.has_gx else 0, self.ptr("ws"), int(defer), self.step_ref(), self.stream)
        self.sync()
        return rc

    def call_wgrad(self, B=None):
        rc = self.lib.dctr_mlp_train_wgrad(ctypes.byref(self.desc), self.ptr("x"), self.ld_x, self.B if B is None else B,
                                           self.ptr("g_logit"), self.ptr("ws"), self.ptr("loss"),
                                           self.ptr("g_bias") if self.has_g_bias else None, self.step_ref(), self.stream)
        self.sync()
        return rc

    # ---- what a call may write, what it must produce -----------------------------------------------------------------------
    def _fwd_names(self):
        return [("h", l) for l in range(len(self.hidden))]

    def _data_names(self):
        return [("dh", l) for l in range(len(self.hidden))] + (["gx"] if self.has_gx else [])

    def _wgrad_names(self):
        out = [("gW", l) for l in range(len(self.hidden)) if l not in self.no_gW]
        out += [("gbias", l) for l in range(len(self.hidden)) if l not in self.no_bias]
        return out + (["g_w_out"] if self.proj else [])

    def _may(self, names, stepped):
        may = np.zeros(self.fa.numel(), bool)
        for n in names:
            may[self.ix[n].ravel()] = True
            if isinstance(n, tuple) and n[0] in ("h", "dh"):
                nn = self.hidden[n[1]]
                may[self.pad[n][:, :r4(nn) - nn].ravel()] = True
            elif isinstance(n, tuple) and n[0] == "gW":
                may[self.pad[n].ravel()] = True
            elif n == "gx":
                may[self.pad[n][:, :_ru(self.K, 64) - self.K].ravel()] = True
        for k in stepped:
            may[self.ix[k].ravel()] = True
            if self.opt == "adagrad":
                may[self.ix[_state_key(k)].ravel()] = True
        return may

    def _expect(self, m, g=None):
        """the model's outputs at its current parameters (train: head included)"""
        pres, hs, logit = m.forward(self.x)
        out = dict((("h", l), h) for l, h in enumerate(hs))
        if self.mode == "train":
            hd = m.head(logit, self.p0_now, self.p1_now, self.head_bias, self.y_now)
            out.update((k, np.atleast_1d(hd[k])) for k in ("y_pred", "loss", "g_logit", "g_bias"))
            g = hd["g_logit"]
        elif logit is not None:
            out["logit"] = logit
        if g is not None:
            out.update(m.backward(self.x, hs, g))
        return out

    def _bar(self, name):
        kind = name[0] if isinstance(name, tuple) else name
        return {"y_pred": (TOL_YPRED, False), "g_logit": (TOL_GLOGIT, False), "loss": (TOL_LOSS, True)}.get(kind, (TOL, True))

    def _verify(self, tag, before, names, may_names, stepped=(), exp=None, exp32=None):
        after = self.snapshot()
        may = self._may(may_names, stepped)
        changed = np.flatnonzero((_bits(after) != _bits(before)) & ~may)
        assert not changed.size, "%s: %d floats outside what the call writes changed (first at arena offset %d: %r -> %r): " \
            "a guard band, an input, a pad column, a NULL tensor's slot or the float behind the workspace" % (
                tag, changed.size, changed[0], before[changed[0]], after[changed[0]])
        # (b) the pad columns the header speaks of
        for n in names:
            kind = n[0] if isinstance(n, tuple) else n
            if kind == "gW":
                assert np.all(after[self.pad[n]] == 0), "%s: %s pad columns [K, ld_w) are not all 0" % (tag, n)
            elif kind in ("h", "dh"):
                nn = self.hidden[n[1]]
                v = after[self.pad[n][:, :r4(nn) - nn]]
                assert np.all((v == 0) | (_bits(v) == SENT_BITS)), "%s: %s columns [N, r4(N)) hold neither 0 nor what they held" % (
                    tag, n)
            elif kind == "gx":
                lo = min(_ru(self.K, 32), self.ld_gx) - self.K
                hi = min(_ru(self.K, 64), self.ld_gx) - self.K
                assert np.all(after[self.pad[n][:, :lo]] == 0), "%s: gx columns [K, round_up(K, 32)) are not all 0" % tag
                v = after[self.pad[n][:, lo:hi]]
                assert np.all((v == 0) | (_bits(v) == SENT_BITS)), "%s: gx columns from round_up(K, 32) hold neither 0 nor " \
                    "what they held" % tag
        # (c) (e) values
        line = []
        for n in names:
            x, r, r32 = after[self.ix[n]].astype(np.float64), np.asarray(exp[n], np.float64), np.asarray(exp32[n], np.float64)
            r, r32 = r.reshape(x.shape), r32.reshape(x.shape)
            if not x.size:
                continue
            kind = n[0] if isinstance(n, tuple) else n
            assert np.all(np.isfinite(x)), "%s %s: %d values are not finite" % (tag, n, (~np.isfinite(x)).sum())
            bound, rel = self._bar(n)
            scale = max(1.0, float(np.abs(r).max())) if rel else 1.0
            err, err32 = float(np.abs(x - r).max()), float(np.abs(r32 - r).max())
            self._worst(kind, err / scale, err32 / scale)
            line.append("%s %.1e|%.1e" % (kind if not isinstance(n, tuple) else "%s%d" % n, err / scale, err32 / scale))
            assert err32 <= 0.25 * bound * scale, "%s %s: plain float32 is %.3e from float64, more than a quarter of the bar " \
                "%.3e: the case is not comparable" % (tag, n, err32, bound * scale)
            assert err <= bound * scale, "%s %s: max|d| %.3e (scale %.3g), bound %.3e (plain float32: %.3e)" % (
                tag, n, err, scale, bound * scale, err32)
            zero = r == 0
            if kind == "h":
                zero = zero & ~self.risky[:, None]
            if kind not in ("y_pred", "loss", "g_bias"):
                bad = zero & (x != 0)
                assert not bad.any(), "%s %s: %d values are not 0 where the float64 reference is exactly 0 (first %r)" % (
                    tag, n, bad.sum(), x[bad][0])
        if "g_logit" in names:
            assert np.all(after[self.ix["g_logit"]][self.risky] == 0), "%s: g_logit of a saturated row is not exactly 0" % tag
        # (d) parameters and state behind the in-kernel step
        for k in stepped:
            for n, is_state in ((k, False), (_state_key(k), True)) if self.opt == "adagrad" else ((k, False),):
                x = after[self.ix[n]].astype(np.float64)
                r, r32 = [(m.state[k] if is_state else m.param(k)).astype(np.float64).reshape(x.shape)
                          for m in (self.ref, self.ref32)]
                assert np.all(np.isfinite(x)), "%s %s: not finite" % (tag, n)
                scale = float(np.abs(r).max())
                err, err32 = float(np.abs(x - r).max()), float(np.abs(r32 - r).max())
                bound = max(4.0 * err32 / scale, 4.0 * ULP)
                kind = ("state " if is_state else "param ") + (k[0] if isinstance(k, tuple) else k)
                self._worst(kind, err / scale, err32 / scale)
                line.append("%s %.1e|%.1e" % (kind, err / scale, err32 / scale))
                assert err <= bound * scale, "%s %s: max|d| %.3e (scale %.3g) ratio %.3e, bound %.3e (plain float32: %.3e)" % (
                    tag, kind, err, scale, err / scale, bound, err32 / scale)
        print("%s: %s" % (tag, "  ".join(line)))
        return after

    @staticmethod
    def _worst(kind, ratio, ratio32):
        w = WORST.setdefault(kind, [0.0, 0.0])
        w[0], w[1] = max(w[0], ratio), max(w[1], ratio32)

    # ---- the routes ----------------------------------------------------------------------------------------------------
    def run_fwd_bwd(self):
        """dctr_mlp_fwd, dctr_mlp_bwd, and dctr_mlp_bwd again: the same bits"""
        tag = "B=%d K=%d %s %s" % (self.B, self.K, tuple(self.hidden), "w_out" if self.proj else "no-w_out")
        self.prepare_bwd()
        before = self.snapshot()
        assert self.call_fwd() == 0, tag + ": dctr_mlp_fwd failed"
        exp, exp32 = self._expect(self.ref, self.g_now), self._expect(self.ref32, self.g_now)
        names = self._fwd_names() + (["logit"] if self.proj else [])
        before = self._verify(tag + " fwd", before, names, names, exp=exp, exp32=exp32)
        assert self.call_bwd() == 0, tag + ": dctr_mlp_bwd failed"
        names = self._data_names() + self._wgrad_names()
        first = self._verify(tag + " bwd", before, names, names + ["ws"], exp=exp, exp32=exp32)
        assert self.call_bwd() == 0
        again = self.snapshot()
        assert np.array_equal(_bits(first), _bits(again)), tag + ": a second dctr_mlp_bwd leaves other bits"
        return again

    def train_once(self, defer, tag=""):
        """one train step by either route, verified; the models take the optimizer step after it"""
        tag = "B=%d K=%d %s %s %s%s" % (self.B, self.K, tuple(self.hidden), self.opt or "no-step",
                                       "deferred" if defer else "direct", tag)
        self.prepare_train()
        before = self.snapshot()
        exp, exp32 = self._expect(self.ref), self._expect(self.ref32)
        first = self._fwd_names() + ["y_pred", "g_logit"] + self._data_names()
        second = self._wgrad_names() + ["loss"] + (["g_bias"] if self.has_g_bias else [])
        stepped = self.params() if self.opt else []
        assert self.call_train(defer) == 0, tag + ": dctr_mlp_train_step failed"
        if defer:
            # y_pred, g_logit, gx, h, dh are complete; loss / gW / ... may or may not have been touched, the parameters not
            before = self._verify(tag + " (1st call)", before, first, first + second + ["ws"], exp=exp, exp32=exp32)
            assert self.call_wgrad() == 0, tag + ": dctr_mlp_train_wgrad failed"
            first_may = []
        else:
            first_may = first
        if self.opt:
            for m, e in ((self.ref, exp), (self.ref32, exp32)):
                for k in stepped:
                    m.step(k, e[_grad_key(k)])
        return self._verify(tag, before, (first if not defer else []) + second, first_may + second + ["ws"], stepped,
                            exp=exp, exp32=exp32)


def same_bits(a, b, what):
    diff = np.flatnonzero(_bits(a) != _bits(b))
    assert not diff.size, "%s: %d of %d arena floats differ (first at offset %d: %r | %r)" % (
        what, diff.size, a.size, diff[0], a[diff[0]], b[diff[0]])


# ---- the routes of one geometry ------------------------------------------------------------------------------------------
def fwd_bwd(lib, dev, **kw):
    """dctr_mlp_fwd + dctr_mlp_bwd with w_out and without"""
    TowerCase(lib, dev, "bwd", proj=True, **kw).run_fwd_bwd()
    kw = dict((k, v) for k, v in kw.items() if k not in ("parts", "head_bias", "g_bias"))
    TowerCase(lib, dev, "bwd", proj=False, **kw).run_fwd_bwd()


def train(lib, dev, opt=None, steps=None, **kw):
    """dctr_mlp_train_step(defer_wgrad = 0) against (defer_wgrad = 1) + dctr_mlp_train_wgrad: each verified against the
    models, and the same bits in the whole arena.  step = NULL: one step and the same call again (identical bits);
    SGD / Adagrad: three successive steps."""
    steps = (3 if opt else 1) if steps is None else steps
    arenas = []
    for defer in (0, 1):
        c = TowerCase(lib, dev, "train", opt=opt, **kw)
        for i in range(steps):
            last = c.train_once(defer, " step %d" % (i + 1) if opt else "")
        if not opt:
            assert c.call_train(defer) == 0 and (not defer or c.call_wgrad() == 0)
            same_bits(last, c.snapshot(), "a second identical call (%s)" % ("deferred" if defer else "direct"))
        arenas.append(last)
    same_bits(arenas[0], arenas[1], "defer_wgrad = 0 against defer_wgrad = 1 + dctr_mlp_train_wgrad (%s)" % (opt or "no step"))
    return c


def empty_batch(lib, dev):
    """B = 0: DCTR_OK from every entry point, nothing written"""
    for mode in ("bwd", "train"):
        c = TowerCase(lib, dev, mode, B=3, K=13, hidden=(8,), opt="adagrad" if mode == "train" else None)
        before = c.snapshot()
        calls = (c.call_fwd, c.call_bwd) if mode == "bwd" else (lambda B: c.call_train(0, B), lambda B: c.call_train(1, B),
                                                               c.call_wgrad)
        for fn in calls:
            assert fn(B=0) == 0, "B = 0 is not DCTR_OK"
            same_bits(before, c.snapshot(), "a call with B = 0 wrote something")


def split_batch(lib, dev, opt):
    """B = 200 at 39 -> (256, 128): the weight gradients split the batch"""
    kw = dict(B=200, K=39, hidden=(256, 128), seed=21)
    p = wgrad_plan(39, (256, 128), 200, True, [r4(39) + 4, r4(256) + 4])
    assert p["S"] == 3 and p["bs"] == 72 and 200 - 2 * 72 == 56, "the case no longer splits the batch into 72 + 72 + 56 rows"
    c = train(lib, dev, opt=opt, **kw)
    if c.real:          # S from the advertised size, as tests/test_gpu_wgrad_assignment.py reads it
        S, rest = divmod(c.n_ws - 2 * ((200 + 15) // 16), p["slab"])
        assert rest == 0 and S == 3, "advertised workspace: %d floats are not 3 slabs of %d + the head's partials" % (
            c.n_ws, p["slab"])


# geometry id -> (arguments, the arm of mlp_train_body it was chosen for: fast, kc (None: not of interest), bwd_off > 0)
GEOMETRY = [
    ("fast1-keep-B64-K429-256x128", dict(B=64, K=429, hidden=(256, 128), seed=1), (1, 512, True)),
    ("fast2-keep-B37-K13-8", dict(B=37, K=13, hidden=(8,), seed=2), (2, 512, True)),
    ("fast2-keep-B1-K13-8", dict(B=1, K=13, hidden=(8,), seed=3), (2, 512, True)),
    ("fast1-alias-B37-K500-512x64", dict(B=37, K=500, hidden=(512, 64), seed=4), (1, 512, False)),
    ("fast0-keep-B50-K754-64x32x16", dict(B=50, K=754, hidden=(64, 32, 16), seed=5), (0, 512, True)),
    ("fast0-alias-kc256-B70-K429-1024x512x256", dict(B=70, K=429, hidden=(1024, 512, 256), seed=6), (0, 256, False)),
    ("fast0-alias-kc64-B40-K1100-1152x64", dict(B=40, K=1100, hidden=(1152, 64), seed=7), (0, 64, False)),
    ("rows-B15", dict(B=15, K=13, hidden=(8,), seed=8), (2, 512, True)),
    ("rows-B16", dict(B=16, K=13, hidden=(8,), seed=9), (2, 512, True)),
    ("rows-B17", dict(B=17, K=13, hidden=(8,), seed=10), (2, 512, True)),
    ("rows-B33", dict(B=33, K=13, hidden=(8,), seed=11), (2, 512, True)),
    ("layers12-B20", dict(B=20, K=11, hidden=(8, 24, 9, 23, 10, 22, 11, 21, 12, 20, 13, 19), seed=12), (2, 512, True)),
    ("identity-B33-K18-10x7", dict(B=33, K=18, hidden=(10, 7), relu=0, seed=13), (2, 512, True)),
    ("bias-null-layer1", dict(B=21, K=18, hidden=(10, 12, 7), no_bias=(1,), seed=14), (2, 512, True)),
    ("gW-null-layer0", dict(B=21, K=18, hidden=(10, 12, 7), no_gW=(0,), seed=15), (2, 512, True)),
    ("gx-null", dict(B=21, K=18, hidden=(10, 7), gx=False, seed=16), (2, 512, True)),
    # gx's pad columns past a column group: K = 32 leaves [32, 36) to no group, K = 64 leaves [64, 68) past round_up(K, 64)
    ("gx-pad-K32", dict(B=21, K=32, hidden=(10,), seed=17), (2, 512, True)),
    ("gx-pad-K64", dict(B=21, K=64, hidden=(10,), seed=18), (2, 512, True)),
    # NaN in x's row padding, through the fast bodies' staging, the general body's chunked staging and the weight gradients
    ("x-pad-nan-fast", dict(B=37, K=13, hidden=(8,), seed=19, x_pad=np.nan), (2, 512, True)),
    ("x-pad-nan-general", dict(B=50, K=754, hidden=(64, 32, 16), seed=20, x_pad=np.nan), (0, 512, True)),
]
# the head's operands, on the narrow tower: (part0, part1), head bias, g_bias
HEAD = [("head-part0-only", dict(parts=(True, False))), ("head-part1-only", dict(parts=(False, True))),
        ("head-no-parts", dict(parts=(False, False))), ("head-bias-null", dict(head_bias=False)),
        ("head-g_bias-null", dict(g_bias=False)), ("head-bare", dict(parts=(False, False), head_bias=False, g_bias=False))]


def _armed(fn, kw, arm):
    def run(lib, dev):
        a = launch_arm(kw["K"], kw["hidden"])
        got = (a["fast"], a["kc"], a["bwd_off"] > 0)
        assert got == arm, "the case no longer reaches the arm it was chosen for: (fast, kc, bwd_off > 0) = %s, not %s" % (
            got, arm)
        fn(lib, dev, **kw)
    return run


def case_list():
    """[(id, fn(lib, dev))]: every case of tests/test_gpu_tower_abi.py; tests/test_tower_abi_host.py runs the same list"""
    out = []
    for name, kw, arm in GEOMETRY:
        light = name.startswith(("gx-", "rows-", "x-pad-"))
        if not light:
            out.append((name + "-fwd-bwd", _armed(fwd_bwd, kw, arm)))
        out.append((name + "-train", _armed(train, kw, arm)))
        if not light:
            out.append((name + "-sgd", _armed(lambda lib, dev, **k: train(lib, dev, opt="sgd", **k), kw, arm)))
        out.append((name + "-adagrad", _armed(lambda lib, dev, **k: train(lib, dev, opt="adagrad", **k), kw, arm)))
    for name, extra in HEAD:
        kw = dict(B=37, K=13, hidden=(8,), seed=30 + len(out), **extra)
        out.append((name + "-train", _armed(train, kw, (2, 512, True))))
        out.append((name + "-adagrad", _armed(lambda lib, dev, **k: train(lib, dev, opt="adagrad", **k), kw, (2, 512, True))))
    # Adagrad's eps at 1e-10 is invisible (sqrt(s) + eps against sqrt(s + eps) differ by 1e-9 of the step): one case at 0.1
    out.append(("adagrad-eps0.1", lambda lib, dev: train(lib, dev, opt="adagrad", eps=0.1, B=37, K=13, hidden=(8,), seed=2)))
    for opt in (None, "sgd", "adagrad"):
        out.append(("split-batch-B200-%s" % (opt or "train"), lambda lib, dev, o=opt: split_batch(lib, dev, o)))
    out.append(("empty-batch", empty_batch))
    return out
