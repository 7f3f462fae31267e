"""Three properties of the C ABI that need no oracle ("Isolation"): a call's results depend neither on the bytes its workspace
and output buffers held before (check_fill_independence), nor on which calls the same buffers served earlier (check_history_independence),
nor on what lies beside the buffers it was given -- and it writes nothing there (check_redzones).

Each check drives one FORM LIST through harness.Runner: every entry-point form an engine issues on one workspace.  A form is self-contained
(it runs its own forward), so it means the same at any place of a history.  What a form returns, and what is compared: hvo, all 8 stats,
d_hvo, the WHOLE flat gradient buffer (the tensors, the alignment gaps, the guard element), parameters, moments and gt_step_state after
each update, and the saved tensors check_step reads (x0, P, hact, memory).  Whole workspaces are never compared: unwritten regions differ
by design.

Under gt_set_deterministic(1) everything is compared with np.array_equal (a NaN anywhere fails) -- but the 8 stats of the stand-alone gt_loss
and the buffer gt_backward(accumulate = 1) added to, float atomics in either mode (ATOMIC_ALWAYS), which take the bar below.  deterministic=False: the forward side
stays bitwise; gradients, parameters and moments must be finite and within check_accumulate's bar for two summation orders of the same sum
(parity.ACC_TOL of the tensor's largest entry plus one ulp; behind Adam plus what that difference itself propagates to, adam_bars) -- and every form then starts from the initial parameters, so the forward side
of a later form does not inherit that freedom."""
import ctypes

import numpy as np

import parity
from harness import Runner
from oracle import numpy_groove as ng
from transformergrooveinfilling_amd import _lib

BASE, QNAN = 0x40E80000, 0x7FC00000                 # 7.25f: harness.Runner's own workspace fill; a quiet NaN
FILLS = {"7.25": BASE, "qnan": QNAN, "all-ones": 0xFFFFFFFF, "+inf": 0x7F800000, "one": 0x00000001}     # (1: a plausible serial / ticket value)
RNG, LR, PENALTY, PD_SEED = (1234, 99, 7), 0.05, 0.4, 0x5EED
PACKS_CURRENT = 4                                    # GT_STEP_PACKS_CURRENT
LOSS_OPTS = dict(penalty_h=0.4, penalty_vo=0.7, pos_weight=[1.5, 1.0, 2.0, 1.0, 0.5, 1.0, 3.0, 1.0, 1.25],
                 voice_weight=[1.0, 0.5, 1.0, 2.0, 1.0, 1.0, 0.25, 1.0, 1.5], focal_gamma=1.5, term_weight=(1.0, 0.5, 2.0))
SAVED = (("x0", 0), ("P", 0), ("hact", 0), ("memory", 0))
GRAD_SIDE = ("grads", "grads_before_update", "bucket0", "params", "m", "v")
# the stand-alone gt_loss adds its workgroups' partial sums into stats with float atomics (csrc/gt_misc.h loss_kernel<TICKET = false>; the
# fused steps' loss and gt_loss_ex take a ticket and add in a fixed order): the same sum in another order on every run, in either mode
# gt_backward(accumulate = 1): on the rider schedules the tail launch cuts the token range of layer 0's in-proj and of the input layer in two
# and the partial tiles meet in fp32 atomics (csrc/gt_seq_wg.h seq_tail_kernel) -- order-independent on a zeroed buffer, (G0 + a) + b against
# (G0 + b) + a on the non-zero one this form adds to; gt_set_deterministic does not change that split
ATOMIC_ALWAYS = ("loss_stats", "accumulate.grads")
STEP_FORMS = ("sgd", "adam", "skip1_update", "skip2_skip3", "step_loss")     # the forms whose first call is gt_train_step[_loss]
LEAVES_PACKS = ("sgd", "adam", "skip1_update", "step_loss")                   # ... and whose last launch is an update that writes the next step's packs


def forms_of(cfg):
    f = ["eval", "step", "accumulate", "sgd", "adam", "skip1_update", "skip2_skip3", "step_loss"]
    return f + (["predict", "predict_pd"] if cfg.get("num_decoder_layers", 0) else [])


class Session:
    """One Runner with the form list's inputs.  after_call(name): run after every library call.  prefill: a bit pattern hvo, stats, d_hvo and
    tgt hold before the first call.  x_short: x is handed over this many rows short (a negative control: the library then reads the rest
    from whatever follows).  adopt_ws: another Runner's workspace buffer to run on, after gt_workspace_init for THIS configuration."""

    def __init__(self, backend, cfg, B, p, seq=True, flags=0, ws_fill=BASE, guard=None, prefill=None, after_call=None, x_short=0, adopt_ws=None):
        self.cfg = cfg = dict(cfg, dropout=p)
        self.train = int(p > 0)
        self.after_call = after_call
        self.r = r = Runner(cfg, B, backend, rng=RNG, lr=LR, seq=seq, flags=flags, ws_fill=ws_fill, guard=guard)
        if adopt_ws is not None:
            assert (adopt_ws.t.numel() if hasattr(adopt_ws, "t") else adopt_ws.a.size) >= r.lib.workspace_floats(r.c)
            r.ws = adopt_ws
            r.lib.call("gt_workspace_init", ctypes.byref(r.c), r.ws.ptr, ctypes.c_void_p(0))
        r.set_params(ng.init_params(cfg, seed=3, perturb=0.05))
        x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=5)
        self.encdec = bool(cfg.get("num_decoder_layers", 0))
        r.x = r.Buf(np.asarray(x, np.float32).reshape(r.M, -1)[:r.M - x_short])
        r.y = r.Buf(np.asarray(y, np.float32).reshape(r.M, 27))
        r.tgt_in = r.Buf(np.asarray(parity.shift_right(y), np.float32).reshape(r.M, 27)) if self.encdec else None
        r.m, r.v = r.Buf(np.zeros(r.total, np.float32)), r.Buf(np.zeros(r.total, np.float32))
        if prefill is not None:
            poison = lambda *shape: r.Buf(np.full(shape, prefill, np.uint32).view(np.float32))
            r.hvo, r.d_hvo, r.tgt, r.stats = poison(r.M, 27), poison(r.M, 27), poison(r.M, 27), poison(8)
        self.lo = _lib.make_loss_opts(**LOSS_OPTS)
        self.voice = r.Buf(np.zeros(36, np.float32))
        self.scratch = r.Buf(np.zeros(int(r.lib.cdll.gt_loss_scratch_floats(ctypes.byref(r.c))), np.float32))
        rnd = np.random.default_rng(43)
        self.G0 = np.zeros(r.total, np.float32)             # check_accumulate's: multiples of 2^-10 inside the tensors, zero outside
        for off, size, _, _ in r.entries:
            self.G0[off:off + size] = (rnd.integers(-1024, 1025, size) / 1024.0).astype(np.float32)
        self.bucket0 = r.lib.grad_buckets(r.c)[0]
        self.packs = False                                   # did the last call leave the next step's weight packs in the workspace?
        self.initial = self.opt_state()

    # ---- state a fresh Runner takes over ---------------------------------------------------------------------------------------------
    def opt_state(self):
        r = self.r
        return {k: getattr(r, k).numpy().copy() for k in ("params", "m", "v", "state")}

    def set_opt_state(self, st):
        for k, a in st.items():
            setattr(self.r, k, self.r.Buf(a.copy()))
        self.packs = False

    # ---- calls ---------------------------------------------------------------------------------------------------------------------
    def call(self, name, *args):
        self.r.lib.call(name, *args)
        if self.after_call is not None:
            self.after_call(name)

    def ws_words(self, name, layer):
        """the raw 32-bit words of a saved tensor (its bf16 copy where that is the only one), without copying the whole workspace back"""
        r = self.r
        off, cnt = r.lib.ws_find(r.c, name, layer)
        if r.bf16_only(name, layer):
            off, cnt = r.lib.ws_find(r.c, name + "16", layer)[0], (cnt + 1) // 2
        if hasattr(r.ws, "t"):
            import torch
            torch.cuda.synchronize()
            return r.ws.t[off:off + cnt].cpu().numpy().view(np.uint32)
        return r.ws.numpy()[off:off + cnt].view(np.uint32).copy()

    def saved(self):
        return {"ws." + n: self.ws_words(n, l) for n, l in SAVED}

    def get(self, *names):
        return {n: getattr(self.r, n).numpy().copy() for n in names}

    def zero_grads(self):
        self.r.grads = self.r.Buf(np.zeros(self.r.total, np.float32))

    def forward(self, train):
        r = self.r
        self.call("gt_forward", ctypes.byref(r.c), r.params.ptr, r.pe.ptr, r.x.ptr, r.tgt_in.ptr if self.encdec else None, r.hvo.ptr, r.ws.ptr,
                  r.state.ptr, int(train), r.stream)

    def loss(self):
        r = self.r
        self.call("gt_loss", ctypes.byref(r.c), r.hvo.ptr, r.y.ptr, ctypes.c_float(PENALTY), r.stats.ptr, r.d_hvo.ptr, r.stream)

    def backward(self, accumulate):
        r = self.r
        self.call("gt_backward", ctypes.byref(r.c), r.params.ptr, r.grads.ptr, r.x.ptr, r.tgt_in.ptr if self.encdec else None, r.hvo.ptr,
                  r.d_hvo.ptr, r.ws.ptr, r.state.ptr, self.train, int(accumulate), r.stream)

    def train_step(self, algo, skip, stats=True):
        r = self.r
        args = (ctypes.byref(r.c), algo, r.params.ptr, r.grads.ptr, r.m.ptr if algo else None, r.v.ptr if algo else None, r.pe.ptr, r.x.ptr,
                r.y.ptr, ctypes.c_float(PENALTY), r.hvo.ptr, r.stats.ptr if stats else None, r.tgt.ptr, r.ws.ptr, r.state.ptr, int(skip), r.stream)
        if stats:
            return self.call("gt_train_step", *args)
        rc = r.lib.cdll.gt_train_step(*args)
        assert rc != 0 and b"stats" in r.lib.cdll.gt_last_error(), rc
        if self.after_call is not None:
            self.after_call("gt_train_step (failing)")

    def step_outputs(self):
        out = self.get("stats", "hvo")
        if self.encdec:
            out.update(self.get("tgt"))              # the shifted target the step wrote for its decoder
        return out

    # ---- the forms: bit = PACKS_CURRENT or 0, or-ed into skip_update where the form starts with a train step ------------------------------
    def form_eval(self, bit):
        self.forward(0)
        return dict(self.get("hvo"), **self.saved())

    def form_step(self, bit):
        self.forward(self.train)
        out = dict(self.get("hvo"), **self.saved())
        self.loss()
        out.update(self.get("d_hvo"), loss_stats=self.r.stats.numpy().copy())
        self.backward(0)
        return dict(out, **self.get("grads"))

    def form_accumulate(self, bit):
        self.forward(self.train)
        self.loss()
        self.r.grads = self.r.Buf(self.G0.copy())
        self.backward(1)
        return dict(self.get("hvo", "d_hvo", "grads"), loss_stats=self.r.stats.numpy().copy())

    def form_sgd(self, bit):
        self.zero_grads()
        self.train_step(0, 0 | bit)
        return dict(self.step_outputs(), **self.get("grads", "params", "state"), **self.saved())

    def form_adam(self, bit):
        self.zero_grads()
        self.train_step(1, 0 | bit)
        return dict(self.step_outputs(), **self.get("grads", "params", "m", "v", "state"))

    def form_skip1_update(self, bit):
        r = self.r
        self.zero_grads()
        self.train_step(0, 1 | bit)
        out = dict(self.step_outputs(), grads_before_update=r.grads.numpy().copy())
        self.call("gt_optimizer_step_ws", ctypes.byref(r.c), 0, r.params.ptr, r.grads.ptr, None, None, r.ws.ptr, r.state.ptr, 1, r.stream)
        return dict(out, **self.get("grads", "params", "state"))

    def form_skip2_skip3(self, bit):
        self.zero_grads()
        self.train_step(0, 2 | bit)
        o0, c0 = self.bucket0
        out = dict(self.step_outputs(), bucket0=self.r.grads.numpy()[o0:o0 + c0].copy())          # final after the first half; the rest is not yet
        self.train_step(0, 3)
        return dict(out, **self.get("grads", "state"))

    def form_step_loss(self, bit):
        r = self.r
        self.zero_grads()
        self.call("gt_train_step_loss", ctypes.byref(r.c), 0, r.params.ptr, r.grads.ptr, None, None, r.pe.ptr, r.x.ptr, r.y.ptr,
                  ctypes.byref(self.lo), self.voice.ptr, self.scratch.ptr, r.hvo.ptr, r.stats.ptr, r.tgt.ptr, r.ws.ptr, r.state.ptr, 0 | bit, r.stream)
        return dict(self.step_outputs(), voice_stats=self.voice.numpy().copy(), loss_scratch=self.scratch.numpy().copy(),
                    **self.get("grads", "params", "state"))

    def form_predict(self, bit):
        r = self.r
        self.call("gt_predict", ctypes.byref(r.c), r.params.ptr, r.pe.ptr, r.x.ptr, r.hvo.ptr, ctypes.c_float(0.5), 1, r.tgt.ptr, r.ws.ptr, r.stream)
        return self.get("hvo")

    def form_predict_pd(self, bit):
        r = self.r
        self.call("gt_predict_pd", ctypes.byref(r.c), r.params.ptr, r.pe.ptr, r.x.ptr, r.hvo.ptr, ctypes.c_uint32(PD_SEED), r.tgt.ptr, r.ws.ptr, r.stream)
        return self.get("hvo")

    def form_bare_backward(self, bit):
        """NEGATIVE CONTROL, never part of a form list: gt_backward on a workspace no forward has written"""
        self.backward(0)
        return self.get("grads")

    def run(self, name, packs_bit=False):
        """one form; packs_bit: pass GT_STEP_PACKS_CURRENT where the form starts with a train step and the previous call left the packs"""
        bit = PACKS_CURRENT if packs_bit and self.packs and name in STEP_FORMS else 0
        out = getattr(self, "form_" + name)(bit)
        self.packs = name in LEAVES_PACKS
        return out

    def run_all(self, forms, reset):
        out = {}
        for name in forms:
            if reset:
                self.set_opt_state(self.initial)
            out.update({name + "." + k: v for k, v in self.run(name).items()})
        return out


def compare(got, want, tag, exact=True):
    """every result of `got` against the same result of `want`: np.array_equal -- or, with exact False and for gradients, parameters and
    moments only, finite and within parity.ACC_TOL x max |want| + one ulp.  AssertionError naming the result and its first differing element."""
    assert list(got) == list(want), (tag, sorted(set(got) ^ set(want)))
    extra = adam_bars(got, want) if not exact and "adam.state" in want else {}
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, k, a.shape, b.shape)
        if np.array_equal(a, b):
            continue
        a, b = a.reshape(-1), b.reshape(-1)
        if b.dtype.kind == "f" and not (np.isfinite(a).all() and np.isfinite(b).all()):
            i = int(np.flatnonzero(~(np.isfinite(a) & np.isfinite(b)))[0])
            raise AssertionError("%s: %s is not finite: element %d of %d: %r against %r" % (tag, k, i, a.size, a[i], b[i]))
        if k.split(".")[-1] in ATOMIC_ALWAYS or k in ATOMIC_ALWAYS or (not exact and k.split(".")[-1] in GRAD_SIDE):
            a64, b64 = a.astype(np.float64), b.astype(np.float64)
            bar = parity.ACC_TOL * np.abs(b64).max() + np.spacing(np.abs(b)) + extra.get(k, 0.0)
            if (np.abs(a64 - b64) <= bar).all():
                continue
        i = int(np.flatnonzero(a != b)[0])
        raise AssertionError("%s: %s differs in %d of %d elements, first at %d: %r against %r"
                             % (tag, k, int((a != b).sum()), a.size, i, a[i], b[i]))


def adam_bars(got, want, form="adam"):
    """What two summation orders of the same gradient may differ by AFTER Adam, from the two runs' own outputs.  m' is linear in the gradient
    and keeps the accumulation bar; v' and the parameters are not -- an element whose gradient is rounding noise around zero moves by up to
    lr whichever sign the noise has.  Both runs started from the same parameters and moments, so with t, lr, the betas and eps read from the
    state the step left, in fp64:
      params: |p_a - p_b| = |u(m'_a, v'_a) - u(m'_b, v'_b)|,  u = lr (m' / (1 - beta1^t)) / (sqrt(v' / (1 - beta2^t)) + eps)
      v':     |v'_a - v'_b| = (1 - beta2) |g_a - g_b| |g_a + g_b| <= (1 - beta2) (|m'_a - m'_b| / (1 - beta1)) (|g_a| + |g_b|), |g| <= sqrt(v' / (1 - beta2))
    -> {result name: the array to ADD to the accumulation bar}."""
    st = np.asarray(want[form + ".state"]).view(np.uint8)
    t = int(st[12:16].view(np.uint32)[0])
    lr, _, b1, b2, eps = (float(f) for f in st[16:36].view(np.float32))
    f64 = lambda r, k: np.asarray(r[form + "." + k], np.float64).reshape(-1)
    u = lambda r: lr * (f64(r, "m") / (1 - b1 ** t)) / (np.sqrt(f64(r, "v") / (1 - b2 ** t)) + eps)
    dg = np.abs(f64(got, "m") - f64(want, "m")) / (1 - b1)
    return {form + ".params": np.abs(u(got) - u(want)),
            form + ".v": (1 - b2) * dg * (np.sqrt(f64(got, "v") / (1 - b2)) + np.sqrt(f64(want, "v") / (1 - b2)))}


def assert_written(res, tag):
    """every float the API defines is a number: no element of a pre-filled NaN is left, and the three spare stats are zero"""
    for k, a in res.items():
        if np.asarray(a).dtype.kind == "f":
            assert np.isfinite(a).all(), "%s: %s holds %d non-finite elements" % (tag, k, int((~np.isfinite(a)).sum()))
        if k.split(".")[-1] in ("stats", "loss_stats"):
            assert a[2] == 0 and a[6] == 0 and a[7] == 0, (tag, k, a)


def _lib_of(backend):
    import harness
    return harness.emu_lib() if backend == "emu" else _lib.get_lib()


def other_config(backend, cfg, B):
    """(cfg, batch) of ANOTHER model -- another d_model, another batch -- whose workspace is at least as large as that of (cfg, B)"""
    lib = _lib_of(backend)
    floats = lambda c, b: lib.workspace_floats(_lib.make_config(b, c["embedding_size_src"], c["d_model"], c["n_heads"], c["dim_feedforward"],
                                                                c["num_encoder_layers"], c.get("num_decoder_layers", 0), c.get("dropout", 0.0),
                                                                c.get("precision", 0)))
    mk = lambda d, h: dict(d_model=d, n_heads=h, dim_feedforward=2 * d if d < 256 else 512, num_encoder_layers=1, num_decoder_layers=0,
                           embedding_size_src=16, dropout=0.1)
    need = floats(cfg, B)
    for other in (mk(64, 4), mk(32, 4), mk(256, 2), mk(512, 8)):          # the first other width that gets there within 600 sequences
        if other["d_model"] == cfg["d_model"]:
            continue
        b = max(1, need // max(1, floats(other, 2) - floats(other, 1)))
        while b == B or floats(other, b) < need:
            b += 1
        if b <= 600:
            break
    return other, b


def check_fill_independence(backend, cfg, B, p, seq=True, flags=0, fills=tuple(FILLS), deterministic=True, forms=None, prefill=True, other=True):
    """The form list once per workspace fill: every result equals the baseline's (fill 7.25).  prefill: once more with the workspace AND hvo,
    stats, d_hvo and tgt holding quiet NaNs -- every element the API defines comes back written.  other: once more on a workspace another
    configuration has just trained on (its activations, tags and tickets), after gt_workspace_init for this one.  Returns the runs made."""
    forms = forms or forms_of(cfg)
    runs = []
    with parity._deterministic(_lib_of(backend), deterministic):
        reset = not deterministic
        base = Session(backend, cfg, B, p, seq, flags, ws_fill=BASE).run_all(forms, reset)
        assert_written(base, "fill 7.25")
        for name in fills:
            if FILLS[name] == BASE:
                continue
            got = Session(backend, cfg, B, p, seq, flags, ws_fill=FILLS[name]).run_all(forms, reset)
            compare(got, base, "workspace fill %s against 7.25" % name, deterministic)
            runs.append(name)
        if prefill:
            got = Session(backend, cfg, B, p, seq, flags, ws_fill=QNAN, prefill=QNAN).run_all(forms, reset)
            assert_written(got, "outputs pre-filled with NaN")
            compare(got, base, "workspace and outputs pre-filled with NaN against 7.25", deterministic)
            runs.append("prefill")
        if other:
            ocfg, ob = other_config(backend, cfg, B)
            o = Session(backend, ocfg, ob, 0.1, True, 0, ws_fill=QNAN)
            o.run("step")
            o.run("sgd")
            got = Session(backend, cfg, B, p, seq, flags, ws_fill=1, adopt_ws=o.r.ws).run_all(forms, reset)
            compare(got, base, "workspace left by d_model %d at batch %d against 7.25" % (ocfg["d_model"], ob), deterministic)
            runs.append("other")
    return runs


def history_order(cfg, seed):
    """the form list in its fixed order, then once more in a seeded shuffle; a failing call after the first whole step and inside the shuffle"""
    forms = forms_of(cfg)
    again = list(forms)
    np.random.default_rng(seed).shuffle(again)
    order = forms + again
    order.insert(forms.index("sgd") + 1, "fail")
    order.insert(len(forms) + 1 + len(again) // 2, "fail")
    return order


def check_history_independence(backend, cfg, B, p, seq=True, flags=0, deterministic=True, seed=0):
    """ONE Runner through history_order(); after every form its results equal those of the same form on a FRESH Runner that received the
    parameters, moments and step state from just before it.  Where the previous call left the next step's weight packs, the history side
    passes GT_STEP_PACKS_CURRENT and the fresh side cannot: the folded packs are held to freshly packed ones, bit for bit.  Returns how many
    forms ran with the bit."""
    with_bit = 0
    with parity._deterministic(_lib_of(backend), deterministic):
        h = Session(backend, cfg, B, p, seq, flags)
        for i, name in enumerate(history_order(cfg, seed)):
            if name == "fail":
                keep = h.opt_state()
                h.train_step(0, 0, stats=False)
                compare(h.opt_state(), keep, "call %d: a failing gt_train_step" % i)
                continue
            before = h.opt_state()
            with_bit += bool(h.packs and name in STEP_FORMS)
            got = h.run(name, packs_bit=True)
            f = Session(backend, cfg, B, p, seq, flags)
            f.set_opt_state(before)
            named = lambda res: {name + "." + k: v for k, v in res.items()}
            compare(named(got), named(f.run(name)), "call %d (%s) of the history against a fresh Runner" % (i, name), deterministic)
    return with_bit


def check_redzones(backend, cfg, B, p, seq=True, flags=0, forms=None, x_short=0, deterministic=True):
    """The form list with every buffer between red zones of quiet NaNs, and again between red zones of 7.25: after every library call no
    red zone has changed by a bit (an out-of-bounds WRITE), and the two runs' results are bitwise equal (an out-of-bounds READ that reaches
    a result takes the pattern along; deterministic False: gradients, parameters and moments under compare()'s accumulation bar, where a
    NaN still fails)."""
    forms = forms or forms_of(cfg)
    res = []
    with parity._deterministic(_lib_of(backend), deterministic):
        for pattern in (QNAN, BASE):
            s = Session(backend, cfg, B, p, seq, flags, guard=pattern, x_short=x_short)

            def intact(call, s=s, pattern=pattern):
                bad = s.r.redzones_intact()
                assert not bad, "red zones (pattern 0x%08X) of %s changed during %s" % (pattern, bad, call)
            intact("the set-up")
            s.after_call = intact
            res.append(s.run_all(forms, not deterministic))
    compare(res[0], res[1], "results between red zones of NaN against red zones of 7.25", deterministic)
