"""The loss options of the train step -- separate hit and velocity / offset penalties, pos_weight, voice and term weights, focal
modulation, per-voice statistics -- without a GPU: gt_loss_ex's kernel against the fp64 restatement of tests/loss_opts_ref.py,
gt_train_step_loss against forward / restated loss / backward and against the oracle's model, StepEngine.loss_opts, calculate_loss,
train_loop and train.py's configuration.  The kernels run in the host-emulator build of the same sources (tests/emu);
tests/test_loss_opts_gpu.py repeats the checks through the HIP library."""
import ctypes
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

import loss_opts_ref as ref
import parity
from harness import Runner, cfg_dict, emu_lib, run_ranks
from test_clip_grad_norm import ENGINE_DIMS, _engine, _ptr, _stream, _sync
from transformergrooveinfilling_amd import _lib, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PW = [0.5, 1.0, 2.0, 3.5, 6.0, 12.0, 1.5, 0.75, 9.0]
VW = [2.0, 1.5, 1.0, 0.0, 0.5, 0.25, 1.0, 3.0, 0.1]
# every option alone and all together; "defaults": every option neutral, penalty_vo = penalty_h
VARIANTS = {
    "defaults": dict(penalty_h=0.47),
    "penalties": dict(penalty_h=0.47, penalty_vo=0.0),
    "pos_weight": dict(penalty_h=0.47, pos_weight=PW),
    "voice_weight": dict(penalty_h=0.47, voice_weight=VW),
    "term_weight": dict(penalty_h=0.47, term_weight=(0.7, 2.0, 0.0)),
    "focal_0.5": dict(penalty_h=0.47, focal_gamma=0.5),
    "focal_2": dict(penalty_h=0.47, focal_gamma=2.0),
    "all_focal_0.5": dict(penalty_h=0.3, penalty_vo=0.05, pos_weight=PW, voice_weight=VW, term_weight=(0.7, 2.0, 0.4), focal_gamma=0.5),
    "all_focal_2": dict(penalty_h=0.3, penalty_vo=0.05, pos_weight=PW, voice_weight=VW, term_weight=(0.7, 2.0, 0.4), focal_gamma=2.0),
}
# batch 70: more workgroups (one per sequence) than the last arriver's 64 lanes cover in one stride
BATCHES = (1, 3, 70)
STAT_TOL, GRAD_TOL = 1e-5, 1e-5                     # the bars of tests/parity.py:83 and :87
# everything gt_loss_ex must refuse before any launch
REJECTED = [dict(penalty_h=-0.1), dict(penalty_vo=-1.0), dict(penalty_h=float("nan")), dict(penalty_vo=float("inf")),
            dict(pos_weight=[1.0] * 8 + [0.0]), dict(pos_weight=[-2.0] + [1.0] * 8), dict(pos_weight=[1.0] * 4 + [float("nan")] + [1.0] * 4),
            dict(pos_weight=float("inf")), dict(voice_weight=[1.0] * 8 + [-0.5]), dict(voice_weight=float("nan")),
            dict(term_weight=(1.0, -1.0, 1.0)), dict(term_weight=(1.0, 1.0, float("inf"))), dict(focal_gamma=-0.5), dict(focal_gamma=8.5),
            dict(focal_gamma=float("nan"))]


def raw_opts(**kw):
    """a GtLossOpts WITHOUT the host-side validation of _lib.make_loss_opts (the library's own checks are under test)"""
    o = ref.opts_f32(**{k: v for k, v in kw.items()})
    return _lib.GtLossOpts(o["penalty_h"], o["penalty_vo"], (ctypes.c_float * 9)(*o["pos_weight"]), (ctypes.c_float * 9)(*o["voice_weight"]),
                           o["focal_gamma"], (ctypes.c_float * 3)(*o["term_weight"]))


class LossCall:
    """gt_loss_ex on one batch size (lib: the emulator or the HIP library; device: where the buffers live)"""

    def __init__(self, lib, device, B):
        self.lib, self.device, self.B = lib, torch.device(device), B
        self.cfg = _lib.make_config(B, 16, 32, 4, 64, 1)
        n = int(lib.cdll.gt_loss_scratch_floats(ctypes.byref(self.cfg)))
        assert n >= 36 * B + 1
        self.scratch = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.stats = torch.full((8,), 7.0, dtype=torch.float32, device=self.device)
        self.voice = torch.full((36,), 7.0, dtype=torch.float32, device=self.device)
        self.d_out = torch.full((B * 32, 27), 7.0, dtype=torch.float32, device=self.device)

    def rc(self, hvo, y, lo, wrt_logits=0, stats=True, voice=True, d_out=True, scratch=True, null_hvo=False, null_y=False):
        return self.lib.cdll.gt_loss_ex(ctypes.byref(self.cfg), None if null_hvo else _ptr(hvo), None if null_y else _ptr(y),
                                        None if lo is None else ctypes.byref(lo), _ptr(self.stats) if stats else None,
                                        _ptr(self.voice) if voice else None, _ptr(self.d_out) if d_out else None, int(wrt_logits),
                                        _ptr(self.scratch) if scratch else None, _stream(self.device))

    def __call__(self, hvo, y, lo, wrt_logits=0, **kw):
        assert self.rc(hvo, y, lo, wrt_logits, **kw) == 0, self.lib.cdll.gt_last_error()
        _sync(self.device)
        return self.stats.cpu().numpy().copy(), self.voice.cpu().numpy().copy(), self.d_out.cpu().numpy().copy()


def check_kernel(lib, device, B, variant, wrt_logits):
    """gt_loss_ex against the fp64 restatement: stats, voice stats, hit accuracies, d_out, repeatability, the scratch contract.

    Measured over every case of this file: the largest stats error is 0.02 of the 1e-5 bar on the emulator and on the MI355X, the
    largest d_out rel_err 2.9e-7 on both -- the focal cases included, so the allowance of 4x torch's own fp32 error that a focal case
    over a bar could claim is not used: the plain bars hold."""
    kw = VARIANTS[variant]
    opts, lo = ref.opts_f32(**kw), _lib.make_loss_opts(**kw)
    hvo_np, y_np = ref.make_inputs(B, seed=B)
    want = ref.restate(hvo_np, y_np, opts, wrt_logits)
    call = LossCall(lib, device, B)
    hvo, y = torch.from_numpy(hvo_np).to(call.device), torch.from_numpy(y_np).to(call.device)
    stats, voice, d_out = call(hvo, y, lo, wrt_logits)
    M = B * 32
    worst = 0.0
    for i in (0, 3, 4, 5):
        e = abs(stats[i] - want[0][i]) / max(1.0, abs(want[0][i]))
        worst = max(worst, e)
        assert e <= STAT_TOL, (i, stats[i], want[0][i])
    assert stats[2] == 0.0 and stats[6] == 0.0 and stats[7] == 0.0
    for k in range(27):
        e = abs(voice[k] - want[1][k]) / max(1.0, abs(want[1][k]))
        worst = max(worst, e)
        assert e <= STAT_TOL, (k, voice[k], want[1][k])
    for q in range(3):                              # the voices' shares add up to the total
        assert abs(float(voice[9 * q:9 * q + 9].astype(np.float64).sum()) - stats[3 + q]) <= STAT_TOL * max(1.0, abs(want[0][3 + q])), q
    # hit accuracies: (h > 0) == y_h on fp32 inputs has no margin -- the counts are exact
    counts = ref.hit_counts(hvo_np, y_np)
    assert np.array_equal(np.rint(voice[27:].astype(np.float64) * M), counts) and np.abs(voice[27:] - counts / M).max() <= 1e-6
    assert round(float(stats[1]) * M * 9) == int(counts.sum()) and abs(stats[1] - counts.sum() / (M * 9)) <= 1e-6
    assert np.isfinite(d_out).all() and np.isfinite(stats).all() and np.isfinite(voice).all()
    err = parity.rel_err(d_out, want[2])
    print("%s B %d wrt_logits %d: stats %.3f of the bar, d_out rel_err %.3g" % (variant, B, wrt_logits, worst / STAT_TOL, err))
    assert err < GRAD_TOL, err
    assert float(call.scratch.abs().max()) == 0.0   # left zero: partials cleared, ticket re-armed
    again = call(hvo, y, lo, wrt_logits)            # bitwise repeatable
    for a, b in zip((stats, voice, d_out), again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert float(call.scratch.abs().max()) == 0.0
    # optional outputs: without voice_stats and d_out the same stats, nothing else written
    call.voice.fill_(7.0); call.d_out.fill_(7.0)
    s2, v2, d2 = call(hvo, y, lo, wrt_logits, voice=False, d_out=False)
    assert np.array_equal(s2.view(np.uint32), stats.view(np.uint32)) and (v2 == 7.0).all() and (d2 == 7.0).all()
    return worst / STAT_TOL, err


@pytest.mark.parametrize("wrt_logits", [0, 1])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("B", BATCHES)
def test_kernel_against_fp64_restatement(B, variant, wrt_logits):
    check_kernel(emu_lib(), "cpu", B, variant, wrt_logits)


def check_kernel_saturated(lib, device, B, wrt_logits):
    """gt_loss_ex where trained heads live: hit logits drawn as N(0, 20) (|h| up to 80: exp(|h|) overflows fp32 beyond 88, sigmoid(-|h|) and
    the focal factor q^gamma underflow towards 0), pos_weight set and focal_gamma = 2 -- DESIGN "loss options" claims that nothing overflows
    for finite logits.  Every output finite; statistics, voice statistics and d_out under check_kernel's fixed bars AND within
    regimes.NOISE_FACTOR x the error of the same restatement evaluated in fp32 (4-ulp floor): tests/regimes.py."""
    import regimes
    kw = dict(penalty_h=0.47, pos_weight=PW, focal_gamma=2.0)
    opts, lo = ref.opts_f32(**kw), _lib.make_loss_opts(**kw)
    hvo_np, y_np = ref.make_inputs(B, seed=B)
    hvo_np[:, :9] = (np.random.default_rng(B + 1000).standard_normal((B * 32, 9)) * 20.0).astype(np.float32)
    assert (np.abs(hvo_np[:, :9]) > 10).mean() > 0.5 and np.abs(hvo_np[:, :9]).max() > 50
    want = ref.restate(hvo_np, y_np, opts, wrt_logits)
    want32 = ref.restate(hvo_np, y_np, opts, wrt_logits, dtype=torch.float32)
    call = LossCall(lib, device, B)
    stats, voice, d_out = call(torch.from_numpy(hvo_np).to(call.device), torch.from_numpy(y_np).to(call.device), lo, wrt_logits)
    assert np.isfinite(d_out).all() and np.isfinite(stats).all() and np.isfinite(voice).all()
    noise = regimes.Noise()
    for i in (0, 3, 4, 5):
        e = noise.add("stats[%d]" % i, stats[i], want32[0][i], want[0][i], scale=max(1.0, abs(want[0][i])))
        assert e <= STAT_TOL, (i, stats[i], want[0][i])
    for k in range(27):
        e = noise.add("voice[%d]" % k, voice[k], want32[1][k], want[1][k], scale=max(1.0, abs(want[1][k])))
        assert e <= STAT_TOL, (k, voice[k], want[1][k])
    e = noise.add("d_out", d_out, want32[2], want[2])
    print("saturated B %d wrt_logits %d: d_out rel_err %.3g, worst noise ratio %.2f at %s" % (B, wrt_logits, e, noise.worst()[4], noise.worst()[0]))
    assert e < GRAD_TOL, e
    noise.check()
    counts = ref.hit_counts(hvo_np, y_np)
    assert np.array_equal(np.rint(voice[27:].astype(np.float64) * B * 32), counts)
    return noise


@pytest.mark.parametrize("wrt_logits", [0, 1])
def test_kernel_against_fp64_restatement_saturated(wrt_logits):
    check_kernel_saturated(emu_lib(), "cpu", 3, wrt_logits)


def check_defaults_match_gt_loss(lib, device, B):
    """every option neutral, penalty_vo = penalty_h: d_out bit for bit gt_loss's, stats within the bar"""
    call = LossCall(lib, device, B)
    hvo_np, y_np = ref.make_inputs(B, seed=B)
    hvo, y = torch.from_numpy(hvo_np).to(call.device), torch.from_numpy(y_np).to(call.device)
    stats, _, d_out = call(hvo, y, _lib.make_loss_opts(penalty_h=0.47))
    s0 = torch.zeros(8, dtype=torch.float32, device=call.device)
    d0 = torch.zeros_like(call.d_out)
    lib.call("gt_loss", ctypes.byref(call.cfg), _ptr(hvo), _ptr(y), ctypes.c_float(0.47), _ptr(s0), _ptr(d0), _stream(call.device))
    _sync(call.device)
    assert np.array_equal(d_out.view(np.uint32), d0.cpu().numpy().view(np.uint32))
    s0 = s0.cpu().numpy()
    for i in (0, 1, 3, 4, 5):
        assert abs(stats[i] - s0[i]) <= STAT_TOL * max(1.0, abs(s0[i])), (i, stats[i], s0[i])


@pytest.mark.parametrize("B", BATCHES)
def test_defaults_are_gt_loss(B):
    check_defaults_match_gt_loss(emu_lib(), "cpu", B)


def check_rejected(lib, device):
    """every rejected argument combination returns < 0 with a message and launches nothing"""
    B = 3
    call = LossCall(lib, device, B)
    hvo_np, y_np = ref.make_inputs(B, seed=1)
    hvo, y = torch.from_numpy(hvo_np).to(call.device), torch.from_numpy(y_np).to(call.device)
    good = raw_opts(penalty_h=0.47)
    cases = [(raw_opts(**kw), {}) for kw in REJECTED]
    cases += [(None, {}), (good, dict(null_hvo=True)), (good, dict(null_y=True)), (good, dict(stats=False)), (good, dict(scratch=False))]
    for lo, kw in cases:
        assert call.rc(hvo, y, lo, **kw) < 0, (None if lo is None else _lib.loss_opts_tuple(lo), kw)
        assert lib.cdll.gt_last_error()
    _sync(call.device)
    assert (call.stats == 7.0).all() and (call.voice == 7.0).all() and (call.d_out == 7.0).all() and float(call.scratch.abs().max()) == 0.0
    for kw in REJECTED:                             # ... and the host-side constructor refuses the same values
        with pytest.raises(ValueError):
            _lib.make_loss_opts(**kw)
    with pytest.raises(ValueError, match="expected 1 or 9"):
        _lib.make_loss_opts(pos_weight=[1.0, 2.0])


def test_rejected_arguments_launch_nothing():
    check_rejected(emu_lib(), "cpu")


def test_struct_layout_matches_the_header():
    src = open(os.path.join(ROOT, "include", "groove_hip.h")).read()
    body = re.search(r"typedef struct gt_loss_opts \{(.*?)\} gt_loss_opts;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"GT_VOICES": 9}
    fields = []
    for m in re.finditer(r"float\s+(\w+)(?:\[(\w+)\])?\s*;", body):
        n = m.group(2)
        fields.append((m.group(1), 1 if n is None else int(sizes.get(n, n))))
    assert fields == [("penalty_h", 1), ("penalty_vo", 1), ("pos_weight", 9), ("voice_weight", 9), ("focal_gamma", 1), ("term_weight", 3)]
    got = [(n, ctypes.sizeof(t) // 4) for n, t in _lib.GtLossOpts._fields_]
    assert got == fields
    assert all((t._type_ if hasattr(t, "_length_") else t) is ctypes.c_float for _, t in _lib.GtLossOpts._fields_)
    assert ctypes.sizeof(_lib.GtLossOpts) == 4 * sum(n for _, n in fields) == 96
    off = 0
    for n, k in fields:
        assert getattr(_lib.GtLossOpts, n).offset == off, n
        off += 4 * k
    for name in ("gt_loss_scratch_floats", "gt_loss_ex", "gt_train_step_loss"):
        assert name in _lib.EXPORTS


def test_pos_weight_term_is_stock_torch():
    """the restatement's bce0 against F.binary_cross_entropy_with_logits(pos_weight=...) in fp64"""
    hvo, y = ref.make_inputs(3, seed=5)
    h, yt = torch.from_numpy(hvo[:, :9]).double(), torch.from_numpy(y).double()
    opts = ref.opts_f32(pos_weight=PW)
    bce0 = ref.terms(h, torch.zeros_like(h), torch.zeros_like(h), yt, opts)[4]
    stock = torch.nn.functional.binary_cross_entropy_with_logits(h, yt[:, :9], pos_weight=torch.tensor(PW, dtype=torch.float64), reduction="none")
    assert float((bce0 - stock).abs().max()) <= 1e-12 * float(stock.abs().max())


# ---- gt_train_step_loss ---------------------------------------------------------------------------------------------------------------
# name: (configuration, batch, Runner's seq switch): the emulator's equivalents of the schedules -- one workgroup per sequence, the
# four-workgroups-per-sequence forward with rider weight gradients (where gt_train_step runs its forward on into backward phase 0), one
# kernel per operation, encoder-decoder
STEP_CASES = {
    "seq_d32": (cfg_dict(32, 4, 16, 2), 2, True),
    "rider_d128": (cfg_dict(128, 4, 64, 3), 2, "split"),
    "op_d48": (cfg_dict(48, 4, 24, 2), 2, False),
    "op_encdec_d32": (cfg_dict(32, 4, 16, 1, 1), 2, False),
}
STEP_VARIANT = "all_focal_2"


def step_loss(r, x, y, lo, skip_update=1, algo=0):
    """gt_train_step_loss on a harness.Runner -> (stats[8], voice_stats[36])"""
    r.x = r.Buf(np.asarray(x, np.float32).reshape(r.M, -1))
    r.y = r.Buf(np.asarray(y, np.float32).reshape(r.M, 27))
    if getattr(r, "_grads_dirty", False):          # the precondition of gt_train_step: grads are zero on entry
        r.grads = r.Buf(np.zeros(r.total, np.float32))
        r._grads_dirty = False
    if not hasattr(r, "loss_scratch"):
        r.loss_scratch = r.Buf(np.zeros(int(r.lib.cdll.gt_loss_scratch_floats(ctypes.byref(r.c))), np.float32))
        r.voice = r.Buf(np.zeros(36, np.float32))
    r.lib.call("gt_train_step_loss", ctypes.byref(r.c), algo, r.params.ptr, r.grads.ptr, None, None, r.pe.ptr, r.x.ptr, r.y.ptr,
               ctypes.byref(lo), r.voice.ptr, r.loss_scratch.ptr, r.hvo.ptr, r.stats.ptr, r.tgt.ptr, r.ws.ptr, r.state.ptr, int(skip_update),
               r.stream)
    r._grads_dirty = bool(skip_update)
    assert float(np.abs(r.loss_scratch.numpy()).max()) == 0.0
    return r.stats.numpy().copy(), r.voice.numpy().copy()


def check_stats(stats, voice, want):
    for i in (0, 1, 3, 4, 5):
        assert abs(stats[i] - want[0][i]) <= STAT_TOL * max(1.0, abs(want[0][i])), (i, stats[i], want[0][i])
    assert np.abs(voice - want[1]).max() <= STAT_TOL * max(1.0, float(np.abs(want[1]).max()))


def check_step_teacher_forced(backend, cfg, B, seq, p=0.1):
    """gt_train_step_loss(skip_update = 1) against gt_forward(train = 1) on the same state, the restated fp64 d_hvo cast to fp32, gt_backward"""
    from oracle import numpy_groove as ng
    cfg = dict(cfg, dropout=p)
    kw = VARIANTS[STEP_VARIANT]
    opts, lo = ref.opts_f32(**kw), _lib.make_loss_opts(**kw)
    r = Runner(cfg, B, backend, rng=(1234, 99, 7), seq=seq)
    r.set_params(ng.init_params(cfg, seed=3, perturb=0.05))
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=5)
    stats, voice = step_loss(r, x, y, lo, skip_update=1)
    G1 = r.unflatten(r.grads.numpy())
    assert r.step_state().step == 7                # (no update: the dropout stream stays, the forward below draws the same masks)
    tgt = parity.shift_right(y) if cfg.get("num_decoder_layers", 0) else None
    hvo = r.forward(x, tgt, train=True).reshape(r.M, 27)
    want = ref.restate(hvo, y.reshape(r.M, 27), opts, wrt_logits=False)
    check_stats(stats, voice, want)
    G2 = r.backward(want[2].astype(np.float32), train=True)
    assert set(G1) == set(G2)
    worst = 0.0
    for k in G2:
        err = float(np.abs(G1[k] - G2[k]).max() / max(np.abs(G2[k]).max(), 1e-5))
        worst = max(worst, err)
        assert err < parity.GRAD_TOL, (k, err)
    print("teacher-forced: worst gradient tensor %.3g of GRAD_TOL" % (worst / parity.GRAD_TOL))


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_step_teacher_forced(case):
    check_step_teacher_forced("emu", *STEP_CASES[case])


def oracle_grads(cfg, P, x, y, opts):
    """one step's gradients of oracle.torch_groove's model (fp64, dropout 0) under the restated loss -> {state-dict name: array}"""
    from oracle import torch_groove as tg
    m = tg.build(dict(cfg, dropout=0.0)).double()
    sd = m.state_dict()
    for k in sd:
        if k in P:
            sd[k] = torch.from_numpy(np.asarray(P[k], np.float64)).reshape(sd[k].shape)
    m.load_state_dict(sd)
    m.train()
    xt, yt = torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(y, np.float64))
    h, v, o = m(xt) if cfg.get("num_decoder_layers", 0) == 0 else m(xt, tg.shift_right(yt))
    M = xt.shape[0] * 32
    bce, mv, mo, _, _ = ref.terms(h.reshape(M, 9), v.reshape(M, 9), o.reshape(M, 9), yt.reshape(M, 27), opts)
    tw = [float(a) for a in opts["term_weight"]]
    ((tw[0] * bce.sum() / M + tw[1] * mv.sum() / M) + tw[2] * mo.sum() / M).backward()
    return {k: t.grad.numpy() for k, t in m.named_parameters()}


def check_step_against_oracle(backend, cfg, B, seq):
    from oracle import numpy_groove as ng
    cfg = dict(cfg, dropout=0.0)
    kw = VARIANTS[STEP_VARIANT]
    opts, lo = ref.opts_f32(**kw), _lib.make_loss_opts(**kw)
    P = ng.init_params(cfg, seed=3, perturb=0.05)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=5)
    r = Runner(cfg, B, backend, seq=seq)
    r.set_params(P)
    step_loss(r, x, y, lo, skip_update=1)
    G, Gr = r.unflatten(r.grads.numpy()), oracle_grads(cfg, P, x, y, opts)
    assert set(G) <= set(Gr)
    worst = 0.0
    for k in G:
        err = float(np.abs(G[k] - Gr[k]).max() / max(np.abs(Gr[k]).max(), 1e-5))
        worst = max(worst, err)
        assert err < parity.GRAD_TOL, (k, err)
    print("oracle: worst gradient tensor %.3g of GRAD_TOL" % (worst / parity.GRAD_TOL))


@pytest.mark.parametrize("case", ["rider_d128", "op_encdec_d32"])
def test_step_against_oracle_model(case):
    check_step_against_oracle("emu", *STEP_CASES[case])


def check_default_options_track_gt_train_step(backend, cfg, B, seq, p=0.1):
    """neutral options: three whole steps of gt_train_step_loss and of gt_train_step from the same start.  Not bitwise (the loss sums run
    in another order); per tensor within parity's update bar over the three steps' movement: GRAD_TOL of the tensor's largest
    movement (floor lr * 1e-5), plus one fp32 ulp of the parameter per step.
    Both runs take the weight gradients WITHOUT the token split (gt_set_deterministic).  With it the fp32 atomic adds of the GPU leave
    last-bit noise in every step's parameters, and over three free-running steps that noise now and then carries a ReLU pre-activation
    across its kink in ONE of the two runs -- either one: gt_train_step against itself does the same.  Measured on an MI355X at the
    d32 / 16-head shape, 2 runs of 6: element [201, 9] of layer 1's linear1.weight 2.2e-6 apart (6.6 x this bar), everything else within
    0.07 of it.  Two trajectories on different sides of a kink are both right and say nothing about the loss kernel."""
    lib = emu_lib() if backend == "emu" else _lib.get_lib()
    lib.cdll.gt_set_deterministic(1)
    try:
        _check_default_options_track(backend, dict(cfg, dropout=p), B, seq)
    finally:
        lib.cdll.gt_set_deterministic(0)


def _check_default_options_track(backend, cfg, B, seq):
    from oracle import numpy_groove as ng
    P = ng.init_params(cfg, seed=3, perturb=0.05)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=5)
    lr = 0.094
    a, b = (Runner(cfg, B, backend, rng=(1234, 99, 7), lr=lr, seq=seq) for _ in range(2))
    lo = _lib.make_loss_opts(penalty_h=0.47)
    for r in (a, b):
        r.set_params(P)
    for _ in range(3):
        sa, _ = step_loss(a, x, y, lo, skip_update=0)
        sb = b.train_step(x, y, 0.47)
        for i in (0, 1, 3, 4, 5):
            assert abs(sa[i] - sb[i]) <= 2 * STAT_TOL * max(1.0, abs(sb[i])), (i, sa[i], sb[i])
    assert a.step_state().step == b.step_state().step == 10 and a.step_state().opt_step == 3
    pa, pb = a.unflatten(a.params.numpy()), b.unflatten(b.params.numpy())
    for k in pb:
        move = float(np.abs(pb[k].astype(np.float64) - P[k]).max())
        bar = parity.GRAD_TOL * max(move, lr * 1e-5) + 3 * np.spacing(np.abs(pb[k])).astype(np.float64)
        assert (np.abs(pa[k].astype(np.float64) - pb[k]) <= bar).all(), k
    assert float(np.abs(a.grads.numpy()).max()) == 0.0       # the update left the gradients zeroed, as gt_train_step's does


@pytest.mark.parametrize("case", ["seq_d32", "rider_d128", "op_d48"])
def test_default_options_track_gt_train_step(case):
    check_default_options_track_gt_train_step("emu", *STEP_CASES[case])


def test_train_step_loss_rejects_before_any_launch():
    from oracle import numpy_groove as ng
    cfg, B, seq = STEP_CASES["seq_d32"]
    r = Runner(cfg, B, "emu", seq=seq)
    r.set_params(ng.init_params(cfg, seed=3, perturb=0.05))
    x, y = ng.synthetic_batch(B, 16, seed=5)
    step_loss(r, x, y, _lib.make_loss_opts(penalty_h=0.47), skip_update=1)
    keep = (r.grads.numpy().copy(), r.hvo.numpy().copy(), r.state.numpy().copy())
    for kw in REJECTED[:3] + [dict(focal_gamma=9.0)]:
        with pytest.raises(_lib.GrooveLibError, match="penalty|focal_gamma"):
            r._grads_dirty = False
            step_loss(r, x, y, raw_opts(**kw), skip_update=1)
    assert all(np.array_equal(a, b) for a, b in zip(keep, (r.grads.numpy(), r.hvo.numpy(), r.state.numpy())))


# ---- StepEngine -----------------------------------------------------------------------------------------------------------------------
ENGINE_OPTS = dict(vo_penalty=0.05, pos_weight=PW, voice_weight=VW, focal_gamma=2.0, term_weights=(0.7, 2.0, 0.4))


def engine_opts_tuple(penalty=0.47, **kw):
    kw = dict(ENGINE_OPTS, **kw)
    return _lib.loss_opts_tuple(_lib.make_loss_opts(penalty, kw["vo_penalty"], kw["pos_weight"], kw["voice_weight"], kw["focal_gamma"], kw["term_weights"]))


def _batch(B, device="cpu"):
    x, y = layout.synthetic_batch(B, 16, seed=9)
    return torch.from_numpy(x).to(device), torch.from_numpy(y).to(device)


def check_engine_off_is_bitwise_unchanged(make, B, device="cpu"):
    """loss_opts = None: graph keys, three steps' stats and parameters bitwise those of an engine that never heard of the options"""
    x, y = _batch(B, device)
    for optimizer in ("sgd", "adam"):
        a, b = make(optimizer), make(optimizer, loss_opts=None)
        assert b._lk == () and b._split_recipe(b.slot(B), "fused") is None
        for _ in range(3):
            sa, sb = a.train_step(x, y).clone(), b.train_step(x, y).clone()
            assert torch.equal(sa, sb) and torch.equal(a.params, b.params)
        assert list(b.slot(B).graphs) == list(a.slot(B).graphs)
        assert all(k == ("fused", b.algo, b.penalty) for k in b.slot(B).graphs)
        assert b.slot(B).voice_stats is None and b.slot(B).loss_scratch is None     # (nothing of the options is even allocated)
    return b


@pytest.mark.parametrize("case", list(ENGINE_DIMS))
def test_engine_without_options_is_bitwise_unchanged(case):
    check_engine_off_is_bitwise_unchanged(lambda opt, **kw: _engine(ENGINE_DIMS[case], 4, opt, **kw), 4)


def check_engine_step_against_module_sequence(eng, twin, B, device="cpu", steps=3):
    """the engine's step with options against forward / StepEngine.loss(opts) (gt_loss_ex) / backward / update on a twin, teacher-forced
    (the twin starts every step from the engine's parameters and step state); stats, voice stats and parameters agree to fp32 rounding"""
    x, y = _batch(B, device)
    opts = eng.loss_opts
    for step in range(steps):
        twin.params.copy_(eng.params); twin.state.copy_(eng.state)
        st = eng.train_step(x, y).clone()
        vs = eng.mean_voice_stats(eng.slot(B)).clone()
        s = twin.slot(B)
        twin.forward(x, None if twin.encoder_only else torch.cat([torch.zeros_like(y[:, :1]), y[:, :-1]], 1), train=True)
        st2, d_hvo = twin.loss(s, y, 0.0, opts=opts)
        twin.grads.zero_()
        twin.backward(s, d_hvo, train=True)
        twin.enqueue_update(slot=s)
        assert float((st - st2).abs().max()) <= 2e-5 and float((vs - s.voice_stats).abs().max()) <= 2e-5, step
        assert float(vs[27:].sum()) > 0 and abs(float(vs[27:].mean()) - float(st[1])) <= 1e-6
        assert float((eng.params - twin.params).abs().max()) <= 1e-6, step
        assert eng.state_struct().opt_step == step + 1 and float(eng.grads.abs().max()) == 0.0


@pytest.mark.parametrize("case", list(ENGINE_DIMS))
def test_engine_step_with_options_matches_module_sequence(case):
    make = lambda **kw: _engine(ENGINE_DIMS[case], 4, "sgd", **kw)
    check_engine_step_against_module_sequence(make(loss_opts=engine_opts_tuple()), make(), 4)


def test_engine_options_are_validated_and_keyed():
    eng = _engine(ENGINE_DIMS["seq_d32"], 2)
    t = eng.make_loss_opts(**ENGINE_OPTS)
    assert t == engine_opts_tuple() and hash(t) is not None and len(t) == 24
    assert eng.make_loss_opts()[:2] == (np.float32(0.47), np.float32(0.47))       # penalty_vo = penalty_h = the engine's hit_loss_penalty
    eng.loss_opts = t
    assert eng._lk == (t,)
    assert eng._split_recipe(eng.slot(2), "fused") is None                        # (no clip, no extras: the fused key + the tuple)
    eng.max_grad_norm = 1.0
    assert eng._split_recipe(eng.slot(2), "fused")[0] == ("fused_clip", 0, 0.47, t, 1.0)
    eng.max_grad_norm = None
    x, y = _batch(2)
    for bad in ((1.0, 2.0), t[:20] + (9.0,) + t[21:], "focal", t[:2] + (0.0,) + t[3:]):
        eng.loss_opts = bad
        before = eng.state.clone()
        with pytest.raises(ValueError):
            eng.train_step(x, y)
        assert torch.equal(eng.state, before) and float(eng.grads.abs().max()) == 0.0
    for kw in (dict(pos_weight=[1.0, 2.0]), dict(voice_weight=[-1.0] * 9), dict(focal_gamma=-1.0), dict(term_weights=(1.0, 1.0))):
        with pytest.raises(ValueError):
            eng.make_loss_opts(**kw)


@pytest.mark.parametrize("variant,max_norm", [("sgd_nesterov_wd", None), ("adamw", None), ("sgd_nesterov_wd", "clip")])
def test_clipped_and_extras_recipes_still_match_torch(variant, max_norm):
    from test_optimizer_prepare import ENGINE_VARIANTS, check_engine_against_torch
    from test_clip_grad_norm import torch_clip_on
    optimizer, kw = ENGINE_VARIANTS[variant]
    t = engine_opts_tuple()
    x, y = _batch(4)
    extra = {}
    if max_norm is not None:
        probe = _engine(ENGINE_DIMS["seq_d32"], 4, optimizer, loss_opts=t)
        box = []
        probe.train_step(x, y, on_grads=lambda: box.append(torch_clip_on(probe, float("inf"))))
        extra = dict(max_grad_norm=0.3 * box[0])
    eng, twin = (_engine(ENGINE_DIMS["seq_d32"], 4, optimizer, loss_opts=t, **kw, **extra) for _ in range(2))
    check_engine_against_torch(eng, optimizer, kw, x, y, max_norm=extra.get("max_grad_norm"), twin=twin)
    plain = _engine(ENGINE_DIMS["seq_d32"], 4, optimizer, **kw, **extra)           # (the options do reach the gradients)
    plain.train_step(x, y)
    assert float((plain.params - eng.params).abs().max()) > 1e-4


def test_indexed_and_watched_steps_take_the_options():
    t = engine_opts_tuple()
    a, b, c = (_engine(ENGINE_DIMS["seq_d32"], 4, "sgd", loss_opts=t) for _ in range(3))
    x, y = _batch(4)
    xs, ys = torch.cat([x, x]), torch.cat([y, y])
    for _ in range(2):
        a.train_step(x, y, on_grads=lambda: None)
        b.train_step(x, y)
        c.train_step_indexed(xs, ys, torch.arange(4, 8))
    assert float((a.params - b.params).abs().max()) <= 1e-6 and torch.equal(b.params, c.params)
    assert torch.equal(b.slot(4).voice_stats, c.slot(4).voice_stats) and torch.equal(a.slot(4).voice_stats, b.slot(4).voice_stats)


# ---- data parallel over gloo --------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out, case):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from harness import emu_lib
    from test_loss_opts import engine_opts_tuple
    from transformergrooveinfilling_amd import layout, parallel
    from transformergrooveinfilling_amd.engine import StepEngine
    parallel.init_distributed("gloo")
    lib = emu_lib()
    for f in ("gt_set_seq_quad", "gt_set_seq_split", "gt_set_seq_ride"):
        getattr(lib.cdll, f)(-1)
    lib.cdll.gt_set_seq(1)
    dims = dict(ENGINE_DIMS[case], num_decoder_layers=0, dropout=0.0, embedding_size_src=16)
    B = 4
    eng = StepEngine(batch_size=B // world, optimizer="sgd", learning_rate=0.05, hit_loss_penalty=0.47, seed=3 | (rank << 32),
                     device="cpu", world_size=world, lib=lib, loss_opts=engine_opts_tuple(), **dims)
    eng.load_named(layout.init_params(dims, seed=5))
    x, y = layout.synthetic_batch(B, 16, seed=9)
    sl = slice(rank * (B // world), (rank + 1) * (B // world))
    for _ in range(2):
        eng.train_step(torch.from_numpy(x[sl]), torch.from_numpy(y[sl]))
    s = eng.slot(B // world)
    torch.save({"params": eng.params.clone(), "stats": eng.mean_stats(s).clone(), "voice": eng.mean_voice_stats(s).clone()}, out % rank)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", list(ENGINE_DIMS))
def test_data_parallel_step_agrees_across_ranks(tmp_path, case):
    B, world = 4, 2
    out = str(tmp_path / "lo%d.pt")
    run_ranks(_dp_worker, world, out, case)
    a, b = torch.load(out % 0), torch.load(out % 1)
    assert torch.equal(a["params"], b["params"]) and torch.equal(a["stats"], b["stats"]) and torch.equal(a["voice"], b["voice"])
    single = _engine(ENGINE_DIMS[case], B, dropout=0.0, loss_opts=engine_opts_tuple())
    x, y = _batch(B)
    for _ in range(2):
        st = single.train_step(x, y)
    assert float((a["params"] - single.params).abs().max()) <= 1e-6          # two half batches average to the whole batch's mean
    assert float((a["stats"][:6] - st[:6]).abs().max()) <= 2e-5 and float((a["voice"] - single.slot(B).voice_stats).abs().max()) <= 2e-5


# ---- train.py ---------------------------------------------------------------------------------------------------------------------------
def test_train_cli_and_yaml_keys(tmp_path):
    sys.path.insert(0, ROOT)
    import train
    p = train.build_parser()
    off = train.load_hyperparameters(p.parse_args(["--experiment", "X"]))
    assert all(off[k] is None for k in ("pos_weight", "voice_weight", "focal_gamma", "vo_penalty", "loss_weights"))
    assert train.loss_setup(off) == ({}, None)
    nine = ",".join(str(v) for v in PW)
    hp = train.load_hyperparameters(p.parse_args(["--experiment", "X", "--pos_weight", nine, "--voice_weight", ",".join(str(v) for v in VW),
                                                  "--focal_gamma", "2", "--vo_penalty", "0.05", "--loss_weights", "0.7,2,0.4"]))
    assert hp["pos_weight"] == PW and hp["voice_weight"] == VW and hp["focal_gamma"] == 2.0 and hp["vo_penalty"] == 0.05
    assert train.loss_setup(hp) == ({"pos_weight": PW}, dict(voice_weight=VW, focal_gamma=2.0, vo_penalty=0.05, term_weights=[0.7, 2.0, 0.4]))
    assert train.load_hyperparameters(p.parse_args(["--experiment", "X", "--pos_weight", "3"]))["pos_weight"] == [3.0]
    for bad in (["--pos_weight", "1,2"], ["--voice_weight", "1,2,3"], ["--loss_weights", "1,2"]):
        with pytest.raises(SystemExit):
            train.load_hyperparameters(p.parse_args(["--experiment", "X"] + bad))
    cfgs = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "reference_configs", "*.yaml")))
    assert cfgs
    for f in cfgs:                                        # the reference's YAMLs lack the keys: the plain loss, as there
        assert train.loss_setup(train.load_hyperparameters(p.parse_args(["--config", f]))) == ({}, None), f
    yml = tmp_path / "lo.yaml"
    yml.write_text(open(cfgs[0]).read() + "\npos_weight: [%s]\nvoice_weight: '%s'\nfocal_gamma: 0.5\nvo_penalty: 0\nloss_weights: [1, 0.5, 0.25]\n"
                   % (nine, ",".join(str(v) for v in VW)))
    hp = train.load_hyperparameters(p.parse_args(["--config", str(yml)]))
    assert train.loss_setup(hp) == ({"pos_weight": PW}, dict(voice_weight=VW, focal_gamma=0.5, vo_penalty=0.0, term_weights=[1.0, 0.5, 0.25]))
