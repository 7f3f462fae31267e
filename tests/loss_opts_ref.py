"""The loss with options (gt_loss_opts, include/groove_hip.h) restated in torch: fp64 by default, the gradient from autograd.  The
reference of tests/test_loss_opts.py and tests/test_loss_opts_gpu.py; `dtype=torch.float32` evaluates the same formulas in fp32 (the
yardstick for what fp32 arithmetic itself loses)."""
import numpy as np
import torch

VOICES = 9
NEUTRAL = dict(penalty_h=1.0, penalty_vo=None, pos_weight=1.0, voice_weight=1.0, focal_gamma=0.0, term_weight=(1.0, 1.0, 1.0))


def opts_f32(**kw):
    """the options as the kernel sees them: every value rounded to fp32, scalars broadcast over the voices"""
    o = dict(NEUTRAL, **kw)
    if o["penalty_vo"] is None:
        o["penalty_vo"] = o["penalty_h"]
    f = lambda a, n: np.broadcast_to(np.asarray(a, np.float32).reshape(-1), (n,)).copy()
    return dict(penalty_h=float(np.float32(o["penalty_h"])), penalty_vo=float(np.float32(o["penalty_vo"])),
                pos_weight=f(o["pos_weight"], VOICES), voice_weight=f(o["voice_weight"], VOICES),
                focal_gamma=float(np.float32(o["focal_gamma"])), term_weight=f(o["term_weight"], 3))


def terms(h, v, o, y, opts, dtype=torch.float64):
    """(bce, mv, mo, ok, bce0): (M,9) tensors of the per-element terms; h, v, o may require grad"""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    yh, yv, yo = y[:, :VOICES], y[:, VOICES:2 * VOICES], y[:, 2 * VOICES:]
    pw, vw = t(opts["pos_weight"]), t(opts["voice_weight"])
    one = torch.ones((), dtype=dtype)
    pen_h = torch.where(yh == 1, one, t(opts["penalty_h"]))
    pen_vo = torch.where(yh == 1, one, t(opts["penalty_vo"]))
    sp = torch.log1p(torch.exp(-h.abs()))
    bce0 = h.clamp(min=0) - h * yh + sp + (pw - 1) * yh * (sp + (-h).clamp(min=0))
    f = one
    if opts["focal_gamma"] != 0.0:
        q = yh * torch.sigmoid(-h) + (1 - yh) * torch.sigmoid(h)
        f = torch.where(q > 0, torch.where(q > 0, q, one) ** opts["focal_gamma"], torch.zeros((), dtype=dtype))
    bce = vw * pen_h * f * bce0
    mv = vw * pen_vo * (v - yv) ** 2
    mo = vw * pen_vo * (o - yo) ** 2
    ok = ((h > 0).to(dtype) == yh).to(dtype)
    return bce, mv, mo, ok, bce0


def restate(hvo, y, opts, wrt_logits=False, dtype=torch.float64):
    """hvo, y: (M,27) float32 arrays; opts: opts_f32(...).  -> (stats[8], voice_stats[36], d_out (M,27)) as float64 numpy arrays"""
    hvo_t = torch.as_tensor(np.asarray(hvo, np.float32)).to(dtype)
    y_t = torch.as_tensor(np.asarray(y, np.float32)).to(dtype)
    M = hvo_t.shape[0]
    h, v, o = (hvo_t[:, i * VOICES:(i + 1) * VOICES].clone().requires_grad_(True) for i in range(3))
    bce, mv, mo, ok, _ = terms(h, v, o, y_t, opts, dtype)
    tw = [float(a) for a in opts["term_weight"]]
    s3, s4, s5 = bce.sum() / M, mv.sum() / M, mo.sum() / M
    loss = (tw[0] * s3 + tw[1] * s4) + tw[2] * s5
    loss.backward()
    gh, gv, go = h.grad, v.grad, o.grad
    if wrt_logits:                                   # the head activations' derivative: v = sigmoid -> v (1 - v), o = 0.5 tanh -> 0.5 - 2 o^2
        gv = gv * (v * (1 - v)).detach()
        go = go * (0.5 - 2 * o * o).detach()
    stats = np.zeros(8)
    stats[0], stats[1], stats[3], stats[4], stats[5] = (float(t.detach()) for t in (loss, ok.mean(), s3, s4, s5))
    voice = torch.cat([bce.sum(0) / M, mv.sum(0) / M, mo.sum(0) / M, ok.sum(0) / M]).detach().double().numpy()
    return stats, voice, torch.cat([gh, gv, go], 1).detach().double().numpy()


def hit_counts(hvo, y):
    """exact per-voice counts of (h > 0) == y_h"""
    hvo, y = np.asarray(hvo, np.float32), np.asarray(y, np.float32)
    return ((hvo[:, :VOICES] > 0).astype(np.float32) == y[:, :VOICES]).sum(0)


def make_inputs(B, seed=0):
    """(hvo, y) (B*32, 27) float32: logits from N(0, 2) with planted +-30 and +-90 (on hits and on rests), v in [0,1] with exact 0 and 1,
    o in [-0.5, 0.5] with exact +-0.5, binary hits at about 10 % density"""
    rng = np.random.default_rng(seed)
    M = B * 32
    h = (rng.standard_normal((M, VOICES)) * 2.0).astype(np.float32)
    v = rng.uniform(0, 1, (M, VOICES)).astype(np.float32)
    o = rng.uniform(-0.5, 0.5, (M, VOICES)).astype(np.float32)
    yh = (rng.uniform(0, 1, (M, VOICES)) < 0.1).astype(np.float32)
    yh[0, 0], yh[1, 0] = 1.0, 0.0                    # (a hit and a rest whatever the draw)
    yv = rng.uniform(0, 1, (M, VOICES)).astype(np.float32)
    yo = rng.uniform(-0.5, 0.5, (M, VOICES)).astype(np.float32)
    plant = [30.0, -30.0, 90.0, -90.0]
    hits, rests = np.argwhere(yh == 1), np.argwhere(yh == 0)
    assert len(hits) >= len(plant) and len(rests) >= len(plant)
    for k, val in enumerate(plant):                  # every planted logit on a hit and on a rest
        for where in (hits, rests):
            r, c = where[k * len(where) // len(plant)]
            h[r, c] = val
    flat = rng.permutation(M * VOICES)[:8]
    v.reshape(-1)[flat[:2]], v.reshape(-1)[flat[2:4]] = 0.0, 1.0
    o.reshape(-1)[flat[4:6]], o.reshape(-1)[flat[6:8]] = 0.5, -0.5
    return np.concatenate([h, v, o], 1), np.concatenate([yh, yv, yo], 1)
