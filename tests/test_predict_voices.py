"""Per-voice generation controls (gt_predict_voices, gt_voice_select; include/groove_hip.h) without a GPU: the cap / mask pass against its
numpy restatement (tests/voice_sampling_ref.py) on constructed inputs, the whole call against the fp64 oracle (thresholds per voice;
a temperature T restated by dividing the hit rows of the oracle's output layer by T), its reduction to gt_predict / gt_predict_pd_at, and
the argument checks.  The kernels run in the host-emulator build of the same sources; tests/test_predict_voices_gpu.py repeats the
checks on the GPU."""
import ctypes
import functools

import numpy as np
import pytest

import voice_sampling_ref as vref
from harness import Runner, cfg_dict
from oracle import numpy_groove as ng
from parity import OUT_TOL
from transformergrooveinfilling_amd import _lib

MARGIN_TOL = 1e-4
THRES = [0.5, 0.45, 0.55, 0.5, 0.4, 0.6, 0.5, 0.48, 0.52]
CAPS = [32, 4, 2, 0, 8, 1, 3, 32, 5]
ENC = (cfg_dict(32, 4, 16, 2), 4)                   # sequence-resident path
ENCDEC = (cfg_dict(32, 4, 64, 2, 2), 3)             # greedy decode
SENTINEL = np.float32(7.5)


def _key(shape):
    cfg, B = shape
    return tuple(sorted(cfg.items())), B


@functools.lru_cache(maxsize=None)
def _inputs(key):
    """the fixed inputs of parity.check_predict for one shape: (cfg with dropout 0.3 -- predict is eval mode --, parameters, x)"""
    cfgk, B = key
    cfg = dict(dict(cfgk), dropout=0.3)
    P = ng.init_params(cfg, seed=21, perturb=0.05)
    x, _ = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=8)
    return cfg, P, x


@functools.lru_cache(maxsize=None)
def oracle(key, temperature):
    """fp64 oracle at per-voice thresholds THRES and a temperature: ((h, v, o), margin, probabilities); computed once per process"""
    cfg, P, x = _inputs(key)
    P64 = {k: a.astype(np.float64) for k, a in P.items()}
    P64["OutputLayer.Linear.weight"][:9] /= temperature
    P64["OutputLayer.Linear.bias"][:9] /= temperature
    hvo, margin = ng.predict(P64, cfg, x, thres=np.array(THRES), dtype=np.float64)
    prob = None
    if not cfg.get("num_decoder_layers", 0):
        (prob, _, _), _ = ng.predict(P64, cfg, x, use_thres=False, dtype=np.float64)
    return hvo, margin, prob


_RUNNERS = {}


def runner(backend, shape):
    k = (backend,) + _key(shape)
    if k not in _RUNNERS:
        cfg, P, _ = _inputs(_key(shape))
        _RUNNERS[k] = Runner(cfg, shape[1], backend)
        _RUNNERS[k].set_params(P)
    return _RUNNERS[k]


def predict_voices(r, x, vs, seed=0, first_seq=0):
    """gt_predict_voices through a Runner -> (hvo (B,32,27), prob (B,32,9))"""
    r.x = r.Buf(np.asarray(x, np.float32).reshape(r.M, -1))
    prob = r.Buf(np.full((r.M, 9), SENTINEL, np.float32))
    r.lib.call("gt_predict_voices", ctypes.byref(r.c), r.params.ptr, r.pe.ptr, r.x.ptr, r.hvo.ptr, ctypes.byref(vs), ctypes.c_uint32(seed),
               ctypes.c_int64(first_seq), prob.ptr, r.tgt.ptr, r.ws.ptr, r.stream)
    return r.hvo.numpy().reshape(r.B, 32, 27).copy(), prob.numpy().reshape(r.B, 32, 9).copy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ---- 1. gt_voice_select alone ------------------------------------------------------------------------------------------------------------
SELECT_CAPS = [0, 1, 2, 31, 32, 4, 31, 1, 2]


def _select_inputs(n_seq):
    """probabilities on a grid of 8 values in voices 0..3 (runs of exactly equal p), continuous elsewhere; per (sequence, voice) in turn
    all 32 steps hit, none, or a random subset; velocity / offset non-zero everywhere, so that a mask shows"""
    rng = np.random.default_rng(100 + n_seq)
    p = rng.random((n_seq, 32, 9), dtype=np.float32)
    p[..., :4] = np.round(p[..., :4] * 8) / 8
    h = (rng.random((n_seq, 32, 9)) < 0.6).astype(np.float32)
    kind = (np.arange(n_seq)[:, None] + np.arange(9)[None, :]) % 4
    h = np.where((kind == 0)[:, None, :], np.float32(1), h)
    h = np.where((kind == 1)[:, None, :], np.float32(0), h)
    vo = rng.uniform(0.1, 1.0, (n_seq, 32, 18)).astype(np.float32) * np.where(rng.random((n_seq, 32, 18)) < 0.5, -1, 1).astype(np.float32)
    return np.concatenate([h, vo], -1).astype(np.float32), p


def check_select(lib, Buf, n_seq, mask_vo, stream=None):
    hvo0, p = _select_inputs(n_seq)
    cnt = (hvo0[..., :9] != 0).sum(1)
    assert (cnt == 0).any() and (cnt == 32).any()                              # voices with no candidate and with all 32
    ties = [len(np.unique(p[s, hvo0[s, :, c] != 0, c])) < int(cnt[s, c]) for s in range(n_seq) for c in range(4) if cnt[s, c] > SELECT_CAPS[c]]
    assert any(ties)                                                           # equal probabilities among an over-full voice's hits
    vs = _lib.make_voice_sampling(0.5, SELECT_CAPS, 1.0, 0, mask_vo)
    hvo, prob = Buf(hvo0.copy()), Buf(p.copy())          # (a host buffer wraps its array: keep the originals)
    lib.call("gt_voice_select", hvo.ptr, prob.ptr, ctypes.byref(vs), ctypes.c_int64(n_seq), stream or ctypes.c_void_p(0))
    got = hvo.numpy().reshape(n_seq, 32, 27)
    want = vref.select(hvo0, p, SELECT_CAPS, mask_vo)
    assert _same_bits(got, want)
    assert ((got[..., :9] != 0).sum(1) <= np.array(SELECT_CAPS)[None, :]).all()
    assert not _same_bits(got[..., :9], hvo0[..., :9])                         # (the caps really dropped hits)
    if not mask_vo:
        assert _same_bits(got[..., 9:], hvo0[..., 9:])                         # velocity and offset come back untouched
    assert _same_bits(prob.numpy(), p)
    # every cap at 32 and no mask: nothing is launched, nothing changes
    hvo = Buf(hvo0.copy())
    lib.call("gt_voice_select", hvo.ptr, prob.ptr, ctypes.byref(_lib.make_voice_sampling()), ctypes.c_int64(n_seq), stream or ctypes.c_void_p(0))
    assert _same_bits(hvo.numpy().reshape(n_seq, 32, 27), hvo0)


@pytest.mark.parametrize("mask_vo", [False, True])
@pytest.mark.parametrize("n_seq", [1, 3, 67])
def test_voice_select_against_numpy(n_seq, mask_vo):
    r = runner("emu", ENC)
    check_select(r.lib, r.Buf, n_seq, mask_vo)


def test_tie_rule_keeps_the_earlier_step():
    """32 hits of one probability under a cap of 2: steps 0 and 1 stay"""
    r = runner("emu", ENC)
    hvo0 = np.zeros((1, 32, 27), np.float32)
    hvo0[..., :9] = 1
    p = np.full((1, 32, 9), 0.75, np.float32)
    p[0, 20, 1] = 0.8                                                           # voice 1: one larger value late in the pattern
    hvo, prob = r.Buf(hvo0.copy()), r.Buf(p)
    r.lib.call("gt_voice_select", hvo.ptr, prob.ptr, ctypes.byref(_lib.make_voice_sampling(0.5, 2)), ctypes.c_int64(1), r.stream)
    got = hvo.numpy().reshape(32, 27)[:, :9]
    assert [list(np.flatnonzero(got[:, c])) for c in range(3)] == [[0, 1], [0, 20], [0, 1]]


# ---- 2. end to end, encoder-only ---------------------------------------------------------------------------------------------------------
def check_encoder_only(backend, shape, temperature):
    r = runner(backend, shape)
    _, _, x = _inputs(_key(shape))
    (h, v, o), margin, prob_ref = oracle(_key(shape), temperature)
    free, pr = predict_voices(r, x, _lib.make_voice_sampling(THRES, 32, temperature))
    # (a) probabilities
    err = float(np.abs(pr - prob_ref).max())
    print("prob max-abs error %g (bar %g)" % (err, OUT_TOL))
    assert err < OUT_TOL
    # (b) uncapped hits where the oracle's margin allows; velocity / offset pass through
    sure = margin > MARGIN_TOL
    print("hit elements inside the margin: %d of %d" % (int((~sure).sum()), sure.size))
    assert (~sure).mean() <= 0.02
    assert np.array_equal(free[..., :9][sure], h[sure]) and set(np.unique(free[..., :9])) <= {0.0, 1.0}
    assert np.abs(free[..., 9:] - np.concatenate([v, o], -1)).max() < OUT_TOL
    assert _same_bits(free[..., :9], vref.decide(pr, THRES))                   # the decision is the documented function of prob_out
    # (c) capped: numpy select on the device's own probabilities and uncapped decisions, every group
    capped, pr2 = predict_voices(r, x, _lib.make_voice_sampling(THRES, CAPS, temperature))
    assert _same_bits(pr2, pr)
    assert _same_bits(capped, vref.select(free, pr, CAPS))
    over, groups = vref.over_cap_groups(free, CAPS)
    print("groups over their cap: %d of %d" % (over, groups))
    assert 3 * over >= groups
    assert ((capped[..., :9] != 0).sum(1) <= np.array(CAPS)[None, :]).all()
    # mask_vo: zero exactly where the final hit is 0, the unmasked values elsewhere
    masked, _ = predict_voices(r, x, _lib.make_voice_sampling(THRES, CAPS, temperature, mask_vo=True))
    assert _same_bits(masked[..., :9], capped[..., :9])
    on = np.tile(capped[..., :9] != 0, 2)
    assert _same_bits(masked[..., 9:], np.where(on, capped[..., 9:], np.float32(0)))
    assert _same_bits(masked, vref.select(free, pr, CAPS, True))


@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_encoder_only_against_oracle(temperature):
    check_encoder_only("emu", ENC, temperature)


# ---- 3. encoder-decoder ------------------------------------------------------------------------------------------------------------------
def check_encoder_decoder(backend, shape, temperature):
    r = runner(backend, shape)
    B = shape[1]
    _, _, x = _inputs(_key(shape))
    (h, v, o), margin, _ = oracle(_key(shape), temperature)
    free, pr = predict_voices(r, x, _lib.make_voice_sampling(THRES, 32, temperature))
    # each sequence up to (not including) its first step with a decision inside the margin: a flipped hit changes every later step
    sure = margin > MARGIN_TOL
    vo = np.concatenate([v, o], -1)
    compared = 0
    for b in range(B):
        unsure = np.flatnonzero(~sure[b].reshape(32, -1).all(1))
        t_end = int(unsure[0]) if len(unsure) else 32
        compared += t_end
        assert np.array_equal(free[b, :t_end, :9], h[b, :t_end]), (b, t_end)
        if t_end:
            assert np.abs(free[b, :t_end, 9:] - vo[b, :t_end]).max() < OUT_TOL, (b, t_end)
    print("compared decode steps: %d of %d" % (compared, 32 * B))
    assert compared > 0
    assert (pr != SENTINEL).all() and _same_bits(free[..., :9], vref.decide(pr, THRES))       # every step wrote its row of prob_out
    # the cap prunes the finished pattern (the decode fed the uncapped hits back)
    capped, pr2 = predict_voices(r, x, _lib.make_voice_sampling(THRES, CAPS, temperature))
    assert _same_bits(pr2, pr)
    assert _same_bits(capped, vref.select(free, pr, CAPS))
    over, groups = vref.over_cap_groups(free, CAPS)
    print("groups over their cap: %d of %d" % (over, groups))
    assert over > 0


@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_encoder_decoder_against_oracle(temperature):
    check_encoder_decoder("emu", ENCDEC, temperature)


# ---- 4. reduction to the existing calls --------------------------------------------------------------------------------------------------
REDUCTIONS = ("thres_0.5", "thres_0.3", "sampled")


def check_reduction(backend, shape, which):
    r = runner(backend, shape)
    _, _, x = _inputs(_key(shape))
    if which != "sampled":
        t = float(which.split("_")[1])
        want = r.predict(x, thres=t, use_thres=True)
        got, _ = predict_voices(r, x, _lib.make_voice_sampling(t))
        assert _same_bits(got, want)
        return
    seed, first = 20240229, 37
    r.x = r.Buf(np.asarray(x, np.float32).reshape(r.M, -1))
    r.lib.call("gt_predict_pd_at", ctypes.byref(r.c), r.params.ptr, r.pe.ptr, r.x.ptr, r.hvo.ptr, ctypes.c_uint32(seed), ctypes.c_int64(first),
               r.tgt.ptr, r.ws.ptr, r.stream)
    want = r.hvo.numpy().reshape(r.B, 32, 27).copy()
    got, pr = predict_voices(r, x, _lib.make_voice_sampling(0.0, mode=1), seed=seed, first_seq=first)
    assert _same_bits(got, want)
    assert 0.02 < float(got[..., :9].mean()) < 0.98                            # really sampled
    u = ng.pd_uniforms(seed, first + r.B)[first:]
    assert _same_bits(got[..., :9], vref.decide(pr, 0.0, u))


@pytest.mark.parametrize("which", REDUCTIONS)
@pytest.mark.parametrize("shape", [ENC, ENCDEC], ids=["enc", "encdec"])
def test_reduces_to_predict_and_predict_pd_at(shape, which):
    check_reduction("emu", shape, which)


# ---- 5. validation -----------------------------------------------------------------------------------------------------------------------
def _bad(**kw):
    vs = _lib.make_voice_sampling(THRES, CAPS)
    for k, val in kw.items():
        if isinstance(val, tuple):
            getattr(vs, k)[val[0]] = val[1]
        else:
            setattr(vs, k, val)
    return vs


REJECTED = {
    "thres_above_1": dict(vs=_bad(thres=(3, 1.5))), "thres_below_0": dict(vs=_bad(thres=(0, -0.01))), "thres_nan": dict(vs=_bad(thres=(8, float("nan")))),
    "cap_negative": dict(vs=_bad(max_count=(2, -1))), "cap_33": dict(vs=_bad(max_count=(7, 33))),
    "temperature_0": dict(vs=_bad(temperature=0.0)), "temperature_negative": dict(vs=_bad(temperature=-1.0)),
    "temperature_inf": dict(vs=_bad(temperature=float("inf"))), "temperature_nan": dict(vs=_bad(temperature=float("nan"))),
    "mode_2": dict(vs=_bad(mode=2)), "mode_negative": dict(vs=_bad(mode=-1)),
    "vs_null": dict(vs=None), "prob_null": dict(prob=False), "first_seq_negative": dict(first_seq=-1),
    "encdec_without_tgt_scratch": dict(shape=ENCDEC, tgt=False),
}


def check_rejected(backend, case):
    kw = dict(REJECTED[case])
    r = runner(backend, kw.get("shape", ENC))
    _, _, x = _inputs(_key(kw.get("shape", ENC)))
    r.x = r.Buf(np.asarray(x, np.float32).reshape(r.M, -1))
    r.hvo = r.Buf(np.full((r.M, 27), SENTINEL, np.float32))
    prob = r.Buf(np.full((r.M, 9), SENTINEL, np.float32))
    vs = kw.get("vs", _bad())
    rc = r.lib.cdll.gt_predict_voices(ctypes.byref(r.c), r.params.ptr, r.pe.ptr, r.x.ptr, r.hvo.ptr, ctypes.byref(vs) if vs is not None else None,
                                      ctypes.c_uint32(1), ctypes.c_int64(kw.get("first_seq", 0)), prob.ptr if kw.get("prob", True) else None,
                                      r.tgt.ptr if kw.get("tgt", True) else None, r.ws.ptr, r.stream)
    assert rc < 0
    assert b"gt_predict_voices" in r.lib.cdll.gt_last_error()
    assert (r.hvo.numpy() == SENTINEL).all() and (prob.numpy() == SENTINEL).all()
    if "vs" in kw:                                                              # gt_voice_select checks the same struct
        rc = r.lib.cdll.gt_voice_select(r.hvo.ptr, prob.ptr, ctypes.byref(vs) if vs is not None else None, ctypes.c_int64(r.B), r.stream)
        assert rc < 0 and b"gt_voice_select" in r.lib.cdll.gt_last_error()
        assert (r.hvo.numpy() == SENTINEL).all()


@pytest.mark.parametrize("case", list(REJECTED))
def test_rejected_before_any_launch(case):
    check_rejected("emu", case)


def test_struct_matches_header():
    assert ctypes.sizeof(_lib.GtVoiceSampling) == 4 * (9 + 9 + 3)
    assert [f[0] for f in _lib.GtVoiceSampling._fields_] == ["thres", "max_count", "temperature", "mode", "mask_vo"]
    with pytest.raises(ValueError):
        _lib.make_voice_sampling([0.5] * 8)


# ---- the host mirror on the emulator: engine.predict's keywords ---------------------------------------------------------------------------
def test_engine_predict_keywords_on_the_emulator():
    import torch
    from transformergrooveinfilling_amd.engine import StepEngine
    cfg, P, x = _inputs(_key(ENC))
    r = runner("emu", ENC)
    eng = StepEngine(batch_size=4, optimizer="sgd", learning_rate=0.05, hit_loss_penalty=0.47, seed=3, device="cpu", lib=r.lib,
                     **{k: cfg[k] for k in ("d_model", "n_heads", "dim_feedforward", "num_encoder_layers", "num_decoder_layers", "dropout",
                                            "embedding_size_src")})
    eng.load_named(P)
    xt = torch.from_numpy(x)
    calls = []
    call = r.lib.call
    try:
        r.lib.call = lambda name, *a: (calls.append(name), call(name, *a))[1]
        plain = eng.predict(xt, thres=0.4).numpy().copy()
        assert "gt_predict" in calls and "gt_predict_voices" not in calls       # all defaults: today's call sequence
        kw = dict(voice_thresholds=THRES, voice_max_count=CAPS, temperature=0.5, mask_vo=True)
        got = eng.predict(xt, **kw).numpy().copy()
        assert "gt_predict_voices" in calls
        # sampled mode: chunked as 2 + 2 or as one call of 4, the same samples
        a = eng.predict(xt, pd_seed=11, voice_max_count=CAPS, chunk=2).numpy().copy()
        b = eng.predict(xt, pd_seed=11, voice_max_count=CAPS, chunk=4).numpy().copy()
    finally:
        r.lib.call = call
    assert _same_bits(plain, r.predict(x, thres=0.4))
    want, _ = predict_voices(r, x, _lib.make_voice_sampling(THRES, CAPS, 0.5, 0, True))
    assert _same_bits(got, want)
    assert _same_bits(a, b) and ((a[..., :9] != 0).sum(1) <= np.array(CAPS)[None, :]).all()
    for bad in (dict(voice_thresholds=[0.5] * 8), dict(voice_max_count=[33] * 9), dict(temperature=0.0), dict(use_thres=False, mask_vo=True)):
        with pytest.raises(ValueError):
            eng.predict(xt, **bad)
