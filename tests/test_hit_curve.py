"""Per-voice hit threshold curves (gt_hit_curve, gt_hit_thresholds; include/groove_hip.h) without a GPU: the counting pass against its numpy
restatement (tests/hit_curve_ref.py) on constructed inputs -- every integer equal --, accumulation over calls, the one-bin case, the
argument checks, the choice against the restatement, and the whole path from the device's own probabilities against the fp64 oracle.  The
kernels run in the host-emulator build of the same sources; tests/test_hit_curve_gpu.py repeats the checks on the GPU."""
import ctypes
import functools

import numpy as np
import pytest

import hit_curve_ref as href
from harness import NpBuf, emu_lib
from oracle import numpy_groove as ng
from test_predict_voices import ENC, ENCDEC, MARGIN_TOL, THRES, _inputs, _key, oracle, runner
from transformergrooveinfilling_amd import _lib

HIT_RATES = [.25, .2, .5, .05, .02, .02, .02, .01, 0]
SENTINEL64 = (1 << 33) + 5
GAP_MIN = 1e-9


def grid_of(n_thres):
    """1: one threshold; 9: tenths; 99: the engine's default; 127: k / 128 -- exact in fp32, with every sixteenth on it"""
    if n_thres == 1:
        return np.array([0.5], np.float32)
    den = {9: 10, 99: 100, 127: 128}[n_thres]
    return (np.arange(1, n_thres + 1).astype(np.float32) / np.float32(den)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(n_seq):
    """(prob (n_seq * 32, 9) fp32, hvo_gt (n_seq * 32, 27)): skewed probabilities that lean towards the ground truth; voice 0 rounded to
    sixteenths (runs of equal p, values exactly ON grid points); voice 8 never hit; one NaN, one 0.0 and one 1.0 in voice 1"""
    rng = np.random.default_rng(4000 + n_seq)
    M = n_seq * 32
    y = rng.random((M, 9)) < np.array(HIT_RATES)[None, :]
    logit = rng.normal(-2.0, 1.5, (M, 9)) + 3.0 * y * rng.random((M, 9))
    p = (1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    p[:, 0] = np.round(p[:, 0] * 16) / 16
    p[3, 1], p[7, 1], p[11, 1] = np.nan, 0.0, 1.0
    gt = np.zeros((M, 27), np.float32)
    gt[:, :9] = y
    gt[:, 9:18] = rng.random((M, 9)) * y
    gt[:, 18:] = (rng.random((M, 9)) - 0.5) * y
    p.setflags(write=False)
    gt.setflags(write=False)
    return p, gt


def hit_curve(lib, Buf, prob, gt, grid, stride=9, counts=None, stream=None):
    """gt_hit_curve on fresh device copies -> the (9, 2, K + 1) counts as int64 (counts: the buffer's contents before the call)"""
    prob = np.asarray(prob, np.float32).reshape(-1, 9)
    M, nb = prob.shape[0], len(grid) + 1
    if stride == 27:                                                # the hit columns of an HVO buffer
        hvo = np.full((M, 27), 7.5, np.float32)
        hvo[:, :9] = prob
        prob = hvo
    pb, gb = Buf(np.array(prob, np.float32)), Buf(np.array(gt, np.float32).reshape(M, 27))      # (copies: the shared inputs are read-only)
    cb = Buf(np.zeros(18 * nb, np.int64) if counts is None else np.asarray(counts, np.int64).reshape(-1).copy())
    words = int(lib.cdll.gt_hit_curve_scratch_words(ctypes.c_int64(M), len(grid)))
    assert 0 < words <= 256 * 18 * nb
    sb = Buf(np.full(words, 0x5EADBEEF, np.int32))                  # no precondition on scratch: garbage
    lib.call("gt_hit_curve", pb.ptr, stride, gb.ptr, ctypes.c_int64(M), (ctypes.c_float * len(grid))(*grid), len(grid), cb.ptr, sb.ptr,
             stream or ctypes.c_void_p(0))
    return cb.numpy().reshape(9, 2, nb).copy()


# ---- 1. the curve against numpy ----------------------------------------------------------------------------------------------------------
def check_curve(lib, Buf, n_seq, stride, n_thres):
    p, gt = inputs(n_seq)
    grid = grid_of(n_thres)
    got = hit_curve(lib, Buf, p, gt, grid, stride)
    want = href.curve(p, gt, grid)
    assert np.array_equal(got, want)
    assert int(got.sum()) == n_seq * 32 * 9
    assert got[8, 1].sum() == 0 and got[1, :, 0].sum() >= 2         # voice 8 is never hit; the NaN and the 0.0 sit in bin 0
    return got


@pytest.mark.parametrize("n_thres", [1, 9, 99, 127])
@pytest.mark.parametrize("stride", [9, 27])
@pytest.mark.parametrize("n_seq", [1, 3, 67])
def test_curve_against_numpy(n_seq, stride, n_thres):
    check_curve(emu_lib(), NpBuf, n_seq, stride, n_thres)


# ---- 2. accumulation ---------------------------------------------------------------------------------------------------------------------
def check_accumulate(lib, Buf):
    p, gt = inputs(67)
    grid = grid_of(99)
    whole = hit_curve(lib, Buf, p, gt, grid)
    first = hit_curve(lib, Buf, p[:40 * 32], gt[:40 * 32], grid)
    both = hit_curve(lib, Buf, p[40 * 32:], gt[40 * 32:], grid, counts=first)
    assert np.array_equal(both, whole)
    swapped = hit_curve(lib, Buf, p[:40 * 32], gt[:40 * 32], grid, counts=hit_curve(lib, Buf, p[40 * 32:], gt[40 * 32:], grid))
    assert np.array_equal(swapped, whole)
    # 64-bit words, added to, not stored
    pre = hit_curve(lib, Buf, p, gt, grid, counts=np.full(18 * 100, SENTINEL64, np.int64))
    assert np.array_equal(pre, whole + SENTINEL64)


def test_accumulation():
    check_accumulate(emu_lib(), NpBuf)


# ---- 3. one bin takes everything ---------------------------------------------------------------------------------------------------------
ONE_BIN = {"below_all": (0.005, 0), "above_all": (0.995, 99), "on_a_grid_value": (float(np.float32(50) / np.float32(100)), 49)}


def check_one_bin(lib, Buf, case):
    value, bin_ = ONE_BIN[case]
    _, gt = inputs(67)
    grid = grid_of(99)
    p = np.full((67 * 32, 9), value, np.float32)
    got = hit_curve(lib, Buf, p, gt, grid)
    assert np.array_equal(got, href.curve(p, gt, grid))
    assert int(got[:, :, bin_].sum()) == 67 * 32 * 9                # strict comparison: p == thres[49] is not above it


@pytest.mark.parametrize("case", list(ONE_BIN))
def test_one_bin(case):
    check_one_bin(emu_lib(), NpBuf, case)


# ---- 4. rejections -----------------------------------------------------------------------------------------------------------------------
def _grid_with(k, v):
    g = grid_of(9).copy()
    g[k] = v
    return g


CURVE_REJECTED = {
    "prob_null": dict(null="prob"), "gt_null": dict(null="gt"), "thres_null": dict(null="thres"), "counts_null": dict(null="counts"),
    "scratch_null": dict(null="scratch"), "rows_0": dict(n_rows=0), "rows_negative": dict(n_rows=-32), "rows_2_31": dict(n_rows=1 << 31),
    "n_thres_0": dict(n_thres=0), "n_thres_128": dict(grid=np.linspace(0.001, 0.999, 128).astype(np.float32)), "stride_10": dict(stride=10),
    "stride_0": dict(stride=0), "thres_nan": dict(grid=_grid_with(4, np.nan)), "thres_below_0": dict(grid=_grid_with(0, -0.01)),
    "thres_above_1": dict(grid=_grid_with(8, 1.5)), "thres_equal": dict(grid=_grid_with(3, grid_of(9)[2])),
    "thres_descending": dict(grid=grid_of(9)[::-1].copy()),
}


def check_curve_rejected(lib, Buf, case):
    kw = CURVE_REJECTED[case]
    p, gt = inputs(1)
    grid = kw.get("grid", grid_of(9))
    n_thres = kw.get("n_thres", len(grid))
    pb, gb = Buf(p.copy()), Buf(gt.copy())
    cb, sb = Buf(np.full(18 * 129, SENTINEL64, np.int64)), Buf(np.zeros(18 * 129, np.int32))
    ptr = lambda name, b: None if kw.get("null") == name else b.ptr
    rc = lib.cdll.gt_hit_curve(ptr("prob", pb), kw.get("stride", 9), ptr("gt", gb), ctypes.c_int64(kw.get("n_rows", 32)),
                               None if kw.get("null") == "thres" else (ctypes.c_float * len(grid))(*grid), n_thres, ptr("counts", cb),
                               ptr("scratch", sb), ctypes.c_void_p(0))
    assert rc < 0 and b"gt_hit_curve" in lib.cdll.gt_last_error()
    assert (cb.numpy() == SENTINEL64).all()


@pytest.mark.parametrize("case", list(CURVE_REJECTED))
def test_curve_rejected_before_any_launch(case):
    check_curve_rejected(emu_lib(), NpBuf, case)


RULE_REJECTED = {
    "counts_null": dict(null="counts"), "thres_null": dict(null="thres"), "rule_null": dict(null="rule"), "thres_out_null": dict(null="thres_out"),
    "index_out_null": dict(null="index_out"), "scores_out_null": dict(null="scores_out"), "n_thres_0": dict(n_thres=0),
    "n_thres_128": dict(grid=np.linspace(0.001, 0.999, 128).astype(np.float32)), "thres_nan": dict(grid=_grid_with(4, np.nan)),
    "thres_above_1": dict(grid=_grid_with(8, 1.5)), "thres_equal": dict(grid=_grid_with(3, grid_of(9)[2])),
    "criterion_2": dict(rule=(2, 1.0, 0.5)), "criterion_negative": dict(rule=(-1, 1.0, 0.5)), "beta_0": dict(rule=(0, 0.0, 0.5)),
    "beta_negative": dict(rule=(0, -1.0, 0.5)), "beta_inf": dict(rule=(0, float("inf"), 0.5)), "beta_nan": dict(rule=(0, float("nan"), 0.5)),
    "fallback_negative": dict(rule=(1, 1.0, -0.1)), "fallback_above_1": dict(rule=(0, 1.0, 1.5)), "fallback_nan": dict(rule=(1, 1.0, float("nan"))),
}


@pytest.mark.parametrize("case", list(RULE_REJECTED))
def test_thresholds_rejected(case):
    lib = emu_lib()
    kw = RULE_REJECTED[case]
    grid = kw.get("grid", grid_of(9))
    cnt = (ctypes.c_uint64 * (18 * 129))(*([3] * (18 * 129)))
    rule = _lib.GtThresholdRule(*kw.get("rule", (0, 1.0, 0.5)))
    th, idx, sc = (ctypes.c_float * 9)(*([7.5] * 9)), (ctypes.c_int32 * 9)(*([77] * 9)), (ctypes.c_float * 36)(*([7.5] * 36))
    arg = lambda name, v: None if kw.get("null") == name else v
    rc = lib.cdll.gt_hit_thresholds(arg("counts", cnt), arg("thres", (ctypes.c_float * len(grid))(*grid)), kw.get("n_thres", len(grid)),
                                    arg("rule", ctypes.byref(rule)), arg("thres_out", th), arg("index_out", idx), arg("scores_out", sc))
    assert rc < 0 and b"gt_hit_thresholds" in lib.cdll.gt_last_error()
    assert list(th) == [7.5] * 9 and list(idx) == [77] * 9 and list(sc) == [7.5] * 36


def test_density_does_not_look_at_beta():
    """beta is checked under criterion 0 only"""
    th, idx, sc = emu_lib().hit_thresholds(href.curve(*inputs(67), grid_of(99)), grid_of(99), 1, float("nan"), 0.5)
    assert idx[0] >= 0 and idx[8] == -1 and all(s[2] == 0.0 for s in sc)


# ---- 5. the choice against numpy ---------------------------------------------------------------------------------------------------------
def check_selection(lib, counts, criterion, beta):
    grid = grid_of(99)
    th, idx, sc = lib.hit_thresholds(counts, grid, criterion, beta, 0.375)
    wth, widx, wsc, cands = href.select(counts, grid, criterion, beta, 0.375)
    if criterion == 0:                                              # the condition under which a last-bit difference cannot move a choice
        gaps = href.fbeta_gaps(counts, beta)
        print("smallest gap between the best and the second-best distinct F-beta: %g" % min(gaps + [np.inf]))
        assert all(g > GAP_MIN for g in gaps)
    assert idx == [int(i) for i in widx]
    assert np.array_equal(np.array(th, np.float32).view(np.uint32), wth.view(np.uint32))
    assert np.abs(np.array(sc, np.float64) - wsc).max() <= 1e-6
    return idx, cands


@pytest.mark.parametrize("beta", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("criterion", [0, 1])
@pytest.mark.parametrize("n_seq", [1, 3, 67])
def test_selection_against_numpy(n_seq, criterion, beta):
    lib = emu_lib()
    counts = check_curve(lib, NpBuf, n_seq, 9, 99)
    idx, cands = check_selection(lib, counts, criterion, beta)
    assert idx[8] == -1                                             # the voice without a true hit takes the fallback
    if n_seq == 67:
        assert max(len(c) for c in cands) >= 6                      # a plateau: the lower-median rule decides
        assert all(i >= 0 for i in idx[:3])


# ---- 6. end to end: the device's own probabilities, against the fp64 oracle -------------------------------------------------------------------
def _gt_of(shape):
    cfg, _, _ = _inputs(_key(shape))
    return ng.synthetic_batch(shape[1], cfg["embedding_size_src"], seed=8)[1].reshape(-1, 27).astype(np.float32)


def _curve_on_device(r, prob_buf, stride, gt, grid):
    nb = len(grid) + 1
    gb, cb = r.Buf(gt), r.Buf(np.zeros(18 * nb, np.int64))
    sb = r.Buf(np.zeros(int(r.lib.cdll.gt_hit_curve_scratch_words(ctypes.c_int64(r.M), len(grid))), np.int32))
    r.lib.call("gt_hit_curve", prob_buf.ptr, stride, gb.ptr, ctypes.c_int64(r.M), (ctypes.c_float * len(grid))(*grid), len(grid), cb.ptr, sb.ptr,
               r.stream)
    return cb.numpy().reshape(9, 2, nb).copy()


def _predict_voices(r, x, vs):
    r.x = r.Buf(np.asarray(x, np.float32).reshape(r.M, -1))
    prob = r.Buf(np.full((r.M, 9), 7.5, np.float32))
    r.lib.call("gt_predict_voices", ctypes.byref(r.c), r.params.ptr, r.pe.ptr, r.x.ptr, r.hvo.ptr, ctypes.byref(vs), ctypes.c_uint32(0),
               ctypes.c_int64(0), prob.ptr, r.tgt.ptr, r.ws.ptr, r.stream)
    return prob


def check_end_to_end_encoder(backend, shape):
    r = runner(backend, shape)
    _, _, x = _inputs(_key(shape))
    gt, grid = _gt_of(shape), grid_of(9)
    # the two sources of probabilities: gt_predict(use_thres = 0) into an HVO buffer, gt_predict_voices' prob_out
    hvo = r.predict(x, use_thres=False).reshape(-1, 27)
    c27 = _curve_on_device(r, r.hvo, 27, gt, grid)
    assert np.array_equal(c27, href.curve(hvo[:, :9], gt, grid))                  # (a)
    prob = _predict_voices(r, x, _lib.make_voice_sampling(THRES))
    c9 = _curve_on_device(r, prob, 9, gt, grid)
    assert np.array_equal(c9, href.curve(prob.numpy(), gt, grid)) and np.array_equal(c9, c27)
    # (b) against the oracle's probabilities: cumulative counts differ by at most the oracle's elements inside the margin of that threshold
    pref = oracle(_key(shape), 1.0)[2].reshape(-1, 9)
    near = np.abs(pref[..., None] - grid.astype(np.float64)) <= MARGIN_TOL        # (M, 9, K)
    print("oracle probabilities within %g of a grid value: %d of %d" % (MARGIN_TOL, int(near.any(-1).sum()), near[..., 0].size))
    assert near.any(-1).mean() < 0.01
    g = gt[:, :9] == 1
    dev_tp, dev_fp, _ = href.rates(c27)
    ora_tp, ora_fp, _ = href.rates(href.curve(pref.astype(np.float32), gt, grid))
    slack_tp, slack_fp = (near & g[..., None]).sum(0), (near & ~g[..., None]).sum(0)      # (9, K)
    assert (np.abs(dev_tp - ora_tp) <= slack_tp).all() and (np.abs(dev_fp - ora_fp) <= slack_fp).all()
    assert dev_tp.sum() > 0 and dev_fp.sum() > 0


def check_end_to_end_decoder(backend, shape):
    r = runner(backend, shape)
    _, _, x = _inputs(_key(shape))
    gt, grid = _gt_of(shape), grid_of(9)
    prob = _predict_voices(r, x, _lib.make_voice_sampling(THRES))
    c9 = _curve_on_device(r, prob, 9, gt, grid)
    p = prob.numpy()
    assert (p != 7.5).all() and np.array_equal(c9, href.curve(p, gt, grid)) and int(c9.sum()) == r.M * 9


def test_end_to_end_encoder_only():
    check_end_to_end_encoder("emu", ENC)


def test_end_to_end_encoder_decoder():
    check_end_to_end_decoder("emu", ENCDEC)


# ---- the host mirror on the emulator: engine.hit_curve -------------------------------------------------------------------------------------
def test_struct_matches_header():
    assert ctypes.sizeof(_lib.GtThresholdRule) == 12
    assert [f[0] for f in _lib.GtThresholdRule._fields_] == ["criterion", "beta", "fallback"]
    assert _lib.CURVE_MAX_THRES == 127


def test_engine_hit_curve_on_the_emulator():
    import torch
    from transformergrooveinfilling_amd.engine import StepEngine
    cfg, P, x = _inputs(_key(ENC))
    r = runner("emu", ENC)
    eng = StepEngine(batch_size=4, optimizer="sgd", learning_rate=0.05, hit_loss_penalty=0.47, seed=3, device="cpu", lib=r.lib,
                     **{k: cfg[k] for k in ("d_model", "n_heads", "dim_feedforward", "num_encoder_layers", "num_decoder_layers", "dropout",
                                            "embedding_size_src")})
    eng.load_named(P)
    xt, gt = torch.from_numpy(x), torch.from_numpy(_gt_of(ENC).reshape(4, 32, 27))
    calls = []
    call = r.lib.call
    try:
        r.lib.call = lambda name, *a: (calls.append(name), call(name, *a))[1]
        one = eng.hit_curve(xt, gt).numpy().copy()
        assert "gt_predict" in calls and "gt_predict_voices" not in calls       # encoder-only at temperature 1: the HVO buffer's hit columns
        two = eng.hit_curve(xt, gt, chunk=3).numpy().copy()                     # 3 + 1
        del calls[:]
        warm = eng.hit_curve(xt, gt, grid=grid_of(9), temperature=0.5, voice_thresholds=THRES).numpy().copy()
        assert "gt_predict_voices" in calls
    finally:
        r.lib.call = call
    probs = eng.predict(xt, use_thres=False).numpy()[..., :9]
    assert one.shape == (9, 2, 100) and one.dtype == np.int64
    assert np.array_equal(one, href.curve(probs, gt.numpy(), grid_of(99))) and np.array_equal(two, one)
    assert int(warm.sum()) == 4 * 32 * 9 and not np.array_equal(warm, href.curve(probs, gt.numpy(), grid_of(9)))
    # counts= continues an accumulation: two halves of the set add up to the whole
    half = eng.hit_curve(xt[:2], gt[:2])
    assert eng.hit_curve(xt[2:], gt[2:], counts=half) is half and np.array_equal(half.numpy(), one)
    # "calibrated" thresholds: refused while there are none, then what was stored
    with pytest.raises(ValueError):
        eng.predict(xt, voice_thresholds="calibrated")
    eng.voice_thresholds = list(THRES)
    assert np.array_equal(eng.predict(xt, voice_thresholds="calibrated").numpy(), eng.predict(xt, voice_thresholds=THRES).numpy())
    for bad in (dict(grid=[0.5, 0.5]), dict(grid=[]), dict(grid=[0.2, 1.5]), dict(counts=torch.zeros(9, 2, 5, dtype=torch.int64))):
        with pytest.raises(ValueError):
            eng.hit_curve(xt, gt, **bad)
