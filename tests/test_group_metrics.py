"""Per-group and removed-cell evaluation counts (gt_group_metrics; include/groove_hip.h) without a GPU: the counting pass against its numpy
restatement (tests/group_metrics_ref.py) on constructed inputs -- every integer equal --, accumulation over calls, garbage in scratch, the
all-zero mask, the cross-check with gt_voice_metrics, the argument checks, and the Python front (metrics.group_metrics, rank_sequences,
the cells / removed conversions).  The kernels run in the host-emulator build of the same sources; tests/test_group_metrics_gpu.py repeats
the checks on the GPU."""
import ctypes
import functools

import numpy as np
import pytest

import group_metrics_ref as gref
from harness import NpBuf, emu_lib
from test_hit_curve import HIT_RATES, SENTINEL64
from transformergrooveinfilling_amd import _lib, metrics

SCRATCH_GARBAGE = 0x5EADBEEF
SEQ_SENTINEL = 0x7EADBEE5


@functools.lru_cache(maxsize=None)
def inputs(n_seq):
    """(hvo_pred, hvo_gt), both (n_seq * 32, 27) fp32: hit rates per voice as test_hit_curve's (voice 8 never hit), predicted hits that lean
    towards the truth, velocities in (0,1), offsets in (-0.5,0.5) on both sides; in sequence 0: one NaN and one 5.0 in a velocity column,
    one +inf in an offset column, one NaN and one 0.5 in a hit column"""
    rng = np.random.default_rng(7000 + n_seq)
    M = n_seq * 32
    y = rng.random((M, 9)) < np.array(HIT_RATES)[None, :]
    ph = np.where(y, rng.random((M, 9)) < 0.7, rng.random((M, 9)) < np.array(HIT_RATES)[None, :] * 0.5)
    gt, pred = np.zeros((M, 27), np.float32), np.zeros((M, 27), np.float32)
    gt[:, :9], pred[:, :9] = y, ph
    gt[:, 9:18] = rng.random((M, 9)) * y
    gt[:, 18:] = (rng.random((M, 9)) - 0.5) * y
    pred[:, 9:18] = rng.random((M, 9))
    pred[:, 18:] = rng.random((M, 9)) - 0.5
    pred[1, 9 + 0], pred[2, 9 + 1], pred[3, 18 + 2] = np.nan, 5.0, np.inf
    pred[4, 0], pred[5, 1] = np.nan, 0.5
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


@functools.lru_cache(maxsize=None)
def tags(n_seq, n_groups):
    """group ids from -1..n_groups (both ends are skipped sequences); group 1 (where there is one) stays empty and group 0 takes more
    than half of the sequences"""
    rng = np.random.default_rng(7100 + 64 * n_seq + n_groups)
    g = rng.integers(-1, n_groups + 1, n_seq).astype(np.int32)
    g[g == 1] = 0
    g[rng.random(n_seq) < 0.7] = 0
    if n_seq > 1:
        g[0], g[1] = 0, -1                                          # sequence 0 carries the planted values; at least one is skipped
    g.setflags(write=False)
    return g


MASKS = ("null", "random", "zeros", "ones", "bit0", "bit31")


def mask_of(kind, n_seq):
    if kind == "null":
        return None
    if kind == "random":
        return np.random.default_rng(7200 + n_seq).integers(0, 1 << 32, (n_seq, 9), dtype=np.uint64).astype(np.uint32)
    return np.full((n_seq, 9), {"zeros": 0, "ones": 0xFFFFFFFF, "bit0": 1, "bit31": 1 << 31}[kind], np.uint32)


def scratch_words(lib, n_seq, n_groups):
    words = int(lib.cdll.gt_group_metrics_scratch_words(ctypes.c_int64(n_seq), n_groups))
    assert 0 < words <= 2048 * gref.acc_words(n_groups)
    return words


def group_metrics(lib, Buf, pred, gt, group=None, cells=None, n_groups=1, acc=None, seq_out=True, scratch_fill=SCRATCH_GARBAGE, stream=None,
                  keep=None):
    """gt_group_metrics on fresh device copies -> (acc as int64, seq_out (n_seq, 4) as int64 or None); acc: the buffer's contents before
    the call; scratch holds garbage; keep: a list that receives the call's buffers (a guarded class is checked after the call)"""
    pred = np.array(pred, np.float32).reshape(-1, 27)
    n_seq = pred.shape[0] // 32
    pb, gb = Buf(pred), Buf(np.array(gt, np.float32).reshape(-1, 27))                     # (copies: the shared inputs are read-only)
    grp = None if group is None else Buf(np.array(group, np.int32))
    cb = None if cells is None else Buf(np.array(cells, np.uint32).view(np.int32))
    ab = Buf(np.zeros(gref.acc_words(n_groups), np.int64) if acc is None else np.asarray(acc, np.int64).reshape(-1).copy())
    qb = Buf(np.full((n_seq, 4), SEQ_SENTINEL, np.int32)) if seq_out else None
    sb = Buf(np.full(2 * scratch_words(lib, n_seq, n_groups), scratch_fill, np.uint32).view(np.int32))
    lib.call("gt_group_metrics", pb.ptr, gb.ptr, grp.ptr if grp else None, cb.ptr if cb else None, ctypes.c_int64(n_seq), n_groups, ab.ptr,
             qb.ptr if qb else None, sb.ptr, stream or ctypes.c_void_p(0))
    if keep is not None:
        keep.extend(b for b in (pb, gb, grp, cb, ab, qb, sb) if b is not None)
    return ab.numpy().astype(np.int64).copy(), (qb.numpy().astype(np.int64).copy() if qb else None)


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------------
def check_against_ref(lib, Buf, n_seq, n_groups, mask, seq_out=True):
    pred, gt = inputs(n_seq)
    group, cells = tags(n_seq, n_groups), mask_of(mask, n_seq)
    got, seq = group_metrics(lib, Buf, pred, gt, group, cells, n_groups, seq_out=seq_out)
    want, want_seq = gref.group_metrics(pred, gt, group, cells, n_groups)
    assert np.array_equal(got, want)
    if seq_out:
        assert np.array_equal(seq, want_seq)                        # written for every sequence, the skipped ones included
    words, seqs, rej, skipped = gref.split(got, n_groups)
    assert int(seqs.sum()) + skipped == n_seq
    if n_groups > 1:
        assert seqs[1] == 0 and not words[1].any()                  # the empty group
    if n_seq >= 67:
        assert 2 * seqs[0] > n_seq                                  # one group takes more than half
    if n_seq == 67 and mask == "null":                              # the case is not vacuous
        w = words.sum(0)                                            # (9, 8) over the groups
        assert int(((w[:, 1] > 0) & (w[:, 2] > 0) & (w[:, 3] > 0)).sum()) >= 8
        assert skipped >= 1 and int(w[:, 4:].max()) > 1 << 32
        assert (w[:8, 6:8] != 0).all() and (w[:8, 6:8] != w[:8, 4:6]).all()
        assert int(rej.sum()) >= 3                                  # (sequence 0 carries the planted values)
    return got, seq


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("n_groups", [1, 5, 64])
@pytest.mark.parametrize("n_seq", [1, 3, 67, 1024])
def test_against_the_restatement(n_seq, n_groups, mask):
    """1: one sequence; 3: fewer sequences than a workgroup's share; 67: a ragged tail; 1024: every workgroup walks several sequences
    (grid-stride) and the second kernel adds many partials"""
    check_against_ref(emu_lib(), NpBuf, n_seq, n_groups, mask)


@pytest.mark.parametrize("n_groups,mask", [(1, "null"), (5, "random")])
def test_without_seq_out(n_groups, mask):
    check_against_ref(emu_lib(), NpBuf, 67, n_groups, mask, seq_out=False)


def test_rejected_values_are_counted():
    """the planted NaN, 5.0 and +inf sit in sequence 0: exactly three rejected values without a mask, whatever group takes them"""
    pred, gt = inputs(67)
    got, _ = group_metrics(emu_lib(), NpBuf, pred, gt, None, None, 1)
    words, seqs, rej, skipped = gref.split(got, 1)
    assert int(rej[0]) == 3 and skipped == 0 and int(seqs[0]) == 67 and (words[0, :, 0] == 67 * 32).all()


# ---- 2. accumulation ---------------------------------------------------------------------------------------------------------------------
def check_accumulate(lib, Buf, n_groups=5):
    pred, gt = inputs(67)
    group, cells = tags(67, n_groups), mask_of("random", 67)
    cut = 40
    a, b = slice(0, cut * 32), slice(cut * 32, None)
    whole, _ = group_metrics(lib, Buf, pred, gt, group, cells, n_groups)
    first, _ = group_metrics(lib, Buf, pred[a], gt[a], group[:cut], cells[:cut], n_groups)
    both, _ = group_metrics(lib, Buf, pred[b], gt[b], group[cut:], cells[cut:], n_groups, acc=first)
    assert np.array_equal(both, whole)
    second, _ = group_metrics(lib, Buf, pred[b], gt[b], group[cut:], cells[cut:], n_groups)
    swapped, _ = group_metrics(lib, Buf, pred[a], gt[a], group[:cut], cells[:cut], n_groups, acc=second)
    assert np.array_equal(swapped, whole)
    # 64-bit words, added to, not stored
    pre, _ = group_metrics(lib, Buf, pred, gt, group, cells, n_groups, acc=np.full(gref.acc_words(n_groups), SENTINEL64, np.int64))
    assert np.array_equal(pre, whole + SENTINEL64)


def test_accumulation():
    check_accumulate(emu_lib(), NpBuf)


# ---- 3. scratch has no precondition ------------------------------------------------------------------------------------------------------
def check_scratch(lib, Buf, n_groups=5):
    pred, gt = inputs(67)
    group = tags(67, n_groups)
    one = group_metrics(lib, Buf, pred, gt, group, None, n_groups, scratch_fill=SCRATCH_GARBAGE)
    two = group_metrics(lib, Buf, pred, gt, group, None, n_groups, scratch_fill=0)
    three = group_metrics(lib, Buf, pred, gt, group, None, n_groups, scratch_fill=0xFFFFFFFF)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1])
    assert np.array_equal(one[0], gref.group_metrics(pred, gt, group, None, n_groups)[0])


def test_scratch_garbage():
    check_scratch(emu_lib(), NpBuf)


# ---- 4. the all-zero mask ----------------------------------------------------------------------------------------------------------------
def check_zero_mask(lib, Buf, n_groups=5):
    pred, gt = inputs(67)
    group = tags(67, n_groups)
    got, seq = group_metrics(lib, Buf, pred, gt, group, mask_of("zeros", 67), n_groups)
    words, seqs, rej, skipped = gref.split(got, n_groups)
    assert not words.any() and not rej.any() and not seq.any()
    assert int(seqs.sum()) + skipped == 67 and int(seqs.sum()) > 0 and skipped > 0


def test_all_zero_mask():
    check_zero_mask(emu_lib(), NpBuf)


# ---- 5. cross-check with gt_voice_metrics --------------------------------------------------------------------------------------------------
def check_voice_metrics_agree(lib, Buf, n_seq=67):
    pred, gt = (np.array(a) for a in inputs(n_seq))
    pred[:, :9] = pred[:, :9] == 1                                  # 0 / 1 hit columns: equality of the hits is what both passes count
    pred[:, 9:] = np.where(np.isfinite(pred[:, 9:]) & (np.abs(pred[:, 9:]) < 2), pred[:, 9:], 0.25)
    got, _ = group_metrics(lib, Buf, pred, gt)
    w = gref.split(got, 1)[0][0].astype(np.float64)                 # (9, 8)
    M = n_seq * 32
    pb, gb, ob = Buf(pred), Buf(gt), Buf(np.zeros(30, np.float32))
    sb = Buf(np.zeros(int(lib.cdll.gt_voice_metrics_scratch_floats(ctypes.c_int64(M))), np.float32))
    lib.call("gt_voice_metrics", pb.ptr, gb.ptr, ctypes.c_int64(M), ob.ptr, sb.ptr, ctypes.c_void_p(0))
    out30 = ob.numpy().astype(np.float64)
    assert np.abs((w[:, 0] - w[:, 2] - w[:, 3]) / w[:, 0] - out30[1:10]).max() <= 1e-6
    for k, base in ((4, 11), (5, 21)):                              # out30 is an fp32 sum: the bound is about its rounding
        mse = w[:, k] / 4294967296.0 / w[:, 0]
        assert (mse > 0).all() and (np.abs(mse - out30[base:base + 9]) <= 1e-5 * mse).all()


def test_agrees_with_voice_metrics():
    check_voice_metrics_agree(emu_lib(), NpBuf)


# ---- 6. rejections -----------------------------------------------------------------------------------------------------------------------
REJECTED = {
    "pred_null": dict(null="pred"), "gt_null": dict(null="gt"), "acc_null": dict(null="acc"), "scratch_null": dict(null="scratch"),
    "n_seq_0": dict(n_seq=0), "n_seq_negative": dict(n_seq=-1), "n_seq_2_26": dict(n_seq=1 << 26), "n_groups_0": dict(n_groups=0),
    "n_groups_negative": dict(n_groups=-3), "n_groups_65": dict(n_groups=65),
}


def check_rejected(lib, Buf, case):
    kw = REJECTED[case]
    pred, gt = inputs(1)
    pb, gb = Buf(pred.copy()), Buf(gt.copy())
    ab, qb = Buf(np.full(gref.acc_words(65), SENTINEL64, np.int64)), Buf(np.full((1, 4), SEQ_SENTINEL, np.int32))
    sb = Buf(np.zeros(gref.acc_words(65), np.int64))
    ptr = lambda name, b: None if kw.get("null") == name else b.ptr
    rc = lib.cdll.gt_group_metrics(ptr("pred", pb), ptr("gt", gb), None, None, ctypes.c_int64(kw.get("n_seq", 1)), kw.get("n_groups", 2),
                                   ptr("acc", ab), qb.ptr, ptr("scratch", sb), ctypes.c_void_p(0))
    assert rc < 0 and b"gt_group_metrics" in lib.cdll.gt_last_error()
    assert (ab.numpy() == SENTINEL64).all() and (qb.numpy() == SEQ_SENTINEL).all()
    if "null" not in kw:                                            # the size query refuses the same ranges
        assert lib.cdll.gt_group_metrics_scratch_words(ctypes.c_int64(kw.get("n_seq", 1)), kw.get("n_groups", 2)) == 0


@pytest.mark.parametrize("case", list(REJECTED))
def test_rejected_before_any_launch(case):
    check_rejected(emu_lib(), NpBuf, case)


# ---- train.py's tags (host side only) --------------------------------------------------------------------------------------------------------
def test_train_py_reads_the_tags(tmp_path):
    import train as train_cli
    x, y = train_cli.synthetic_tensors(12, 16, 3)
    tag = np.array([0, 2, 1, 1, 0, 2, 2, 0, 1, 0, 0, 3], np.int64)

    def load(**arrays):
        f = tmp_path / "eval.npz"
        np.savez(f, validation_inputs=x.numpy(), validation_gt=y.numpy(), **arrays)
        args = train_cli.build_parser().parse_args(["--experiment", "InfillingClosedHH", "--eval-npz", str(f), "--eval-size", "8"])
        info = {}
        sets = train_cli.load_eval_sets(args, x, y, 16, None, info)
        return sets, info

    sets, info = load(validation_groups=tag, group_names=np.array(["rock", "funk"]))
    assert sorted(sets) == ["Train_Set", "Validation_Set"] and sorted(info) == ["Validation_Set"]       # the untagged train subset has no entry
    v = info["Validation_Set"]
    assert v["n_groups"] == 4 and v["names"] == ["rock", "funk", "group2", "group3"] and v["groups"].tolist() == tag.tolist()
    assert load(validation_groups=tag)[1]["Validation_Set"]["names"] == ["group0", "group1", "group2", "group3"]
    assert load()[1] == {} and load(train_groups=tag)[1] == {}       # no tags; tags of a set that did not come from the file
    for bad in (np.arange(12) * 6, tag[:5], tag.astype(np.float32)):      # 67 groups; too few tags; not integers
        with pytest.raises(SystemExit, match="groups"):
            load(validation_groups=bad)


# ---- 7. the Python front -----------------------------------------------------------------------------------------------------------------
def test_constants_match_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "groove_hip.h")).read()
    assert int(re.search(r"#define GT_GM_MAX_GROUPS (\d+)", hdr).group(1)) == _lib.GM_MAX_GROUPS == 64
    assert int(re.search(r"#define GT_GM_WORDS (\d+)", hdr).group(1)) == _lib.GM_WORDS == gref.WORDS
    assert [_lib.gm_acc_words(k) for k in (1, 5, 64)] == [gref.acc_words(k) for k in (1, 5, 64)] == [75, 371, 4737]


def _known_acc():
    """two groups; group 0: KICK and SNARE counted; group 1: nothing but a sequence (every denominator zero)"""
    acc = np.zeros(gref.acc_words(2), np.int64)
    acc[0:8] = [100, 6, 2, 4, 3 << 32, 1 << 32, 3 << 31, 3 << 30]                 # KICK
    acc[8:16] = [60, 0, 0, 10, 6 << 32, 0, 0, 0]                                 # SNARE: no TP
    acc[144:148] = [5, 2, 1, 0]
    acc[148] = 7
    return acc


def test_metrics_from_a_known_acc():
    res = metrics.group_metrics_from_acc(_known_acc(), 2, names=["rock", "jazz"], beta=2.0)
    assert set(res) == {"Overall", "rock", "jazz", "Skipped_Sequences"} and res["Skipped_Sequences"] == 7.0
    keys = {"%s_%s" % (q, v) for q in metrics.GM_QUANTITIES for v in ("Overall",) + metrics.VOICES} | {"Sequences", "Cells", "Rejected_Values"}
    assert len(metrics.GM_QUANTITIES) == 8 and all(set(res[g]) == keys for g in ("Overall", "rock", "jazz"))
    r = res["rock"]
    assert (r["Sequences"], r["Cells"], r["Rejected_Values"]) == (5.0, 160.0, 2.0)
    assert r["Hits_Accuracy_KICK"] == 94 / 100 and r["Hits_Precision_KICK"] == 6 / 8 and r["Hits_Recall_KICK"] == 6 / 10
    assert r["Hits_F1_KICK"] == 5 * 6 / (5 * 6 + 4 * 4 + 2)                      # F-beta at beta 2
    assert r["Velocity_MSE_KICK"] == 3 / 100 and r["Offset_MSE_KICK"] == 1 / 100
    assert r["Velocity_MSE_Hits_KICK"] == 1.5 / 6 and r["Offset_MSE_Hits_KICK"] == 0.75 / 6
    assert r["Hits_Accuracy_SNARE"] == 50 / 60 and r["Hits_Precision_SNARE"] == 0.0 and r["Hits_Recall_SNARE"] == 0.0
    assert r["Hits_F1_SNARE"] == 0.0 and r["Velocity_MSE_Hits_SNARE"] == 0.0 and r["Velocity_MSE_SNARE"] == 6 / 60
    assert all(r["%s_RIDE" % q] == 0.0 for q in metrics.GM_QUANTITIES)           # no cells at all: every denominator zero
    # micro-average over the voices: the integers first
    assert r["Hits_Accuracy_Overall"] == (160 - 2 - 14) / 160 and r["Hits_Recall_Overall"] == 6 / 20 and r["Velocity_MSE_Overall"] == 9 / 160
    assert r["Velocity_MSE_Hits_Overall"] == 1.5 / 6
    j = res["jazz"]
    assert j["Sequences"] == 1.0 and j["Cells"] == 0.0 and all(j["%s_Overall" % q] == 0.0 for q in metrics.GM_QUANTITIES)
    # Overall over the groups: the integer sum
    o = res["Overall"]
    assert (o["Sequences"], o["Cells"], o["Rejected_Values"]) == (6.0, 160.0, 2.0)
    assert all(o[k] == r[k] for k in keys - {"Sequences"})
    assert list(metrics.group_metrics_from_acc(_known_acc(), 2)) == ["Overall", "group0", "group1", "Skipped_Sequences"]
    for bad in (dict(acc=_known_acc()[:-1], n_groups=2), dict(acc=_known_acc(), n_groups=2, names=["a"]),
                dict(acc=_known_acc(), n_groups=2, names=["a", "a"]), dict(acc=_known_acc(), n_groups=2, names=["a", "Overall"])):
        with pytest.raises(ValueError):
            metrics.group_metrics_from_acc(**bad)


def test_rank_sequences():
    #        cells TP FP FN      F1
    sc = [[288, 4, 0, 0],      # 1.0
          [288, 0, 0, 0],      # 0 (zero denominator)
          [288, 2, 1, 1],      # 2/3
          [288, 4, 0, 0],      # 1.0 (a tie with 0)
          [288, 0, 3, 0],      # 0 (a tie with 1)
          [288, 1, 0, 2],      # 1/2
          [288, 9, 0, 0]]      # group 1
    res = metrics.rank_sequences(np.array(sc), groups=[0, 0, 0, 0, 0, 0, 1], k=3)
    assert res == {0: {"lowest": [1, 4, 5], "highest": [0, 3, 2]}, 1: {"lowest": [6], "highest": [6]}}
    assert metrics.rank_sequences(np.array(sc), k=2) == {0: {"lowest": [1, 4], "highest": [0, 3]}}
    assert metrics.rank_sequences(np.array(sc), groups=[-1, 0, 0, -1, 0, 0, -1], k=1) == {0: {"lowest": [1], "highest": [2]}}
    with pytest.raises(ValueError):
        metrics.rank_sequences(np.array(sc), groups=[0, 1])


@pytest.fixture(scope="module")
def engine():
    from test_predict_voices import ENC, _inputs, _key, runner
    from transformergrooveinfilling_amd.engine import StepEngine
    cfg, P, _ = _inputs(_key(ENC))
    eng = StepEngine(batch_size=4, optimizer="sgd", learning_rate=0.05, hit_loss_penalty=0.47, seed=3, device="cpu", lib=runner("emu", ENC).lib,
                     **{k: cfg[k] for k in ("d_model", "n_heads", "dim_feedforward", "num_encoder_layers", "num_decoder_layers", "dropout",
                                            "embedding_size_src")})
    eng.load_named(P)
    return eng


def test_engine_group_metrics_on_the_emulator(engine):
    import torch
    pred, gt = (torch.from_numpy(np.array(a)).reshape(-1, 32, 27) for a in inputs(67))
    group, words = np.array(tags(67, 5)), mask_of("random", 67)
    want, want_seq = gref.group_metrics(pred.numpy(), gt.numpy(), group, words, 5)
    acc, seq = engine.group_metrics(pred, gt, groups=torch.from_numpy(np.array(group)), n_groups=5,
                                    cells=torch.from_numpy(words.view(np.int32).copy()), seq_counts=True)
    assert acc.dtype == torch.int64 and tuple(acc.shape) == (371,) and np.array_equal(acc.numpy(), want)
    assert seq.dtype == torch.int32 and np.array_equal(seq.numpy(), want_seq)
    # a bool mask is the same mask; chunks and acc= continue the same words
    as_bool = torch.from_numpy(gref.cell_bits(words, 67))
    assert np.array_equal(engine.group_metrics(pred, gt, groups=group, n_groups=5, cells=as_bool, chunk=25).numpy(), want)
    half = engine.group_metrics(pred[:30], gt[:30], groups=group[:30], n_groups=5, cells=as_bool[:30])
    assert engine.group_metrics(pred[30:], gt[30:], groups=group[30:], n_groups=5, cells=as_bool[30:], acc=half) is half
    assert np.array_equal(half.numpy(), want)
    # removed: each removed voice is the all-ones word
    removed = np.random.default_rng(5).integers(0, 512, 67).astype(np.int32)
    voice_words = np.where((removed[:, None] >> np.arange(9)) & 1, 0xFFFFFFFF, 0).astype(np.uint32)
    assert np.array_equal(engine.group_metrics(pred, gt, removed=torch.from_numpy(removed)).numpy(),
                          gref.group_metrics(pred.numpy(), gt.numpy(), None, voice_words, 1)[0])
    # n_groups from the tags: the largest + 1 (tag 5 of tags(67, 5) becomes a group of its own; -1 stays skipped)
    auto = engine.group_metrics(pred, gt, groups=group)
    assert tuple(auto.shape) == (_lib.gm_acc_words(int(group.max()) + 1),)
    for bad in (dict(cells=as_bool, removed=removed), dict(n_groups=65), dict(n_groups=0), dict(groups=group[:5]), dict(removed=removed[:5]),
                dict(cells=as_bool[:5]), dict(acc=torch.zeros(7, dtype=torch.int64))):
        with pytest.raises(ValueError):
            engine.group_metrics(pred, gt, **bad)


def test_metrics_group_metrics_on_the_emulator(engine):
    import torch

    class Model:
        pass
    model = Model()
    model.engine = engine
    pred, gt = (torch.from_numpy(np.array(a)).reshape(-1, 32, 27) for a in inputs(67))
    group = np.array(tags(67, 5))
    names = ["rock", "funk", "jazz", "latin", "soul"]
    res = metrics.group_metrics(model, pred, gt, groups=group, names=names)
    want = metrics.group_metrics_from_acc(gref.group_metrics(pred.numpy(), gt.numpy(), group, None, 5)[0], 5, names)
    assert res == want and list(res) == ["Overall"] + names + ["Skipped_Sequences"]
    assert res["funk"]["Sequences"] == 0.0 and res["Skipped_Sequences"] >= 1.0 and 0.0 < res["rock"]["Hits_F1_Overall"] < 1.0
    one = metrics.group_metrics(model, pred, gt)
    assert list(one) == ["Overall", "group0", "Skipped_Sequences"] and one["Overall"] == one["group0"] and one["group0"]["Sequences"] == 67.0
