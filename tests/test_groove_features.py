"""Groove descriptors and rhythmic distances per sequence (gt_groove_features; include/groove_hip.h) without a GPU: the pass against its
numpy restatement (tests/groove_features_ref.py) on constructed inputs -- every integer equal, reserved words included --, grooves with
closed forms, position independence, the argument checks, and the host derivations (metrics.groove_descriptors, groove_distances,
descriptor_table).  The kernel runs in the host-emulator build of the same sources; tests/test_groove_features_gpu.py repeats the checks on
the GPU."""
import ctypes
import functools

import numpy as np
import pytest

import groove_features_ref as fref
from harness import NpBuf, emu_lib
from test_group_metrics import engine, inputs as gm_inputs  # noqa: F401  (engine: the module's emulator-backed StepEngine fixture)
from test_hit_curve import SENTINEL64
from transformergrooveinfilling_amd import _lib, metrics

COMBOS = ("a", "ab", "ab_no_feat_b", "ab_no_pair")
FIX = 1 << 32


@functools.lru_cache(maxsize=None)
def inputs(n_seq):
    """(hvo_a, hvo_b) = test_group_metrics.inputs (prediction, ground truth) with values planted AT HITS of sequence 0 of buffer a: a NaN
    velocity (rejected), a 5.0 velocity (valid), a 17.0 velocity (rejected), a +inf offset (rejected); the NaN and the 0.5 in hit columns
    are that construction's own"""
    a, b = (np.array(x) for x in gm_inputs(n_seq))
    for row, c, col, val in ((6, 0, 9, np.nan), (7, 1, 10, 5.0), (8, 2, 11, 17.0), (9, 0, 18, np.inf)):
        a[row, c], a[row, col] = 1.0, val
    assert np.isnan(a[4, 0]) and a[5, 1] == 0.5
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def groove_features(lib, Buf, a, b=None, feat_b=True, pair=True, fill=SENTINEL64, keep=None, n_seq=None, stream=None):
    """gt_groove_features on fresh device copies, the outputs pre-filled with `fill` -> (feat_a, feat_b or None, pair or None) as int64;
    keep: a list that receives the call's buffers (a guarded class is checked after the call)"""
    a = np.array(a, np.float32).reshape(-1, 27)
    n = a.shape[0] // 32 if n_seq is None else n_seq
    ab = Buf(a)
    bb = None if b is None else Buf(np.array(b, np.float32).reshape(-1, 27))
    fa = Buf(np.full((n, 32), fill, np.int64))
    fb = Buf(np.full((n, 32), fill, np.int64)) if (b is not None and feat_b) else None
    pw = Buf(np.full((n, 8), fill, np.int64)) if (b is not None and pair) else None
    lib.call("gt_groove_features", ab.ptr, bb.ptr if bb else None, ctypes.c_int64(n), fa.ptr, fb.ptr if fb else None, pw.ptr if pw else None,
             stream or ctypes.c_void_p(0))
    if keep is not None:
        keep.extend(x for x in (ab, bb, fa, fb, pw) if x is not None)
    return tuple(None if x is None else x.numpy().astype(np.int64).copy() for x in (fa, fb, pw))


def run_combo(lib, Buf, a, b, combo, **kw):
    if combo == "a":
        return groove_features(lib, Buf, a, **kw)
    return groove_features(lib, Buf, a, b, feat_b=combo != "ab_no_feat_b", pair=combo != "ab_no_pair", **kw)


@functools.lru_cache(maxsize=None)
def reference(n_seq):
    out = fref.groove_features(*inputs(n_seq))
    for x in out:
        x.setflags(write=False)
    return out


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------------
def check_against_ref(lib, Buf, n_seq, combo):
    a, b = inputs(n_seq)
    want_a, want_b, want_p = reference(n_seq)
    fa, fb, pw = run_combo(lib, Buf, a, b, combo)
    assert np.array_equal(fa, want_a)                               # every word, the reserved word 14 included (the sentinel is gone)
    assert (fb is None) == (combo in ("a", "ab_no_feat_b")) and (pw is None) == (combo in ("a", "ab_no_pair"))
    if fb is not None:
        assert np.array_equal(fb, want_b)
    if pw is not None:
        assert np.array_equal(pw, want_p)
    if n_seq == 67:                                                 # the case is not vacuous
        assert (want_a[:, 12] < 0).any() and (want_a[:, 12] > 0).any() and (want_b[:, 12] < 0).any() and (want_b[:, 12] > 0).any()
        assert (want_p[:, 2] > 0).any() and int(want_p[:, 2].sum()) > 67
        assert want_a[0, 7] == 2 and want_a[0, 8] == 1 and not want_a[1:, 7:9].any()       # the planted values, nothing else
        assert len(set(want_a[:, 1].tolist())) > 1 and len(set(want_b[:, 1].tolist())) > 1
        assert any(len(set(r[16:32].tolist())) == 16 for r in want_a)
        assert (want_p[:, 5] > 0).all() and (want_p[:, 4] > 0).all() and (want_a[:, 15:32] < 1 << 53).all()


@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("n_seq", [1, 3, 67, 1024])
def test_against_the_restatement(n_seq, combo):
    """1: one sequence; 3: fewer sequences than a workgroup's share; 67: a ragged tail; 1024: every workgroup walks several sequences"""
    check_against_ref(emu_lib(), NpBuf, n_seq, combo)


# ---- 2. constructed grooves with closed forms ----------------------------------------------------------------------------------------------
def groove(hits, v=1.0, o=0.0):
    """(32, 27): the cells (t, c) of `hits` hit at velocity v and offset o"""
    g = np.zeros((32, 27), np.float32)
    for t, c in hits:
        g[t, c], g[t, 9 + c], g[t, 18 + c] = 1.0, v, o
    return g


FOUR_ON_THE_FLOOR = [(t, 0) for t in range(0, 32, 4)]


def check_closed_forms(lib, Buf):
    empty = np.zeros((32, 27), np.float32)
    fa, fb, pw = groove_features(lib, Buf, empty, empty)
    assert not fa.any() and not fb.any() and not pw.any()
    # every cell a hit at v = 16, o = -16: the largest words there are
    full = groove([(t, c) for t in range(32) for c in range(9)], 16.0, -16.0)
    fa, _, pw = groove_features(lib, Buf, full, full)
    assert fa[0, :9].tolist() == [288, 9, 32, 72, 72, 144, 144, 0, 0]
    assert fa[0, 9:15].tolist() == [288 << 36, 288 << 40, 288 << 36, -(288 << 36), 288 << 40, 0]
    assert (fa[0, 15:] == 32 * (9 << 20) ** 2).all()
    assert pw[0].tolist() == [0, 288, 0, 0, 0, 288, 32 * (9 << 20) ** 2, 0]
    # a kick on every beat
    kick = groove(FOUR_ON_THE_FLOOR)
    fa, _, _ = groove_features(lib, Buf, kick)
    assert fa[0, :7].tolist() == [8, 1, 8, 8, 0, 0, 4] and fa[0, 7:15].tolist() == [0, 0, 8 * FIX, 8 * FIX, 0, 0, 0, 0]
    assert fa[0, 15:].tolist() == [8 * FIX if l % 4 == 0 else 0 for l in range(17)]
    # a groove against itself one step later, no hits colliding: every moved hit differs twice and is a near miss twice
    hits = FOUR_ON_THE_FLOOR + [(2, 2), (10, 2), (18, 2)]
    late = groove([(t + 1, c) for t, c in hits])
    fa, fb, pw = groove_features(lib, Buf, late, groove(hits))
    assert pw[0, :3].tolist() == [2 * len(hits), 0, 2 * len(hits)] and pw[0, 5] == 0 and fa[0, 0] == fb[0, 0] == len(hits)
    assert pw[0, 3] == 2 * len(hits) * FIX and pw[0, 6] == 0
    # ... and no wrap-around: a hit at step 31 is no neighbour of one at step 0
    _, _, pw = groove_features(lib, Buf, groove([(31, 0)]), groove([(0, 0)]))
    assert pw[0, :3].tolist() == [2, 0, 0]
    # a == b
    b = inputs(67)[1]
    fa, fb, pw = groove_features(lib, Buf, b, b)
    assert np.array_equal(fa, fb) and not pw[:, [0, 2, 3, 4, 7]].any()
    assert np.array_equal(pw[:, 6], fa[:, 15]) and np.array_equal(pw[:, 1], fa[:, 0]) and np.array_equal(pw[:, 5], fa[:, 0])


def test_closed_forms():
    check_closed_forms(emu_lib(), NpBuf)


def check_boundary_values(lib, Buf):
    g = np.zeros((32, 27), np.float32)
    above16 = np.nextafter(np.float32(16), np.float32(np.inf))
    denorm = -np.float32(1.401298464324817e-45)                     # the smallest negative denormal
    assert denorm < 0 and above16 > 16
    for t, (v, o) in enumerate([(-0.0, -0.0), (above16, 0.0), (denorm, 0.0), (0.0, 16.0), (0.0, -16.0)]):
        g[t, 3], g[t, 12], g[t, 21] = 1.0, v, o
    g[10, 0], g[11, 1], g[12, 2] = -1.0, 2.0, np.nan                # no hits, whatever their value columns hold
    g[10, 9], g[11, 10], g[12, 11], g[10, 18] = 3.0, np.nan, 99.0, np.inf
    fa, _, _ = groove_features(lib, Buf, g)
    assert np.array_equal(fa, fref.record(g))
    assert fa[0, :9].tolist() == [5, 1, 5, 2, 1, 2, 0, 2, 0]
    assert fa[0, 9:15].tolist() == [0, 0, 32 * FIX, 0, 512 * FIX, 0] and not fa[0, 15:].any()


def test_boundary_values():
    check_boundary_values(emu_lib(), NpBuf)


# ---- 3. position independence ----------------------------------------------------------------------------------------------------------------
def check_position_independence(lib, Buf):
    a, b = (x.reshape(67, 32, 27) for x in inputs(67))
    want = groove_features(lib, Buf, a, b)
    perm = np.random.default_rng(11).permutation(67)
    got = groove_features(lib, Buf, a[perm], b[perm])
    assert all(np.array_equal(g, w[perm]) for g, w in zip(got, want))
    for s in (0, 41, 66):
        alone = groove_features(lib, Buf, a[s], b[s])
        assert all(np.array_equal(g[0], w[s]) for g, w in zip(alone, want))


def test_position_independence():
    check_position_independence(emu_lib(), NpBuf)


# ---- 4. rejections ---------------------------------------------------------------------------------------------------------------------------
REJECTED = {
    "hvo_a_null": dict(null=("a",)), "feat_a_null": dict(null=("fa",)), "n_seq_0": dict(n_seq=0), "n_seq_negative": dict(n_seq=-1),
    "n_seq_2_26": dict(n_seq=1 << 26), "feat_b_without_hvo_b": dict(null=("b", "pw")), "pair_without_hvo_b": dict(null=("b", "fb")),
    "both_without_hvo_b": dict(null=("b",)),
}


def check_rejected(lib, Buf, case):
    kw = REJECTED[case]
    a, b = inputs(1)
    ab, bb = Buf(a.copy()), Buf(b.copy())
    fa, fb, pw = Buf(np.full((1, 32), SENTINEL64, np.int64)), Buf(np.full((1, 32), SENTINEL64, np.int64)), Buf(np.full((1, 8), SENTINEL64, np.int64))
    ptr = lambda name, buf: None if name in kw.get("null", ()) else buf.ptr
    rc = lib.cdll.gt_groove_features(ptr("a", ab), ptr("b", bb), ctypes.c_int64(kw.get("n_seq", 1)), ptr("fa", fa), ptr("fb", fb), ptr("pw", pw),
                                     ctypes.c_void_p(0))
    assert rc < 0 and b"gt_groove_features" in lib.cdll.gt_last_error()
    assert all((x.numpy() == SENTINEL64).all() for x in (fa, fb, pw))


@pytest.mark.parametrize("case", list(REJECTED))
def test_rejected_before_any_launch(case):
    check_rejected(emu_lib(), NpBuf, case)


def test_hvo_b_without_outputs_is_legal():
    """hvo_b with feat_b and pair both NULL: the record of a alone"""
    a, b = inputs(3)
    lib = emu_lib()
    ab, bb, fa = NpBuf(a.copy()), NpBuf(b.copy()), NpBuf(np.full((3, 32), SENTINEL64, np.int64))
    lib.call("gt_groove_features", ab.ptr, bb.ptr, ctypes.c_int64(3), fa.ptr, None, None, ctypes.c_void_p(0))
    assert np.array_equal(fa.numpy(), reference(3)[0])


# ---- 5. host derivations -----------------------------------------------------------------------------------------------------------------------
def test_constants_match_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "groove_hip.h")).read()
    assert int(re.search(r"#define GT_GF_WORDS (\d+)", hdr).group(1)) == _lib.GF_WORDS == fref.WORDS
    assert int(re.search(r"#define GT_GF_PAIR_WORDS (\d+)", hdr).group(1)) == _lib.GF_PAIR_WORDS == fref.PAIR_WORDS


def test_descriptors_of_closed_form_grooves():
    kick, empty = groove(FOUR_ON_THE_FLOOR, v=0.5, o=-0.25), np.zeros((32, 27), np.float32)
    d = metrics.groove_descriptors(fref.record(np.stack([kick, empty])))
    assert list(d) == list(metrics.DESCRIPTORS) and all(v.shape == (2,) and v.dtype == np.float64 for v in d.values())
    k = {name: v[0] for name, v in d.items()}
    assert k["Statistical::NoI"] == 1 and k["Statistical::Total Step Density"] == 0.25 and k["Statistical::Avg Voice Density"] == 0.25
    assert k["Statistical::Weak to Strong Ratio"] == 0 and k["Statistical::Symmetry"] == 1
    assert k["Auto-Correlation::Beat"] == k["Auto-Correlation::Bar"] == k["Auto-Correlation::Max"] == 1
    assert k["Statistical::Poly Velocity Mean"] == 0.5 and k["Statistical::Poly Velocity std"] == 0
    assert k["Statistical::Poly Offset Mean"] == -0.25 and k["Statistical::Poly Offset std"] == 0 and k["Micro-Timing::Accuracy"] == 0.25
    assert k["Auto-Correlation::Centroid"] == 10.0 and k["Auto-Correlation::Skewness"] == 0.0          # lags 4, 8, 12, 16 weigh the same
    assert all(v[1] == 0.0 for v in d.values())                     # the empty groove: every denominator zero
    # rejected values leave the denominators: one hit, its velocity invalid
    bad = groove([(0, 0)], v=17.0, o=0.125)
    r = {name: v[0] for name, v in metrics.groove_descriptors(fref.record(bad)).items()}
    assert r["Statistical::Poly Velocity Mean"] == 0.0 and r["Statistical::Poly Offset Mean"] == 0.125 and r["Auto-Correlation::Max"] == 0.0


def test_distances_of_closed_form_grooves():
    hits = FOUR_ON_THE_FLOOR + [(2, 2), (10, 2), (18, 2)]
    a = np.stack([groove([(t + 1, c) for t, c in hits]), groove(hits, v=0.75, o=0.25), np.zeros((32, 27), np.float32)])
    b = np.stack([groove(hits), groove(hits, v=0.25, o=-0.25), np.zeros((32, 27), np.float32)])
    d = metrics.groove_distances(*fref.groove_features(a, b))
    assert list(d) == list(metrics.DISTANCES)
    assert d["Hamming"].tolist() == [22, 0, 0] and d["Fuzzy Hamming"].tolist() == [11, 0, 0] and d["Jaccard"].tolist() == [1, 0, 0]
    assert d["Velocity L2"].tolist() == [np.sqrt(22.0), np.sqrt(11 * 0.25), 0] and d["Offset RMS"].tolist() == [0, 0.5, 0]
    assert d["Profile Cosine"][0] == 1.0 and abs(d["Profile Cosine"][1]) < 1e-15 and d["Profile Cosine"][2] == 0.0


def test_descriptor_table_on_a_hand_made_sample():
    gt, pred, dist = [1, 2, 3, 4, 10], [2, 2, 5, 1, 0], [0, 1, 2, 3, 4]
    tab = metrics.descriptor_table({"X": gt}, {"X": pred}, {"D": dist}, groups=[0, 0, 1, 1, 7], names=["rock", "jazz"])
    assert list(tab) == ["Overall", "rock", "jazz"] and list(tab["Overall"]) == ["X__Ground_Truth", "X__Prediction", "X__W1", "Distance::D"]
    o = tab["Overall"]
    assert o["X__Ground_Truth"] == {"mean": 4.0, "std": np.sqrt(10.0), "min": 1.0, "max": 10.0, "median": 3.0, "q1": 2.0, "q3": 4.0}
    assert o["X__Prediction"] == {"mean": 2.0, "std": np.sqrt(2.8), "min": 0.0, "max": 5.0, "median": 2.0, "q1": 1.0, "q3": 2.0}
    assert o["X__W1"] == 2.0 and o["Distance::D"]["median"] == 2.0 and o["Distance::D"]["q3"] == 3.0
    assert list(o["X__Prediction"]) == list(metrics.TABLE_STATS) and len(metrics.TABLE_STATS) == 7
    r = tab["rock"]
    assert r["X__Ground_Truth"]["q1"] == 1.25 and r["X__W1"] == 0.5 and r["Distance::D"]["mean"] == 0.5
    assert tab["jazz"]["X__Ground_Truth"]["mean"] == 3.5 and tab["jazz"]["X__W1"] == 1.5        # (3, 4) against (1, 5); tag 7: Overall only
    assert list(metrics.descriptor_table({"X": gt}, {"X": pred})) == ["Overall"]
    assert list(metrics.descriptor_table({"X": gt}, {"X": pred}, groups=[0, 0, 2, 2, 2])) == ["Overall", "group0", "group1", "group2"]
    assert metrics.descriptor_table({"X": gt}, {"X": pred}, groups=[0, 0, 2, 2, 2])["group1"]["X__W1"] == 0.0
    for bad in (dict(desc_gt={"X": gt}, desc_pred={"Y": pred}), dict(desc_gt={"X": gt}, desc_pred={"X": pred[:3]}),
                dict(desc_gt={"X": gt}, desc_pred={"X": pred}, groups=[0, 1]),
                dict(desc_gt={"X": gt}, desc_pred={"X": pred}, groups=[0] * 5, names=["Overall"])):
        with pytest.raises(ValueError):
            metrics.descriptor_table(**bad)


# ---- the Python front on the emulator ------------------------------------------------------------------------------------------------------------
def test_engine_groove_features_on_the_emulator(engine):  # noqa: F811
    import torch
    a, b = (torch.from_numpy(np.array(x)).reshape(-1, 32, 27) for x in inputs(67))
    want_a, want_b, want_p = reference(67)
    fa, fb, pw = engine.groove_features(a, b)
    assert all(t.dtype == torch.int64 for t in (fa, fb, pw)) and tuple(fa.shape) == tuple(fb.shape) == (67, 32) and tuple(pw.shape) == (67, 8)
    assert np.array_equal(fa.numpy(), want_a) and np.array_equal(fb.numpy(), want_b) and np.array_equal(pw.numpy(), want_p)
    only = engine.groove_features(a)
    assert torch.is_tensor(only) and np.array_equal(only.numpy(), want_a)
    fa2, pw2 = engine.groove_features(a, b, feat_b=False, chunk=25)                       # 25 + 25 + 17
    assert np.array_equal(fa2.numpy(), want_a) and np.array_equal(pw2.numpy(), want_p)
    fa3, fb3 = engine.groove_features(a, b, pair=False, chunk=5)
    assert np.array_equal(fa3.numpy(), want_a) and np.array_equal(fb3.numpy(), want_b)
    for bad in (dict(hvo_a=a[:, :, :20]), dict(hvo_a=a, hvo_b=b[:5]), dict(hvo_a=a[:0])):
        with pytest.raises(ValueError):
            engine.groove_features(**bad)


def test_groove_table_on_the_emulator(engine):  # noqa: F811
    import torch

    class Model:
        pass
    model = Model()
    model.engine = engine
    a, b = (torch.from_numpy(np.array(x)).reshape(-1, 32, 27) for x in inputs(67))
    want_a, want_b, want_p = reference(67)
    group = np.arange(67) % 3
    want = metrics.descriptor_table(metrics.groove_descriptors(want_b), metrics.groove_descriptors(want_a),
                                    metrics.groove_distances(want_a, want_b, want_p), groups=group, names=["rock", "funk", "jazz"])
    assert metrics.groove_table(model, a, b, groups=group, names=["rock", "funk", "jazz"]) == want
    assert metrics.groove_table(model, a, b, groups=group, names=["rock", "funk", "jazz"], gt_feat=engine.groove_features(b)) == want
    o = want["Overall"]
    assert len(o) == 3 * len(metrics.DESCRIPTORS) + len(metrics.DISTANCES) and o["Distance::Hamming"]["min"] > 0
    assert 0 < o["Statistical::NoI__W1"] and 0 < o["Auto-Correlation::Beat__Prediction"]["mean"] < 1


def test_train_py_flag_is_off_by_default():
    import train as train_cli
    p = train_cli.build_parser()
    args = p.parse_args(["--experiment", "InfillingClosedHH"])
    assert "eval_descriptors" not in train_cli.load_hyperparameters(args)
    on = train_cli.load_hyperparameters(p.parse_args(["--experiment", "InfillingClosedHH", "--eval_descriptors", "True"]))
    assert on["eval_descriptors"] is True
    assert "eval_descriptors" not in train_cli.load_hyperparameters(p.parse_args(["--experiment", "InfillingClosedHH", "--eval_descriptors", "False"]))
    assert train_cli.load_hyperparameters(p.parse_args(["--experiment", "InfillingClosedHH", "--override", "eval_descriptors=true"]))["eval_descriptors"] is True
