"""Per-group and removed-cell evaluation counts on the GPU: the checks of tests/test_group_metrics.py on the HIP library (the counting pass
against its numpy restatement, accumulation, garbage in scratch, the all-zero mask, the cross-check with gt_voice_metrics, the argument
checks), and what needs the device: metrics.evaluate_groups end to end, the event-level round trip, red zones around acc / seq_out /
scratch, train.py with a tagged validation set."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import group_metrics_ref as gref
from harness import CudaBuf, guarded
from test_group_metrics import (MASKS, REJECTED, check_accumulate, check_against_ref, check_rejected, check_scratch, check_voice_metrics_agree,
                                check_zero_mask, group_metrics, inputs, mask_of, tags)
from test_infill_events import GROOVES, IDX, OPTS, STATES, opts_struct, run_gather, run_merge, state_buf
from test_predict_voices_gpu import DIMS
from transformergrooveinfilling_amd import _lib, layout, metrics

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("n_groups", [1, 5, 64])
@pytest.mark.parametrize("n_seq", [1, 3, 67, 1024])
def test_against_the_restatement_hip(n_seq, n_groups, mask):
    check_against_ref(_lib.get_lib(), CudaBuf, n_seq, n_groups, mask)


@pytest.mark.parametrize("n_groups,mask", [(1, "null"), (5, "random")])
def test_without_seq_out_hip(n_groups, mask):
    check_against_ref(_lib.get_lib(), CudaBuf, 67, n_groups, mask, seq_out=False)


def test_accumulation_hip():
    check_accumulate(_lib.get_lib(), CudaBuf)


def test_scratch_garbage_hip():
    check_scratch(_lib.get_lib(), CudaBuf)


def test_all_zero_mask_hip():
    check_zero_mask(_lib.get_lib(), CudaBuf)


def test_agrees_with_voice_metrics_hip():
    check_voice_metrics_agree(_lib.get_lib(), CudaBuf)


@pytest.mark.parametrize("case", list(REJECTED))
def test_rejected_before_any_launch_hip(case):
    check_rejected(_lib.get_lib(), CudaBuf, case)


def test_capturable():
    """the two launches inside a captured graph: replays keep adding onto acc"""
    lib = _lib.get_lib()
    pred, gt = inputs(67)
    group = tags(67, 5)
    want, want_seq = gref.group_metrics(pred, gt, group, None, 5)
    pb, gb, grp = (torch.from_numpy(np.array(a)).cuda() for a in (pred, gt, group))
    acc, seq = torch.zeros(gref.acc_words(5), dtype=torch.int64, device="cuda"), torch.zeros(67, 4, dtype=torch.int32, device="cuda")
    scratch = torch.empty(int(lib.cdll.gt_group_metrics_scratch_words(ctypes.c_int64(67), 5)), dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call():
        lib.call("gt_group_metrics", p(pb), p(gb), p(grp), None, ctypes.c_int64(67), 5, p(acc), p(seq), p(scratch),
                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                              # (code objects loaded outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    acc.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(acc.cpu().numpy(), 3 * want) and np.array_equal(seq.cpu().numpy(), want_seq)


# ---- 1. end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from transformergrooveinfilling_amd.training import initialize_model
    m, _, _ = initialize_model({"model": dict(DIMS, experiment="InfillingClosedHH", encoder_only=1, optimizer="sgd", max_len=32,
                                              embedding_size_tgt=27, device="cuda"),
                                "training": {"learning_rate": 0.05, "batch_size": 8, "hit_loss_penalty": 0.38}, "load_model": None})
    m.engine.load_named(layout.init_params(DIMS, seed=5))
    return m


def test_evaluate_groups_equals_the_restatement(model):
    x, y = layout.synthetic_batch(13, 16, seed=3)
    x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    group = np.array([0, 2, 1, 1, 0, 2, 2, 0, 1, 0, 0, 2, 1], np.int32)
    names = ["rock", "funk", "jazz"]
    pred = model.predict_hvo(x).clone()
    want, want_seq = gref.group_metrics(pred.cpu().numpy(), y.cpu().numpy(), group, None, 3)
    assert want[:216].reshape(3, 9, 8)[:, :, 1].sum() > 0           # the model places hits that are right: not a count of empty cells only
    res = metrics.evaluate_groups(model, x, y, group, names=names)
    assert res == metrics.group_metrics_from_acc(want, 3, names)
    assert [res[n]["Sequences"] for n in names] == [5.0, 4.0, 4.0] and res["Overall"]["Cells"] == 13 * 288.0
    eng = model.engine
    acc, seq = eng.group_metrics(pred, y, groups=group, n_groups=3, seq_counts=True)
    assert np.array_equal(acc.cpu().numpy(), want) and np.array_equal(seq.cpu().numpy(), want_seq)
    assert np.array_equal(eng.group_metrics(pred, y, groups=group, n_groups=3, chunk=5).cpu().numpy(), want)          # 5 + 5 + 3
    half = eng.group_metrics(pred[:6], y[:6], groups=group[:6], n_groups=3)
    assert eng.group_metrics(pred[6:], y[6:], groups=group[6:], n_groups=3, acc=half) is half and np.array_equal(half.cpu().numpy(), want)
    ranks = metrics.rank_sequences(seq, groups=group, k=2)
    den = 2 * want_seq[:, 1] + want_seq[:, 2] + want_seq[:, 3]
    f1 = np.where(den > 0, 2 * want_seq[:, 1] / np.maximum(den, 1), 0.0)
    for g in range(3):
        idx = np.flatnonzero(group == g)
        assert ranks[g]["lowest"] == [int(i) for i in idx[np.argsort(f1[idx], kind="stable")][:2]]


# ---- 2. the event-level round trip -----------------------------------------------------------------------------------------------------------
def test_events_round_trip():
    """pred = y, in = x and the cells of one gt_gather_infill_events call, merged by gt_infill_merge_cells: over the removed cells the finished
    groove IS the source -- every removed hit a TP at zero error"""
    lib = _lib.get_lib()
    idx = IDX[8]
    rc, x, y, cells = run_gather(lib, CudaBuf, CudaBuf(GROOVES), CudaBuf(np.array(idx, np.int64)), opts_struct(OPTS["r46"]),
                                 state_buf(CudaBuf, *STATES[0]))
    assert rc == 0
    rc, done, _ = run_merge(lib, CudaBuf, y, x, cells, 1)
    assert rc == 0
    got, seq = group_metrics(lib, CudaBuf, done, GROOVES, None, cells, 1)
    w = gref.split(got, 1)[0][0]                                    # (9, 8)
    n_removed = sum(bin(int(v)).count("1") for v in cells.reshape(-1))
    assert n_removed > 0 and int(w[:, 0].sum()) == n_removed
    assert int(w[:, 1].sum()) == n_removed and not w[:, 2].any() and not w[:, 3].any()      # TP = the removed cells; FP = FN = 0
    assert not w[:, 4:].any()                                                              # zero error, on the hits too (words 6, 7)
    assert np.array_equal(seq[:, 0], seq[:, 1]) and int(seq[:, 1].sum()) == n_removed


# ---- 3. isolation: red zones around acc, seq_out and scratch; garbage in scratch --------------------------------------------------------------
@pytest.mark.parametrize("n_groups", [5, 64])
def test_isolation(n_groups):
    lib = _lib.get_lib()
    pred, gt = inputs(67)
    group, cells = tags(67, n_groups), mask_of("random", 67)
    registry, keep = [], []
    Guarded = guarded(CudaBuf, 0x7FC00000, 4096, registry)
    one = group_metrics(lib, Guarded, pred, gt, group, cells, n_groups, scratch_fill=0x5EADBEEF, keep=keep)
    two = group_metrics(lib, Guarded, pred, gt, group, cells, n_groups, scratch_fill=0xFFFFFFFF, keep=keep)
    assert len(keep) == 14 and all(b.intact() for b in keep)        # nothing beside any buffer was written (acc, seq_out, scratch, the inputs)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    want = gref.group_metrics(pred, gt, group, cells, n_groups)
    assert np.array_equal(one[0], want[0]) and np.array_equal(one[1], want[1])


# ---- 4. train.py with a tagged validation set -------------------------------------------------------------------------------------------------
def test_train_py_group_evaluation(tmp_path):
    sys.path.insert(0, ROOT)
    import train as train_cli
    xe, ye = train_cli.synthetic_tensors(48, 16, 77)
    names = ["rock", "funk", "jazz"]
    groups = (np.arange(48) % 3).astype(np.int64)
    npz = tmp_path / "eval.npz"
    np.savez(npz, validation_inputs=xe.numpy(), validation_gt=ye.numpy(), validation_groups=groups, group_names=np.array(names))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--experiment", "InfillingClosedHH", "--synthetic", "64", "--epochs", "1",
                        "--wandb", "False", "--save-dir", str(tmp_path), "--eval-size", "64", "--eval-npz", str(npz), "--dump_eval", "True"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert all("Validation_Set / %s:" % n in r.stdout for n in names)
    by_group = json.load(open(tmp_path / "eval_Validation_Set_groups_Epoch_0.json"))
    assert all(0.0 <= by_group[n]["Hits_F1_Overall"] <= 1.0 for n in names + ["Overall"])
    assert sum(by_group[n]["Sequences"] for n in names) == 48 == by_group["Overall"]["Sequences"] and by_group["Skipped_Sequences"] == 0
    ev = json.load(open(tmp_path / "eval_Validation_Set_Epoch_0.json"))
    assert sorted(ev) == sorted(["epoch"] + ["%s_%s" % (q, v) for q, _ in metrics.GROUPS for v in ("Overall",) + metrics.VOICES])
    assert not os.path.exists(tmp_path / "eval_Train_Set_groups_Epoch_0.json")       # an untagged set gets no per-group file
    assert abs(by_group["Overall"]["Hits_Accuracy_KICK"] - ev["Hits_Accuracy_KICK"]) < 1e-6    # the same predictions, counted twice


# ---- 5. train.py on full grooves: the finished groove scored over the removed part alone --------------------------------------------------------
@pytest.mark.parametrize("mode", ["voices", "events"])
def test_train_py_infill_removed_part(tmp_path, mode):
    sys.path.insert(0, ROOT)
    import train as train_cli
    from transformergrooveinfilling_amd import infill
    hvo, val = train_cli.synthetic_tensors(64, 27, 5)[1], train_cli.synthetic_tensors(24, 27, 6)[1]
    val[3] = 0                                                      # a groove nothing can be removed from: the pairing leaves it out, tag and all
    np.savez(tmp_path / "grooves.npz", hvo=hvo.numpy())
    np.savez(tmp_path / "eval.npz", validation_hvo=val.numpy(), validation_groups=np.arange(24) % 2, group_names=np.array(["even", "odd"]))
    exp = "InfillingRandom_Symbolic" if mode == "events" else "InfillingClosedHH_Symbolic"
    model = train_cli.main(["--experiment", exp, "--infill-npz", str(tmp_path / "grooves.npz"), "--infill_mode", mode, "--eval-npz",
                            str(tmp_path / "eval.npz"), "--epochs", "1", "--wandb", "False", "--save-dir", str(tmp_path), "--d_model", "32",
                            "--n_heads", "4", "--dim_feedforward", "16", "--num_encoder_decoder_layers", "2", "--batch_size", "16",
                            "--eval-size", "32"])
    recs = {k.split("/", 1)[0]: r for r in model.eval_log for k in r if "/" in k}
    assert sorted(recs) == ["Train_Set", "Validation_Set"]
    if mode == "events":
        kw = dict(mode="events", voices=list(range(9)), ratio=[0.4, 0.6])
        x, y, cells = infill.pair_once_events(val, kw, seed=0, device="cuda")
        n_cells = sum(bin(int(w)).count("1") for w in cells.cpu().numpy().view(np.uint32).reshape(-1))
    else:
        x, y, removed = infill.pair_once(val, dict(voices=[2], min_remove=1, max_remove=1, prob=None), seed=0, device="cuda")
        n_cells = 32 * sum(bin(int(w)).count("1") for w in removed.cpu().numpy().reshape(-1))
    n = x.shape[0]
    kept = infill.eligible(val.cuda(), kw if mode == "events" else dict(voices=[2])).cpu().numpy()
    n_even = int((kept % 2 == 0).sum())
    r = recs["Validation_Set"]
    get = lambda k: r["Validation_Set/" + k]
    assert 0 < n < 24 and n_cells > 0 and get("Infill_Removed_Cells") == n_cells and get("Infill_Removed_Sequences") == n
    assert 0.0 <= get("Infill_Removed_Hits_F1_Overall") <= 1.0 and get("Infill_Removed_Rejected_Values") == 0
    assert get("even/Sequences") + get("odd/Sequences") == n and get("even/Sequences") == n_even and get("odd/Sequences") == n - n_even and 3 not in kept
    if mode == "events":
        # outside the removed cells the finished groove is the source by construction: every hit mismatch of the whole groove lies inside them
        wrong_whole = (1.0 - get("Infill_Hits_Accuracy_Overall")) * n * 288
        wrong_removed = (1.0 - get("Infill_Removed_Hits_Accuracy_Overall")) * n_cells
        assert abs(wrong_whole - wrong_removed) < 0.5 and get("Infill_Removed_Hits_Accuracy_Overall") <= get("Infill_Hits_Accuracy_Overall")
    assert "Train_Set/Infill_Removed_Hits_F1_Overall" in recs["Train_Set"] and not any("/even/" in k for k in recs["Train_Set"])
