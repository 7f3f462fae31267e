"""Groove descriptors and rhythmic distances on the GPU: the checks of tests/test_groove_features.py on the HIP library (the pass against its
numpy restatement, the closed forms, position independence, the argument checks), and what needs the device: red zones around all six
buffers, the call in a captured graph, metrics.evaluate_descriptors end to end, train.py --eval_descriptors."""
import csv
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import groove_features_ref as fref
from harness import CudaBuf, guarded
from test_groove_features import (COMBOS, REJECTED, check_against_ref, check_boundary_values, check_closed_forms, check_position_independence,
                                  check_rejected, groove_features, inputs, reference)
from test_predict_voices_gpu import DIMS
from transformergrooveinfilling_amd import _lib, layout, metrics

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("n_seq", [1, 3, 67, 1024])
def test_against_the_restatement_hip(n_seq, combo):
    check_against_ref(_lib.get_lib(), CudaBuf, n_seq, combo)


def test_closed_forms_hip():
    check_closed_forms(_lib.get_lib(), CudaBuf)


def test_boundary_values_hip():
    check_boundary_values(_lib.get_lib(), CudaBuf)


def test_position_independence_hip():
    check_position_independence(_lib.get_lib(), CudaBuf)


@pytest.mark.parametrize("case", list(REJECTED))
def test_rejected_before_any_launch_hip(case):
    check_rejected(_lib.get_lib(), CudaBuf, case)


def test_isolation():
    """red zones around the two inputs and the three outputs; the outputs hold garbage beforehand and the call is made twice"""
    lib = _lib.get_lib()
    a, b = inputs(67)
    registry, keep = [], []
    Guarded = guarded(CudaBuf, 0x7FC00000, 4096, registry)
    one = groove_features(lib, Guarded, a, b, fill=0x5EADBEEF5EADBEEF, keep=keep)
    two = groove_features(lib, Guarded, a, b, fill=-1, keep=keep)
    assert len(keep) == 10 and all(x.intact() for x in keep)        # nothing beside any buffer was written
    assert all(np.array_equal(x, y) and np.array_equal(x, w) for x, y, w in zip(one, two, reference(67)))
    # all six of the ABI's pointers: the same buffers with feat_b / pair left out in turn
    for combo_kw, idx in ((dict(feat_b=False), (0, 2)), (dict(pair=False), (0, 1))):
        keep = []
        got = groove_features(lib, Guarded, a, b, fill=0x5EADBEEF5EADBEEF, keep=keep, **combo_kw)
        assert len(keep) == 4 and all(x.intact() for x in keep) and all(np.array_equal(got[i], reference(67)[i]) for i in idx)


def test_capturable():
    """the launch inside a captured graph, replayed three times: the words are stored, so they equal those of a single call"""
    lib = _lib.get_lib()
    a, b = inputs(67)
    want = reference(67)
    ab, bb = (torch.from_numpy(np.array(x)).cuda() for x in (a, b))
    outs = [torch.full((67, w), 0x5EADBEEF, dtype=torch.int64, device="cuda") for w in (32, 32, 8)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call():
        lib.call("gt_groove_features", p(ab), p(bb), ctypes.c_int64(67), p(outs[0]), p(outs[1]), p(outs[2]),
                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                              # (code objects loaded outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    single = [t.cpu().numpy().copy() for t in outs]
    for t in outs:
        t.fill_(0x5EADBEEF)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert all(np.array_equal(t.cpu().numpy(), s) and np.array_equal(s, w) for t, s, w in zip(outs, single, want))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from transformergrooveinfilling_amd.training import initialize_model
    m, _, _ = initialize_model({"model": dict(DIMS, experiment="InfillingClosedHH", encoder_only=1, optimizer="sgd", max_len=32,
                                              embedding_size_tgt=27, device="cuda"),
                                "training": {"learning_rate": 0.05, "batch_size": 8, "hit_loss_penalty": 0.38}, "load_model": None})
    m.engine.load_named(layout.init_params(DIMS, seed=5))
    return m


def test_evaluate_descriptors_equals_the_restatement(model):
    x, y = layout.synthetic_batch(13, 16, seed=3)
    x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    group = np.array([0, 2, 1, 1, 0, 2, 2, 0, 1, 0, 0, 2, 1], np.int32)
    names = ["rock", "funk", "jazz"]
    pred = model.predict_hvo(x).clone()
    want_a, want_b, want_p = fref.groove_features(pred.cpu().numpy(), y.cpu().numpy())
    assert want_a[:, 0].sum() > 0 and want_p[:, 1].sum() > 0        # the model places hits, some of them right
    want = metrics.descriptor_table(metrics.groove_descriptors(want_b), metrics.groove_descriptors(want_a),
                                    metrics.groove_distances(want_a, want_b, want_p), groups=group, names=names)
    res = metrics.evaluate_descriptors(model, x, y, groups=group, names=names)
    assert res == want and list(res) == ["Overall"] + names
    eng = model.engine
    gt_feat = eng.groove_features(y)
    assert np.array_equal(gt_feat.cpu().numpy(), want_b)
    assert metrics.evaluate_descriptors(model, x, y, groups=group, names=names, gt_feat=gt_feat) == want
    whole, chunked = eng.groove_features(pred, y), eng.groove_features(pred, y, chunk=5)          # 5 + 5 + 3
    assert all(torch.equal(w, c) for w, c in zip(whole, chunked))
    assert all(np.array_equal(w.cpu().numpy(), r) for w, r in zip(whole, (want_a, want_b, want_p)))


def _train(tmp_path, *extra):
    sys.path.insert(0, ROOT)
    import train as train_cli
    xe, ye = train_cli.synthetic_tensors(48, 16, 77)
    npz = tmp_path / "eval.npz"
    np.savez(npz, validation_inputs=xe.numpy(), validation_gt=ye.numpy(), validation_groups=(np.arange(48) % 3).astype(np.int64),
             group_names=np.array(["rock", "funk", "jazz"]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--experiment", "InfillingClosedHH", "--synthetic", "64", "--epochs", "1",
                        "--wandb", "False", "--save-dir", str(tmp_path), "--eval-size", "64", "--eval-npz", str(npz)] + list(extra),
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def test_train_py_descriptor_leg(tmp_path):
    r = _train(tmp_path, "--eval_descriptors", "True")
    assert "Validation_Set descriptors:" in r.stdout and "Train_Set descriptors:" in r.stdout
    rows = list(csv.reader(open(tmp_path / "stats_Validation_Set_local_Epoch_0.csv")))
    cols = rows[0][1:]
    assert [row[0] for row in rows[1:]] == list(metrics.TABLE_STATS) and all(len(row) == len(rows[0]) for row in rows)
    assert cols == [d + s for d in metrics.DESCRIPTORS for s in ("__Ground_Truth", "__Prediction")] + ["Distance::" + d for d in metrics.DISTANCES]
    table = {c: {row[0]: float(row[1 + i]) for row in rows[1:]} for i, c in enumerate(cols)}
    assert all(v["min"] <= v["q1"] <= v["median"] <= v["q3"] <= v["max"] and v["min"] <= v["mean"] <= v["max"] for v in table.values())
    assert table["Statistical::NoI__Ground_Truth"]["max"] >= 1 and 0 < table["Statistical::Total Step Density__Ground_Truth"]["mean"] <= 1
    by_group = json.load(open(tmp_path / "stats_Validation_Set_groups_Epoch_0.json"))
    assert all(n in by_group for n in ("Overall", "rock", "funk", "jazz")) and by_group["groups"] == ["rock", "funk", "jazz"]
    assert by_group["Overall"]["Distance::Hamming"]["mean"] == table["Distance::Hamming"]["mean"]
    assert os.path.exists(tmp_path / "stats_Train_Set_local_Epoch_0.csv") and not os.path.exists(tmp_path / "stats_Train_Set_groups_Epoch_0.json")
    ev = json.load(open(tmp_path / "eval_Validation_Set_Epoch_0.json"))
    assert sorted(ev) == sorted(["epoch"] + ["%s_%s" % (q, v) for q, _ in metrics.GROUPS for v in ("Overall",) + metrics.VOICES])


def test_train_py_without_the_flag_writes_no_stats(tmp_path):
    r = _train(tmp_path)
    assert "descriptors:" not in r.stdout and not [f for f in os.listdir(tmp_path) if f.startswith("stats_")]
    assert os.path.exists(tmp_path / "eval_Validation_Set_Epoch_0.json")
