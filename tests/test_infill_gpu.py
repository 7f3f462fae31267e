"""Infilling pairs on the GPU: the checks of tests/test_infill.py on the HIP library (gt_gather_infill / gt_infill_merge against the
restatement, exact), a captured graph that draws afresh at every replay, and the Python interface: StepEngine.train_step_indexed_infill
against a second engine fed the restatement's arrays, model.infill."""
import ctypes

import numpy as np
import pytest
import torch

import infill_ref as ref
from test_infill import (GROOVES, IDX, MERGE_REJECTED, OPTS, REJECTED, STATES, check_gather, check_merge, check_merge_rejected, check_rejected,
                         check_round_trip, check_without_removed, opts_struct)
from transformergrooveinfilling_amd import _lib, layout

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("state", STATES, ids=["s3", "s4", "seed2"])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("optname", list(OPTS))
def test_gather_infill_against_restatement_hip(optname, B, state):
    check_gather("hip", optname, B, state)


def test_removed_may_be_null_hip():
    check_without_removed("hip")


@pytest.mark.parametrize("case", list(REJECTED))
def test_gather_rejected_before_any_launch_hip(case):
    check_rejected("hip", case)


@pytest.mark.parametrize("alias", [False, True], ids=["out", "alias"])
@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("mode", [0, 1])
def test_merge_against_restatement_hip(mode, masked, alias):
    check_merge("hip", mode, masked, alias)


def test_round_trip_gives_back_the_groove_hip():
    check_round_trip("hip")


@pytest.mark.parametrize("case", list(MERGE_REJECTED))
def test_merge_rejected_before_any_launch_hip(case):
    check_merge_rejected("hip", case)


def _state(seed_lo, seed_hi, step):
    st = _lib.GtStepState(seed_lo, seed_hi, step, 0, 0.05, 1.0, 0.9, 0.999, 1e-8)
    return torch.from_numpy(np.frombuffer(bytes(st), dtype=np.uint8).copy()).cuda()


def test_graph_replay_draws_afresh():
    """[gt_gather_infill, gt_optimizer_step on a 64-float dummy] captured as one chain: the update advances the device step, so each replay
    draws the restatement's masks of the next step with no argument touched from the host"""
    lib = _lib.get_lib()
    o, idx, s0 = OPTS["all_1_9"], IDX[7], 3
    hvo, ix = torch.from_numpy(GROOVES).cuda(), torch.tensor(idx, dtype=torch.int64).cuda()
    x, y = torch.zeros(7, 32, 27, device="cuda"), torch.zeros(7, 32, 27, device="cuda")
    rem = torch.zeros(7, dtype=torch.int32, device="cuda")
    prm, grd = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    state = _state(1234, 99, s0)
    io = opts_struct(o)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def chain():
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        lib.call("gt_gather_infill", p(hvo), p(ix), ctypes.c_int64(7), 7, ctypes.byref(io), p(state), p(x), p(y), p(rem), stream)
        lib.call("gt_optimizer_step", 0, p(prm), p(grd), None, None, ctypes.c_int64(64), p(state), 0, stream)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()                                             # (code objects loaded outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    state.copy_(_state(1234, 99, s0))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    want = [ref.gather_infill(GROOVES, idx, o, 1234, 99, s0 + i) for i in range(3)]
    assert (want[0][2] != want[1][2]).any() and (want[1][2] != want[2][2]).any()
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(rem.cpu().numpy(), want[i][2]), i
        assert np.array_equal(x.cpu().numpy(), want[i][0]) and np.array_equal(y.cpu().numpy(), want[i][1])


# ---- the Python interface ----------------------------------------------------------------------------------------------------------------
DIMS = dict(d_model=32, n_heads=4, dim_feedforward=16, num_encoder_layers=2, num_decoder_layers=0, dropout=0.1, embedding_size_src=27)
LOSS_TOL = 2e-5                                             # tests/parity.py's loss tolerance of the fp32 path (relative to max(1, |loss|))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_engine_indexed_infill_step(use_graph):
    from transformergrooveinfilling_amd.engine import StepEngine
    seed = 1234 | (99 << 32)
    kw = dict(batch_size=4, optimizer="sgd", learning_rate=0.05, hit_loss_penalty=0.5, seed=seed, device="cuda:0", **DIMS)
    a, b = StepEngine(use_graph=use_graph, **kw), StepEngine(use_graph=False, **kw)
    P = layout.init_params(DIMS, seed=5)
    a.load_named(P); b.load_named(P)
    o = OPTS["w112"]
    a.infill_opts = a.make_infill_opts(voices=[0, 2, 4, 5], min_remove=1, max_remove=3, prob=[1, 1, 2])
    assert a.infill_opts == _lib.infill_opts_tuple(opts_struct(o))
    hvo = torch.from_numpy(GROOVES).cuda()
    for step, idx in enumerate(([5, 0, 6, 4], [0, 6, 5, 5])):
        la = float(a.train_step_indexed_infill(hvo, torch.tensor(idx, dtype=torch.int64, device="cuda"))[0])
        wx, wy, wrem = ref.gather_infill(GROOVES, idx, o, 1234, 99, step)
        s = a.slot(4)
        assert np.array_equal(s.removed.cpu().numpy(), wrem) and (wrem != 0).all()
        assert np.array_equal(s.x.cpu().numpy(), wx) and np.array_equal(s.y.cpu().numpy(), wy)
        lb = float(b.train_step(torch.from_numpy(wx), torch.from_numpy(wy))[0])
        print("step %d: loss %.8f (restatement's arrays through train_step: %.8f)" % (step, la, lb))
        assert abs(la - lb) < LOSS_TOL * max(1.0, abs(lb)), (step, la, lb)
    assert a.state_struct().step == 2


def test_engine_infill_step_needs_a_symbolic_model_and_options():
    from transformergrooveinfilling_amd.engine import StepEngine
    hvo, idx = torch.from_numpy(GROOVES).cuda(), torch.tensor([0, 5], dtype=torch.int64, device="cuda")
    e16 = StepEngine(32, 4, 16, 2, embedding_size_src=16, batch_size=2, device="cuda:0", infill_opts=(4, 1, 1) + (1,) + (0,) * 8)
    with pytest.raises(ValueError, match="symbolic"):
        e16.train_step_indexed_infill(hvo, idx)
    e27 = StepEngine(32, 4, 16, 2, embedding_size_src=27, batch_size=2, device="cuda:0")
    with pytest.raises(ValueError, match="infill_opts"):
        e27.train_step_indexed_infill(hvo, idx)


def test_model_infill_keeps_every_input_hit():
    from transformergrooveinfilling_amd.training import initialize_model
    m, _, _ = initialize_model({"model": dict(DIMS, experiment="InfillingClosedHH_Symbolic", encoder_only=1, optimizer="sgd", max_len=32,
                                              embedding_size_tgt=27, device="cuda"),
                                "training": {"learning_rate": 0.05, "batch_size": 4, "hit_loss_penalty": 0.5}, "load_model": None})
    m.engine.load_named(layout.init_params(DIMS, seed=5))
    idx = [0, 4, 5, 6]
    x, _, rem = ref.gather_infill(GROOVES, idx, OPTS["w112"], 1234, 99, 0)
    xin = torch.from_numpy(x).cuda()
    pred = m.predict_hvo(xin, thres=0.3).cpu().numpy()
    hit = x[..., :9] != 0
    for mode in (1, 0):
        for removed in (None, torch.from_numpy(rem)):
            out = m.infill(xin, removed=removed, mode=mode, thres=0.3)
            assert out.shape == (4, 32, 27)
            got = out.cpu().numpy()
            assert np.array_equal(got, ref.merge(pred, x, None if removed is None else rem, mode))
            assert np.array_equal(got[..., :9][hit], x[..., :9][hit])                     # the input's hits are all preserved
            if mode == 1:
                assert np.array_equal(got[..., 9:18][hit], x[..., 9:18][hit]) and np.array_equal(got[..., 18:][hit], x[..., 18:][hit])
    m16, _, _ = initialize_model({"model": dict(DIMS, embedding_size_src=16, experiment="InfillingClosedHH", encoder_only=1, optimizer="sgd",
                                                max_len=32, embedding_size_tgt=27, device="cuda"),
                                  "training": {"learning_rate": 0.05, "batch_size": 4, "hit_loss_penalty": 0.5}, "load_model": None})
    with pytest.raises(ValueError, match="symbolic"):
        m16.infill(xin)


def test_loader_and_train_loop_train_from_full_grooves():
    """DeviceBatchLoader.infilling + train_loop: the indexed step with gt_gather_infill, from ONE tensor of full grooves"""
    from transformergrooveinfilling_amd import parallel
    from transformergrooveinfilling_amd.training import calculate_loss, initialize_model, train_loop
    m, opt, _ = initialize_model({"model": dict(DIMS, experiment="InfillingClosedHH_Symbolic", encoder_only=1, optimizer="sgd", max_len=32,
                                                embedding_size_tgt=27, device="cuda"),
                                  "training": {"learning_rate": 0.05, "batch_size": 2, "hit_loss_penalty": 0.5}, "load_model": None})
    ld = parallel.DeviceBatchLoader.infilling(GROOVES, dict(voices=[2]), 2, "cuda:0", seed=1)
    called = []
    call = m.engine.lib.call
    m.engine.lib.call = lambda name, *a: (called.append(name), call(name, *a))[1]
    try:
        rec = train_loop(dataloader=ld, groove_transformer=m, encoder_only=1, opt=opt, epoch=0, loss_fn=calculate_loss,
                         bce_fn=torch.nn.BCEWithLogitsLoss(reduction="none"), mse_fn=torch.nn.MSELoss(reduction="none"), device="cuda:0",
                         hit_loss_penalty=0.5)
    finally:
        m.engine.lib.call = call
    assert called.count("gt_gather_infill") >= 1 and "gt_gather_batch" not in called
    assert np.isfinite(rec["train/loss"]) and m.engine.state_struct().step == len(ld) == 2
    rem = m.engine.slot(2).removed.cpu().numpy()
    assert (rem == 4).all()                                  # the closed hi-hat, removed from two eligible grooves
