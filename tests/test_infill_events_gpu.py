"""Event-level infilling pairs on the GPU: the checks of tests/test_infill_events.py on the HIP library (gt_gather_infill_events /
gt_infill_merge_cells against the restatement, exact), a captured graph that draws afresh at every replay, and the Python interface:
StepEngine.train_step_indexed_infill_events against a second engine fed the restatement's arrays, model.infill(cells=...), train_loop over
the loader's event form."""
import ctypes

import numpy as np
import pytest
import torch

import infill_events_ref as ref
from test_infill_events import (ELIGIBLE, GROOVES, IDX, MERGE_REJECTED, OPTS, REJECTED, STATES, check_gather, check_merge, check_merge_rejected,
                                check_rejected, check_round_trip, check_without_cells, opts_struct)
from transformergrooveinfilling_amd import _lib, layout

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("state", STATES, ids=["s3", "s4", "seed2"])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("optname", list(OPTS))
def test_gather_events_against_restatement_hip(optname, B, state):
    check_gather("hip", optname, B, state)


@pytest.mark.parametrize("optname", list(OPTS))
def test_gather_events_every_groove_in_one_batch_hip(optname):
    cells = check_gather("hip", optname, 8, STATES[0])
    assert np.nonzero(cells.any(1))[0].tolist() == ELIGIBLE[optname]


def test_cells_may_be_null_hip():
    check_without_cells("hip")


@pytest.mark.parametrize("case", list(REJECTED))
def test_gather_events_rejected_before_any_launch_hip(case):
    check_rejected("hip", case)


@pytest.mark.parametrize("alias", [False, True], ids=["out", "alias"])
@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("mode", [0, 1])
def test_merge_cells_against_restatement_hip(mode, masked, alias):
    check_merge("hip", mode, masked, alias)


def test_round_trip_gives_back_the_groove_hip():
    check_round_trip("hip")


@pytest.mark.parametrize("case", list(MERGE_REJECTED))
def test_merge_cells_rejected_before_any_launch_hip(case):
    check_merge_rejected("hip", case)


def _state(seed_lo, seed_hi, step):
    st = _lib.GtStepState(seed_lo, seed_hi, step, 0, 0.05, 1.0, 0.9, 0.999, 1e-8)
    return torch.from_numpy(np.frombuffer(bytes(st), dtype=np.uint8).copy()).cuda()


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def test_graph_replay_draws_afresh():
    """[gt_gather_infill_events, gt_optimizer_step on a 64-float dummy] captured as one chain: the update advances the device step, so each
    replay draws the restatement's cells of the next step with no argument touched from the host"""
    lib = _lib.get_lib()
    o, idx, s0 = OPTS["r46"], IDX[8], 3
    hvo, ix = torch.from_numpy(GROOVES).cuda(), torch.tensor(idx, dtype=torch.int64).cuda()
    x, y = torch.zeros(8, 32, 27, device="cuda"), torch.zeros(8, 32, 27, device="cuda")
    cells = torch.zeros(8, 9, dtype=torch.int32, device="cuda")
    prm, grd = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    state = _state(1234, 99, s0)
    eo = opts_struct(o)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def chain():
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        lib.call("gt_gather_infill_events", p(hvo), p(ix), ctypes.c_int64(8), 8, ctypes.byref(eo), p(state), p(x), p(y), p(cells), stream)
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
    want = [ref.gather_infill_events(GROOVES, idx, o, 1234, 99, s0 + i) for i in range(3)]
    assert (want[0][2] != want[1][2]).any() and (want[1][2] != want[2][2]).any()
    for i in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_words(cells), want[i][2]), i
        assert np.array_equal(x.cpu().numpy(), want[i][0]) and np.array_equal(y.cpu().numpy(), want[i][1])


# ---- the Python interface ----------------------------------------------------------------------------------------------------------------
DIMS = dict(d_model=32, n_heads=4, dim_feedforward=16, num_encoder_layers=2, num_decoder_layers=0, dropout=0.1, embedding_size_src=27)
LOSS_TOL = 2e-5                                             # tests/parity.py's loss tolerance of the fp32 path (relative to max(1, |loss|))
MODEL = dict(DIMS, experiment="InfillingRandom_Symbolic", encoder_only=1, optimizer="sgd", max_len=32, embedding_size_tgt=27, device="cuda")


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_engine_indexed_infill_events_step(use_graph):
    from transformergrooveinfilling_amd.engine import StepEngine
    seed = 1234 | (99 << 32)
    kw = dict(batch_size=4, optimizer="sgd", learning_rate=0.05, hit_loss_penalty=0.5, seed=seed, device="cuda:0", **DIMS)
    a, b = StepEngine(use_graph=use_graph, **kw), StepEngine(use_graph=False, **kw)
    P = layout.init_params(DIMS, seed=5)
    a.load_named(P); b.load_named(P)
    o = OPTS["sub"]
    a.infill_event_opts = a.make_infill_event_opts(voices=[0, 2, 4, 5], ratio=(0.4, 0.6))
    assert a.infill_event_opts == _lib.infill_event_opts_tuple(opts_struct(o))
    hvo = torch.from_numpy(GROOVES).cuda()
    for step, idx in enumerate(([5, 0, 6, 3], [0, 6, 7, 7])):
        la = float(a.train_step_indexed_infill_events(hvo, torch.tensor(idx, dtype=torch.int64, device="cuda"))[0])
        wx, wy, wcells = ref.gather_infill_events(GROOVES, idx, o, 1234, 99, step)
        s = a.slot(4)
        assert tuple(s.cells.shape) == (4, 9) and np.array_equal(_words(s.cells), wcells) and wcells.any(1).all()
        assert np.array_equal(s.x.cpu().numpy(), wx) and np.array_equal(s.y.cpu().numpy(), wy)
        lb = float(b.train_step(torch.from_numpy(wx), torch.from_numpy(wy))[0])
        print("step %d: loss %.8f (restatement's arrays through train_step: %.8f)" % (step, la, lb))
        assert abs(la - lb) < LOSS_TOL * max(1.0, abs(lb)), (step, la, lb)
    assert a.state_struct().step == 2


def test_engine_events_step_needs_a_symbolic_model_and_options():
    from transformergrooveinfilling_amd.engine import StepEngine
    hvo, idx = torch.from_numpy(GROOVES).cuda(), torch.tensor([0, 5], dtype=torch.int64, device="cuda")
    e16 = StepEngine(32, 4, 16, 2, embedding_size_src=16, batch_size=2, device="cuda:0", infill_event_opts=("events", 0x1FF, 26214, 39322))
    with pytest.raises(ValueError, match="symbolic"):
        e16.train_step_indexed_infill_events(hvo, idx)
    e27 = StepEngine(32, 4, 16, 2, embedding_size_src=27, batch_size=2, device="cuda:0")
    with pytest.raises(ValueError, match="infill_event_opts"):
        e27.train_step_indexed_infill_events(hvo, idx)


def test_model_infill_confines_the_prediction_to_the_cells():
    from transformergrooveinfilling_amd.training import initialize_model
    m, _, _ = initialize_model({"model": MODEL, "training": {"learning_rate": 0.05, "batch_size": 4, "hit_loss_penalty": 0.5}, "load_model": None})
    m.engine.load_named(layout.init_params(DIMS, seed=5))
    idx = [0, 5, 6, 7]
    x, _, cells = ref.gather_infill_events(GROOVES, idx, OPTS["r46"], 1234, 99, 0)
    inside = np.array([[[bool(int(cells[s][c]) >> t & 1) for c in range(9)] for t in range(32)] for s in range(4)])
    xin = torch.from_numpy(x).cuda()
    pred = m.predict_hvo(xin, thres=0.3).cpu().numpy()
    hit = x[..., :9] != 0
    assert (pred[..., :9] != 0)[~inside & ~hit].any()                                     # (the model does place hits outside the cells)
    for mode in (1, 0):
        for given in (torch.from_numpy(cells.view(np.int32)), torch.from_numpy(inside).cuda()):
            out = m.infill(xin, cells=given, mode=mode, thres=0.3)
            assert out.shape == (4, 32, 27)
            got = out.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), ref.merge_cells(pred, x, cells, mode).view(np.uint32))
            assert np.array_equal(got[..., :9][hit], x[..., :9][hit])                     # the input's hits are all preserved
            assert np.array_equal(got[..., :9][~inside], x[..., :9][~inside])             # nothing is placed outside the cells
            for part in (got[..., 9:18], got[..., 18:]):
                assert not part[~inside & ~hit].any()
    with pytest.raises(ValueError, match="not both"):
        m.infill(xin, removed=torch.zeros(4, dtype=torch.int32), cells=torch.from_numpy(inside))


def test_loader_and_train_loop_train_from_full_grooves_by_events():
    """DeviceBatchLoader.infilling with event options + train_loop: the indexed step with gt_gather_infill_events, from ONE tensor of full
    grooves"""
    from transformergrooveinfilling_amd import parallel
    from transformergrooveinfilling_amd.training import calculate_loss, initialize_model, train_loop
    m, opt, _ = initialize_model({"model": MODEL, "training": {"learning_rate": 0.05, "batch_size": 2, "hit_loss_penalty": 0.5}, "load_model": None})
    ld = parallel.DeviceBatchLoader.infilling(GROOVES, dict(mode="events"), 2, "cuda:0", seed=1)
    assert ld.pool.tolist() == ELIGIBLE["r46"]
    called = []
    call = m.engine.lib.call
    m.engine.lib.call = lambda name, *a: (called.append(name), call(name, *a))[1]
    try:
        rec = train_loop(dataloader=ld, groove_transformer=m, encoder_only=1, opt=opt, epoch=0, loss_fn=calculate_loss,
                         bce_fn=torch.nn.BCEWithLogitsLoss(reduction="none"), mse_fn=torch.nn.MSELoss(reduction="none"), device="cuda:0",
                         hit_loss_penalty=0.5)
    finally:
        m.engine.lib.call = call
    assert called.count("gt_gather_infill_events") >= 1 and "gt_gather_batch" not in called and "gt_gather_infill" not in called
    assert np.isfinite(rec["train/loss"]) and m.engine.state_struct().step == len(ld) == 3
    assert m.engine.infill_event_opts == ("events", 0x1FF, 26214, 39322)
    cells = _words(m.engine.slot(2).cells)                   # (6 eligible grooves in 3 batches of 2)
    assert cells.any(1).all()                                # hits were removed from both grooves of the last batch
