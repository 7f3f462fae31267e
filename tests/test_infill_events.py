"""Event-level infilling pairs drawn in the gather (gt_gather_infill_events) and the cell-masked way back (gt_infill_merge_cells) on the host
emulator build of the kernel sources, against the restatement in tests/infill_events_ref.py: every comparison is exact (the draw is integer
arithmetic, kept values are bit copies).  The check_* functions take the backend; tests/test_infill_events_gpu.py runs them on the HIP
library.  Also the host side that needs no GPU: events_eligible, make_infill_event_opts, as_opts, the loader's event form, train.py's flags
and YAML keys."""
import ctypes
import os
import sys

import numpy as np
import pytest

import infill_events_ref as ref
from harness import CudaBuf, NpBuf, emu_lib
from transformergrooveinfilling_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the 8 hand-built grooves -----------------------------------------------------------------------------------------------------------------
def _fill(g, cells, rng):
    """hits at the (t, c) cells, with a velocity in (0, 1] and a non-zero offset; +0 everywhere else (x + y can give back no -0)"""
    for t, c in cells:
        g[t, c] = 1.0
        g[t, 9 + c] = 0.05 + 0.95 * rng.rand()
        g[t, 18 + c] = (0.01 + 0.49 * rng.rand()) * (1 if rng.rand() < 0.5 else -1)


def grooves8():
    rng = np.random.RandomState(23)
    g = np.zeros((8, 32, 27), np.float32)
    _fill(g[0], [(t, c) for t in range(32) for c in range(9)], rng)           # 0: all 288 cells are events: cap = 287, the largest rank loop
    #                                                                           1: no event
    _fill(g[2], [(17, 4)], rng)                                               # 2: exactly one event: cap = 0
    _fill(g[3], [(3, 0), (31, 2)], rng)                                       # 3: exactly two events, candidates under every mask below: cap = 1
    _fill(g[4], [(0, 1), (5, 3), (9, 1), (30, 3), (31, 1)], rng)              # 4: events only in voices outside the mask 0x35: n_cand = 0 there
    _fill(g[5], [(12, 4)] + [(t, c) for t, c in zip((0, 2, 4, 6, 8, 10, 14, 20, 24, 28, 31), (1, 3, 6, 7, 8, 1, 3, 6, 7, 8, 1))], rng)
    #                                                                           5: under 0x35 one candidate among a dozen events
    for s in (6, 7):                                                          # 6, 7: ordinary, about 30 % density
        _fill(g[s], [(t, c) for t in range(32) for c in range(9) if rng.rand() < 0.3], rng)
    return g


GROOVES = grooves8()
R = 65536
# (voice_mask, ratio_lo, ratio_hi) in 1/65536ths
OPTS = {"r46": (0x1FF, 26214, 39322),                        # the reference's thres_range (0.4, 0.6), all voices
        "half": (0x1FF, R // 2, R // 2),                     # lo == hi
        "zero": (0x1FF, 0, 0),                               # k clamps up to 1
        "one": (0x1FF, R, R),                                # k = cap; x keeps at least one event
        "sub": (0x35, 26214, 39322),                         # voices {0, 2, 4, 5}
        "sub_one": (0x35, R, R)}                             # every candidate goes wherever another voice keeps a hit: k = n_cand, no ranking
ELIGIBLE = {"r46": [0, 3, 4, 5, 6, 7], "half": [0, 3, 4, 5, 6, 7], "zero": [0, 3, 4, 5, 6, 7], "one": [0, 3, 4, 5, 6, 7], "sub": [0, 3, 5, 6, 7],
            "sub_one": [0, 3, 5, 6, 7]}
IDX = {1: [0], 3: [3, 2, 4], 5: [6, -2, 5, 6, 40], 8: list(range(8))}      # 5: a duplicate, a negative and a too-large entry
STATES = [(1234, 99, 3), (1234, 99, 4), (77, 5, 3)]          # (seed_lo, seed_hi, step): two steps, two seeds
CELLS_SENTINEL = 0xDEADBEEF


def backend_of(name):
    """(library, buffer class) of "emu" | "hip\""""
    return (emu_lib(), NpBuf) if name == "emu" else (_lib.get_lib(), CudaBuf)


def opts_struct(o):
    return _lib.GtInfillEventOpts(o[0], o[1], o[2])


def state_buf(Buf, seed_lo, seed_hi, step):
    st = _lib.GtStepState(seed_lo, seed_hi, step, 0, 0.05, 1.0, 0.9, 0.999, 1e-8)
    return Buf(np.frombuffer(bytes(st), dtype=np.uint8).copy())


def cells_buf(Buf, B):
    """B x 9 words that all hold the sentinel (as int32: the type every buffer class carries)"""
    return Buf(np.full((B, 9), CELLS_SENTINEL, np.uint32).view(np.int32))


def run_gather(lib, Buf, hvo, idx, eo, state, want_cells=True, fill=None):
    """-> rc, x, y, cells (numpy; x / y start as `fill`, cells as the sentinel)"""
    B = int(idx.numpy().shape[0])
    x = Buf(np.full((B, 32, 27), 0.0 if fill is None else fill, np.float32))
    y = Buf(np.full((B, 32, 27), 0.0 if fill is None else fill, np.float32))
    cells = cells_buf(Buf, B)
    rc = lib.cdll.gt_gather_infill_events(hvo.ptr, idx.ptr, ctypes.c_int64(hvo.numpy().shape[0]), B, ctypes.byref(eo), state.ptr, x.ptr, y.ptr,
                                          cells.ptr if want_cells else None, None)
    return rc, x.numpy(), y.numpy(), cells.numpy().view(np.uint32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def popcount(words):
    return sum(bin(int(w)).count("1") for w in words)


def removed_cells(words):
    return {t * 9 + c for c in range(9) for t in range(32) if int(words[c]) >> t & 1}


# ---- the checks (backend = "emu" | "hip") -----------------------------------------------------------------------------------------------------
def check_gather(backend, optname, B, state):
    lib, Buf = backend_of(backend)
    o = OPTS[optname]
    idx = IDX[B]
    hvo, ix, st = Buf(GROOVES.copy()), Buf(np.array(idx, np.int64)), state_buf(Buf, *state)
    st0 = st.numpy().copy()
    rc, x, y, cells = run_gather(lib, Buf, hvo, ix, opts_struct(o), st, fill=7.25)
    assert rc == 0, lib.cdll.gt_last_error()
    wx, wy, wcells = ref.gather_infill_events(GROOVES, idx, o, *state)
    assert np.array_equal(cells, wcells), (cells, wcells)
    assert np.array_equal(bits(x), bits(wx)) and np.array_equal(bits(y), bits(wy))
    # nothing but the outputs changed
    assert np.array_equal(bits(hvo.numpy()), bits(GROOVES)) and np.array_equal(ix.numpy(), np.array(idx, np.int64)) and np.array_equal(st.numpy(), st0)
    # invariants, on the device output itself
    clamped = np.clip(idx, 0, len(GROOVES) - 1)
    src = GROOVES[clamped]
    assert np.array_equal(bits(x + y), bits(src))
    key = ref.events_key(*state)
    for b in range(len(idx)):
        n_ev, n_cand, cap = ref.count(src[b], o)
        k = ref.size(src[b], int(clamped[b]), key, o)
        assert popcount(cells[b]) == k
        _, cand = ref.flags(src[b], o[0])
        assert all(cand[j] for j in removed_cells(cells[b]))                # every removed cell is a candidate
        if cap < 1:                                                         # ineligible: untouched, nothing removed
            assert k == 0 and not cells[b].any() and not y[b].any() and np.array_equal(bits(x[b]), bits(src[b]))
        else:
            assert 1 <= k <= cap and (x[b][:, :9] != 0).sum() == n_ev - k >= 1 and (y[b][:, :9] != 0).sum() == k
            if optname == "zero":
                assert k == 1
            if optname in ("one", "sub_one"):
                assert k == cap
    dup = [b for b in range(len(idx)) if idx[b] == 6]
    if len(dup) == 2:                                                       # the same source twice in one call: the same draw
        assert np.array_equal(cells[dup[0]], cells[dup[1]]) and np.array_equal(bits(x[dup[0]]), bits(x[dup[1]]))
    return cells


def check_without_cells(backend):
    lib, Buf = backend_of(backend)
    rc, x, y, cells = run_gather(lib, Buf, Buf(GROOVES), Buf(np.array(IDX[5], np.int64)), opts_struct(OPTS["sub"]), state_buf(Buf, *STATES[0]),
                                 want_cells=False)
    assert rc == 0
    wx, wy, _ = ref.gather_infill_events(GROOVES, IDX[5], OPTS["sub"], *STATES[0])
    assert np.array_equal(bits(x), bits(wx)) and np.array_equal(bits(y), bits(wy)) and (cells == CELLS_SENTINEL).all()


REJECTED = {
    "null_set": dict(null="hvo"), "null_idx": dict(null="idx"), "null_eo": dict(null="eo"), "null_state": dict(null="state"),
    "null_x": dict(null="x"), "null_y": dict(null="y"), "batch_0": dict(batch=0), "batch_neg": dict(batch=-1), "n_seq_0": dict(n_seq=0),
    "n_seq_neg": dict(n_seq=-3), "mask_0": dict(o=(0, 0, R)), "mask_bit9": dict(o=(1 << 9 | 4, 0, R)), "mask_neg": dict(o=(-1, 0, R)),
    "lo_neg": dict(o=(0x1FF, -1, R)), "hi_big": dict(o=(0x1FF, 0, R + 1)), "lo_gt_hi": dict(o=(0x1FF, 40000, 30000)),
    "both_big": dict(o=(0x1FF, R + 1, R + 2)), "both_neg": dict(o=(0x1FF, -5, -2)),
}


def check_rejected(backend, case):
    lib, Buf = backend_of(backend)
    kw = REJECTED[case]
    B = 3
    bufs = dict(hvo=Buf(GROOVES), idx=Buf(np.array(IDX[3], np.int64)), state=state_buf(Buf, *STATES[0]),
                x=Buf(np.full((B, 32, 27), 7.25, np.float32)), y=Buf(np.full((B, 32, 27), 7.25, np.float32)))
    cells = cells_buf(Buf, B)
    eo = opts_struct(kw.get("o", OPTS["r46"]))
    p = {k: (None if kw.get("null") == k else v.ptr) for k, v in bufs.items()}
    rc = lib.cdll.gt_gather_infill_events(p["hvo"], p["idx"], ctypes.c_int64(kw.get("n_seq", 8)), kw.get("batch", B),
                                          None if kw.get("null") == "eo" else ctypes.byref(eo), p["state"], p["x"], p["y"], cells.ptr, None)
    assert rc < 0 and b"gt_gather_infill_events" in lib.cdll.gt_last_error()
    assert (bufs["x"].numpy() == 7.25).all() and (bufs["y"].numpy() == 7.25).all() and (cells.numpy().view(np.uint32) == CELLS_SENTINEL).all()


def merge_case():
    """2 sequences: in = a groove with hits removed, pred = hits scattered over every voice (also where the input has one, and outside the
    removed cells)"""
    idx = [6, 7]
    x, y, cells = ref.gather_infill_events(GROOVES, idx, OPTS["r46"], *STATES[0])
    rng = np.random.RandomState(5)
    h = (rng.rand(2, 32, 9) < 0.5).astype(np.float32)
    pred = np.concatenate([h, (0.1 + rng.rand(2, 32, 9)) * h, np.where(h != 0, rng.rand(2, 32, 9) - 0.5, 0.0)], -1).astype(np.float32)
    inside = np.array([[[bool(int(cells[s][c]) >> t & 1) for c in range(9)] for t in range(32)] for s in range(2)])
    ih, ph = x[..., :9] != 0, h != 0
    assert (ih & ph).any() and (ih & ~ph).any() and (ph & ~inside).any() and (ph & inside).any() and (~ph & inside).any()      # every kind of cell
    return pred, x, cells, inside


def run_merge(lib, Buf, pred, inp, cells, mode, alias=False):
    n = pred.shape[0]
    p, i = Buf(pred.copy()), Buf(inp)                                       # (a host buffer shares memory with the array it was made from)
    out = p if alias else Buf(np.full(pred.shape, 7.25, np.float32))
    c = Buf(np.ascontiguousarray(cells, np.uint32).view(np.int32)) if cells is not None else None
    rc = lib.cdll.gt_infill_merge_cells(p.ptr, i.ptr, c.ptr if c is not None else None, ctypes.c_int64(n), mode, out.ptr, None)
    return rc, out.numpy(), p.numpy()


def check_merge(backend, mode, masked, alias):
    lib, Buf = backend_of(backend)
    pred, inp, cells, inside = merge_case()
    rc, out, p_after = run_merge(lib, Buf, pred, inp, cells if masked else None, mode, alias)
    assert rc == 0, lib.cdll.gt_last_error()
    want = ref.merge_cells(pred, inp, cells if masked else None, mode)
    assert np.array_equal(bits(out), bits(want))
    if not alias:
        assert np.array_equal(bits(p_after), bits(pred))                    # the prediction is only read
    hit = inp[..., :9] != 0
    assert np.array_equal(out[..., :9][hit], inp[..., :9][hit])             # the input's hits are all preserved
    if masked:
        assert np.array_equal(out[..., :9][~inside], inp[..., :9][~inside])  # nothing is filled outside the removed cells
    else:                                                                   # cells = NULL is gt_infill_merge(removed = NULL), bit for bit
        p, i = Buf(pred.copy()), Buf(inp)
        o2 = Buf(np.full(pred.shape, 7.25, np.float32))
        assert lib.cdll.gt_infill_merge(p.ptr, i.ptr, None, ctypes.c_int64(pred.shape[0]), mode, o2.ptr, None) == 0
        assert np.array_equal(bits(out), bits(o2.numpy()))


def check_round_trip(backend):
    """merge(pred = y, in = x, cells) gives back the source groove in both modes, eligible or not"""
    lib, Buf = backend_of(backend)
    idx = IDX[8]
    rc, x, y, cells = run_gather(lib, Buf, Buf(GROOVES), Buf(np.array(idx, np.int64)), opts_struct(OPTS["sub"]), state_buf(Buf, *STATES[2]))
    assert rc == 0 and cells.any(1).tolist() == [i in ELIGIBLE["sub"] for i in idx]
    for mode in (0, 1):
        rc, out, _ = run_merge(lib, Buf, y, x, cells, mode)
        assert rc == 0 and np.array_equal(bits(out), bits(GROOVES)), mode


MERGE_REJECTED = {"null_pred": dict(null="pred"), "null_in": dict(null="in"), "null_out": dict(null="out"), "n_seq_0": dict(n=0),
                  "n_seq_neg": dict(n=-2), "n_seq_2p26": dict(n=1 << 26), "mode_2": dict(mode=2), "mode_neg": dict(mode=-1)}


def check_merge_rejected(backend, case):
    lib, Buf = backend_of(backend)
    kw = MERGE_REJECTED[case]
    pred, inp, cells, _ = merge_case()
    b = {"pred": Buf(pred), "in": Buf(inp), "out": Buf(np.full(pred.shape, 7.25, np.float32))}
    p = {k: (None if kw.get("null") == k else v.ptr) for k, v in b.items()}
    for c in (Buf(cells.view(np.int32)), None):                             # with a mask and with cells = NULL
        rc = lib.cdll.gt_infill_merge_cells(p["pred"], p["in"], c.ptr if c is not None else None, ctypes.c_int64(kw.get("n", 2)), kw.get("mode", 1),
                                            p["out"], None)
        assert rc < 0 and b"gt_infill_merge_cells" in lib.cdll.gt_last_error()
        assert (b["out"].numpy() == 7.25).all() and np.array_equal(b["pred"].numpy(), pred)


# ---- the emulator runs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES, ids=["s3", "s4", "seed2"])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("optname", list(OPTS))
def test_gather_events_against_restatement(optname, B, state):
    check_gather("emu", optname, B, state)


@pytest.mark.parametrize("optname", list(OPTS))
def test_gather_events_every_groove_in_one_batch(optname):
    cells = check_gather("emu", optname, 8, STATES[0])
    assert np.nonzero(cells.any(1))[0].tolist() == ELIGIBLE[optname]


def test_cells_may_be_null():
    check_without_cells("emu")


def test_the_two_steps_and_the_two_seeds_draw_differently():
    """(the inputs of the RNG cases tell a working step / seed dependence from a constant draw)"""
    for optname in ("r46", "sub"):
        m = [ref.gather_infill_events(GROOVES, IDX[8], OPTS[optname], *s)[2] for s in STATES]
        assert (m[0] != m[1]).any() and (m[0] != m[2]).any()


@pytest.mark.parametrize("case", list(REJECTED))
def test_gather_events_rejected_before_any_launch(case):
    check_rejected("emu", case)


@pytest.mark.parametrize("alias", [False, True], ids=["out", "alias"])
@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("mode", [0, 1])
def test_merge_cells_against_restatement(mode, masked, alias):
    check_merge("emu", mode, masked, alias)


def test_round_trip_gives_back_the_groove():
    check_round_trip("emu")


@pytest.mark.parametrize("case", list(MERGE_REJECTED))
def test_merge_cells_rejected_before_any_launch(case):
    check_merge_rejected("emu", case)


def test_share_of_the_specified_draw():
    """The specification, not the kernel: over 4000 source indices of the all-events groove at ratio (0.4, 0.6) every k lies in
    round(0.4 * 288) .. round(0.6 * 288), both ends' neighbourhoods are reached, and the mean share is 0.5 within 4 standard errors of a
    uniform share on [0.4, 0.6] (sigma = 0.2 / sqrt(12))."""
    o = OPTS["r46"]
    key = ref.events_key(1234, 99, 0)
    k = np.array([ref.size(GROOVES[0], src, key, o) for src in range(4000)])
    assert k.min() >= 115 and k.max() <= 173 and k.min() <= 117 and k.max() >= 171
    assert abs(k.mean() / 288 - 0.5) <= 4 * (0.2 / np.sqrt(12)) / np.sqrt(4000) + 0.5 / 288      # (+ the rounding of k to a whole cell)


# ---- host side -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optname", list(OPTS))
def test_events_eligible_agrees_with_the_kernel(optname):
    import torch
    from transformergrooveinfilling_amd import infill
    lib, Buf = backend_of("emu")
    o = OPTS[optname]
    rc, _, _, cells = run_gather(lib, Buf, Buf(GROOVES), Buf(np.arange(8, dtype=np.int64)), opts_struct(o), state_buf(Buf, *STATES[0]))
    assert rc == 0
    got = infill.events_eligible(torch.from_numpy(GROOVES), opts_struct(o)).tolist()
    assert got == np.nonzero(cells.any(1))[0].tolist() == ref.eligible(GROOVES, o).tolist() == ELIGIBLE[optname]
    voices = [c for c in range(9) if o[0] >> c & 1]
    assert infill.events_eligible(torch.from_numpy(GROOVES), dict(mode="events", voices=voices, ratio=(o[1] / R, o[2] / R))).tolist() == got
    assert infill.eligible(torch.from_numpy(GROOVES), _lib.infill_event_opts_tuple(opts_struct(o))).tolist() == got
    with pytest.raises(ValueError):
        infill.events_eligible(torch.from_numpy(GROOVES), dict(voices=[2]))            # (voice options)
    with pytest.raises(ValueError):
        infill.infill_eligible(torch.from_numpy(GROOVES), opts_struct(o))


def test_make_infill_event_opts_rounds_and_refuses():
    t = _lib.infill_event_opts_tuple
    assert ctypes.sizeof(_lib.GtInfillEventOpts) == 12
    assert t(_lib.make_infill_event_opts()) == ("events", 0x1FF, 26214, 39322)          # 0.4 * 65536 = 26214.4, 0.6 * 65536 = 39321.6
    assert t(_lib.make_infill_event_opts(voices=[0, 2, 4, 5], ratio=(0.5, 0.5))) == ("events", 0x35, 32768, 32768)
    assert t(_lib.make_infill_event_opts(voices=2, ratio=(0, 1))) == ("events", 4, 0, 65536)
    assert t(_lib.make_infill_event_opts(ratio=(0.00001, 0.999999))) == ("events", 0x1FF, 1, 65536)
    assert t(_lib.infill_event_opts_struct(("events", 0x35, 7, 9))) == ("events", 0x35, 7, 9)
    for kw in (dict(voices=[]), dict(voices=[9]), dict(voices=[-1]), dict(ratio=(0.6, 0.4)), dict(ratio=(-0.1, 0.5)), dict(ratio=(0.5, 1.1)),
               dict(ratio=(0.1, 0.2, 0.3)), dict(ratio=(float("nan"), 0.5)), dict(ratio=(0.1, float("inf")))):
        with pytest.raises(ValueError):
            _lib.make_infill_event_opts(**kw)
    for bad in (("events", 0, 0, 1), ("events", 0x200, 0, 1), ("events", 1, 2, 1), ("events", 1, 0, 65537), ("events", 1, 0.5, 1), (1, 2, 3, 4)):
        with pytest.raises(ValueError):
            _lib.infill_event_opts_struct(bad)


def test_as_opts_keeps_the_voice_options_and_takes_the_event_options():
    from transformergrooveinfilling_amd import infill
    v = _lib.make_infill_opts(voices=[2, 4], min_remove=1, max_remove=2, prob=[3, 1])
    vt = _lib.infill_opts_tuple(v)
    assert infill.as_opts(v) is v
    for given in (vt, dict(voices=[2, 4], min_remove=1, max_remove=2, prob=[3, 1]), dict(mode="voices", voices=[2, 4], max_remove=2, prob=[3, 1])):
        got = infill.as_opts(given)
        assert isinstance(got, _lib.GtInfillOpts) and _lib.infill_opts_tuple(got) == vt
    assert _lib.infill_opts_tuple(infill.as_opts({})) == _lib.infill_opts_tuple(_lib.make_infill_opts())
    e = _lib.make_infill_event_opts(voices=[0, 2], ratio=(0.25, 0.75))
    et = _lib.infill_event_opts_tuple(e)
    assert infill.as_opts(e) is e and et == ("events", 5, 16384, 49152)
    for given in (et, dict(mode="events", voices=[0, 2], ratio=(0.25, 0.75))):
        got = infill.as_opts(given)
        assert isinstance(got, _lib.GtInfillEventOpts) and _lib.infill_event_opts_tuple(got) == et
    assert infill.opts_tuple(e) == et and infill.opts_tuple(v) == vt
    for bad in ((1, 2, 3), "events", None, ("events", 5, 1), dict(mode="cells")):
        with pytest.raises(ValueError):
            infill.as_opts(bad)


def test_merge_takes_words_or_bools_and_not_both_masks():
    import torch
    from transformergrooveinfilling_amd import infill
    lib = emu_lib()
    pred, inp, cells, inside = merge_case()
    want = ref.merge_cells(pred, inp, cells, 1)
    tp, ti = torch.from_numpy(pred), torch.from_numpy(inp)
    for given in (torch.from_numpy(cells.view(np.int32)), torch.from_numpy(inside), cells.view(np.int32)):
        assert np.array_equal(bits(infill.merge(tp, ti, cells=given, lib=lib).numpy()), bits(want))
    if hasattr(torch, "uint32"):
        assert np.array_equal(bits(infill.merge(tp, ti, cells=torch.from_numpy(cells.view(np.int32)).view(torch.uint32), lib=lib).numpy()), bits(want))
    assert np.array_equal(bits(infill.merge(tp, ti, lib=lib).numpy()), bits(ref.merge_cells(pred, inp, None, 1)))
    top = torch.zeros(2, 32, 9, dtype=torch.bool)
    top[:, 31, :] = True                                                    # (bit 31: the word is negative as int32)
    assert infill.cell_words(top, 2, "cpu").tolist() == [[-(1 << 31)] * 9] * 2
    with pytest.raises(ValueError):
        infill.merge(tp, ti, removed=torch.tensor([1, 2], dtype=torch.int32), cells=torch.from_numpy(inside), lib=lib)
    for bad in (torch.zeros(2, 9), torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 9, 32, dtype=torch.bool)):
        with pytest.raises(ValueError):
            infill.merge(tp, ti, cells=bad, lib=lib)


@pytest.mark.parametrize("optname", ["r46", "sub"])
def test_loader_event_form_permutes_the_eligible_pool(optname):
    import torch
    from transformergrooveinfilling_amd import parallel
    o = OPTS[optname]
    ld = parallel.DeviceBatchLoader.infilling(GROOVES, opts_struct(o), 2, "cpu", seed=3, lib=emu_lib())
    assert isinstance(ld.infill_opts, _lib.GtInfillEventOpts)
    assert ld.n == len(ELIGIBLE[optname]) and len(ld) == (ld.n + 1) // 2
    seen = []
    for ep in range(3):
        ld.set_epoch(ep)
        got = torch.cat(list(ld.index_batches())).tolist()
        assert sorted(got) == ELIGIBLE[optname]                                # a permutation of the eligible grooves, nothing else
        seen.append(got)
    assert seen[0] != seen[1] or seen[0] != seen[2]
    n = 0
    for x, y, idx in ld:                                                       # iteration: the pairs drawn by gt_gather_infill_events
        assert set(idx.tolist()) <= set(ELIGIBLE[optname])
        assert torch.equal(x + y, torch.from_numpy(GROOVES)[idx])
        assert all(bool(y[b].any()) and bool(x[b].any()) for b in range(len(idx)))
        n += len(idx)
    assert n == ld.n
    by_dict = parallel.DeviceBatchLoader.infilling(GROOVES, dict(mode="events", voices=[c for c in range(9) if o[0] >> c & 1]), 2, "cpu")
    assert by_dict.pool.tolist() == ELIGIBLE[optname]
    with pytest.raises(ValueError):
        parallel.DeviceBatchLoader.infilling(GROOVES[[1, 2]], opts_struct(o), 2, "cpu")


def _train_py():
    sys.path.insert(0, ROOT)
    import train
    return train


def test_train_py_parses_the_event_flags():
    train = _train_py()
    parse = lambda argv: train.load_hyperparameters(train.build_parser().parse_args(argv))
    base = ["--experiment", "InfillingRandom_Symbolic", "--infill-npz", "g.npz"]
    hp = parse(base + ["--infill_mode", "events", "--infill_ratio", "0.4,0.6"])
    assert hp["infill_npz"] == "g.npz" and hp["infill"] == dict(mode="events", voices=list(range(9)), ratio=[0.4, 0.6])
    from transformergrooveinfilling_amd import infill
    assert infill.opts_tuple(infill.as_opts(hp["infill"])) == ("events", 0x1FF, 26214, 39322)
    assert train.model_params(hp, "cpu")["model"]["embedding_size_src"] == 27
    hp = parse(base + ["--infill_mode", "events", "--infill_voices", "0,2,4,5", "--infill_ratio", "0.25,0.5"])
    assert hp["infill"] == dict(mode="events", voices=[0, 2, 4, 5], ratio=[0.25, 0.5])
    assert parse(base + ["--infill_mode", "events"])["infill"]["ratio"] == [0.4, 0.6]                  # the reference's thres_range
    for argv in (base, base + ["--infill_mode", "voices"]):                                            # the default mode: today's options
        assert parse(argv)["infill"] == dict(voices=[2], min_remove=1, max_remove=1, prob=None)
    assert parse(["--experiment", "InfillingRandom_Symbolic"])["infill"] is None


def test_train_py_reads_the_event_yaml_keys(tmp_path):
    train = _train_py()
    cfg = tmp_path / "c.yaml"
    cfg.write_text("experiment: InfillingRandom_Symbolic\ninfill_npz: grooves.npz\ninfill_mode: events\ninfill_voices: [0, 2]\n"
                   "infill_ratio: [0.3, 0.5]\n")
    hp = train.load_hyperparameters(train.build_parser().parse_args(["--config", str(cfg)]))
    assert hp["infill_npz"] == "grooves.npz" and hp["infill"] == dict(mode="events", voices=[0, 2], ratio=[0.3, 0.5])
    cfg.write_text("experiment: InfillingRandom_Symbolic\ninfill_npz: grooves.npz\ninfill_mode: events\ninfill_ratio: '0.4,0.6'\n")
    hp = train.load_hyperparameters(train.build_parser().parse_args(["--config", str(cfg)]))
    assert hp["infill"] == dict(mode="events", voices=list(range(9)), ratio=[0.4, 0.6])


@pytest.mark.parametrize("argv, why", [
    (["--experiment", "InfillingRandom", "--infill-npz", "g.npz", "--infill_mode", "events"], "symbolic"),
    (["--experiment", "InfillingRandom", "--infill_mode", "events"], "symbolic"),
    (["--experiment", "InfillingRandom_Symbolic", "--infill_mode", "events"], "need --infill-npz"),
    (["--experiment", "InfillingRandom_Symbolic", "--infill-npz", "g.npz", "--infill_mode", "events", "--infill_min", "1"], "infill_ratio"),
    (["--experiment", "InfillingRandom_Symbolic", "--infill-npz", "g.npz", "--infill_mode", "events", "--infill_prob", "1"], "infill_ratio"),
    (["--experiment", "InfillingRandom_Symbolic", "--infill-npz", "g.npz", "--infill_ratio", "0.4,0.6"], "infill_mode events"),
    (["--experiment", "InfillingRandom_Symbolic", "--infill-npz", "g.npz", "--infill_mode", "events", "--infill_ratio", "0.6,0.4"], "infill options"),
    (["--experiment", "InfillingRandom_Symbolic", "--infill-npz", "g.npz", "--infill_mode", "events", "--infill_ratio", "0.5"], "comma-separated floats"),
    (["--experiment", "InfillingRandom_Symbolic", "--infill-npz", "g.npz", "--infill_mode", "events", "--infill_ratio", "a,b"], "comma-separated floats"),
    (["--experiment", "InfillingRandom_Symbolic", "--infill-npz", "g.npz", "--infill_mode", "events", "--infill_voices", "9"], "infill options")])
def test_train_py_refuses_bad_event_flags(argv, why):
    train = _train_py()
    args = train.build_parser().parse_args(argv)                    # (the flags themselves parse: the refusal is load_hyperparameters')
    with pytest.raises(SystemExit, match=why):
        train.load_hyperparameters(args)


def test_train_py_refuses_an_unknown_infill_mode_in_a_yaml(tmp_path):
    train = _train_py()
    cfg = tmp_path / "c.yaml"
    cfg.write_text("experiment: InfillingRandom_Symbolic\ninfill_npz: grooves.npz\ninfill_mode: cells\n")
    with pytest.raises(SystemExit, match="voices or events"):
        train.load_hyperparameters(train.build_parser().parse_args(["--config", str(cfg)]))
