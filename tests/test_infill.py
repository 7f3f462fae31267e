"""Infilling pairs drawn in the gather (gt_gather_infill) and the way back (gt_infill_merge) on the host emulator build of the kernel
sources, against the restatement in tests/infill_ref.py: every comparison is exact (no tolerance enters -- the draw is integer
arithmetic, kept values are bit copies).  The check_* functions take the backend; tests/test_infill_gpu.py runs them on the HIP library.
Also the host side that needs no GPU: infill_eligible, the loader's infilling form, train.py's flags and YAML keys."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

import infill_ref as ref
from harness import CudaBuf, NpBuf, emu_lib
from transformergrooveinfilling_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the 7 hand-built grooves ---------------------------------------------------------------------------------------------------------------
ACTIVE = [(0, 1, 2, 3, 4, 5, 6, 7, 8),      # 0: every voice active
          (2,),                            # 1: one voice active: nothing can be removed without emptying the input
          (1, 3),                          # 2: no candidate voice of any option set below but "all" is active
          (),                              # 3: all hits zero
          (0, 2),                          # 4: candidates are the only active voices: n_tot - 1 caps the size
          (0, 1, 2, 4, 7),                 # 5, 6: ordinary
          (2, 3, 5, 6, 8)]


def grooves7():
    rng = np.random.RandomState(11)
    g = np.zeros((len(ACTIVE), 32, 27), np.float32)
    for s, voices in enumerate(ACTIVE):
        for c in voices:
            h = rng.rand(32) < 0.3
            h[rng.randint(32)] = True                      # (an active voice has at least one hit)
            g[s, :, c] = h
            g[s, :, 9 + c] = (0.05 + 0.95 * rng.rand(32)) * h
            g[s, :, 18 + c] = np.where(h, rng.rand(32) - 0.5, 0.0)      # (+0 where there is no hit: x + y can give back no -0)
    return g


GROOVES = grooves7()
# (voice_mask, min_remove, max_remove, weights)
OPTS = {"closed_hh": (1 << 2, 1, 1, [1]),                   # the ClosedHH case: single voice {2}
        "all_1_9": (0x1FF, 1, 9, [1] * 9),
        "w010": (0x35, 1, 3, [0, 1, 0]),                    # voices {0, 2, 4, 5}; size 1 and 3 never drawn: groove 4 (hi = 1) becomes ineligible
        "w112": (0x35, 1, 3, [1, 1, 2])}
ELIGIBLE = {"closed_hh": [0, 4, 5, 6], "all_1_9": [0, 2, 4, 5, 6], "w010": [0, 5, 6], "w112": [0, 4, 5, 6]}
IDX = {1: [0], 3: [4, 1, 6], 5: [5, -2, 3, 5, 40], 7: list(range(7))}      # 5: a duplicate, a negative and a too-large entry
STATES = [(1234, 99, 3), (1234, 99, 4), (77, 5, 3)]         # (seed_lo, seed_hi, step): two steps, two seeds


def backend_of(name):
    """(library, buffer class) of "emu" | "hip\""""
    return (emu_lib(), NpBuf) if name == "emu" else (_lib.get_lib(), CudaBuf)


def opts_struct(o):
    return _lib.GtInfillOpts(o[0], o[1], o[2], (ctypes.c_int32 * 9)(*(list(o[3]) + [0] * (9 - len(o[3])))))


def state_buf(Buf, seed_lo, seed_hi, step):
    st = _lib.GtStepState(seed_lo, seed_hi, step, 0, 0.05, 1.0, 0.9, 0.999, 1e-8)
    return Buf(np.frombuffer(bytes(st), dtype=np.uint8).copy())


def run_gather(lib, Buf, hvo, idx, io, state, want_removed=True, fill=None):
    """-> rc, x, y, removed (numpy; outputs start as `fill` / -7 sentinels when given)"""
    B = int(idx.numpy().shape[0])
    x = Buf(np.full((B, 32, 27), 0.0 if fill is None else fill, np.float32))
    y = Buf(np.full((B, 32, 27), 0.0 if fill is None else fill, np.float32))
    rem = Buf(np.full(B, -7, np.int32))
    rc = lib.cdll.gt_gather_infill(hvo.ptr, idx.ptr, ctypes.c_int64(hvo.numpy().shape[0]), B, ctypes.byref(io), state.ptr, x.ptr, y.ptr,
                                   rem.ptr if want_removed else None, None)
    return rc, x.numpy(), y.numpy(), rem.numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def popcount(m):
    return bin(int(m)).count("1")


# ---- the checks (backend = "emu" | "hip") -----------------------------------------------------------------------------------------------------
def check_gather(backend, optname, B, state):
    lib, Buf = backend_of(backend)
    o = OPTS[optname]
    idx = IDX[B]
    rc, x, y, rem = run_gather(lib, Buf, Buf(GROOVES), Buf(np.array(idx, np.int64)), opts_struct(o), state_buf(Buf, *state), fill=7.25)
    assert rc == 0, lib.cdll.gt_last_error()
    wx, wy, wrem = ref.gather_infill(GROOVES, idx, o, *state)
    assert np.array_equal(rem, wrem), (rem, wrem)
    assert np.array_equal(bits(x), bits(wx)) and np.array_equal(bits(y), bits(wy))
    # invariants, on the device output itself
    src = GROOVES[np.clip(idx, 0, len(GROOVES) - 1)]
    assert np.array_equal(bits(x + y), bits(src))
    for b in range(len(idx)):
        vx = {c for c in range(9) if (x[b][:, [c, 9 + c, 18 + c]] != 0).any()}
        vy = {c for c in range(9) if (y[b][:, [c, 9 + c, 18 + c]] != 0).any()}
        assert not vx & vy
        act = ref.active_mask(src[b])
        assert rem[b] & ~(o[0] & act) == 0                                  # removed is a subset of voice_mask and of the active voices
        assert vy == {c for c in range(9) if rem[b] >> c & 1}
        _, hi, W = ref.size_weights(act, o)
        if sum(W.values()) == 0:
            assert rem[b] == 0 and not y[b].any()                           # ineligible: nothing removed
        else:
            assert o[1] <= popcount(rem[b]) <= hi
    dup = [b for b in range(len(idx)) if idx[b] == 5]
    if len(dup) == 2:                                                       # the same source twice in one call: the same draw
        assert rem[dup[0]] == rem[dup[1]] and np.array_equal(x[dup[0]], x[dup[1]])
    return rem


def check_without_removed(backend):
    lib, Buf = backend_of(backend)
    rc, x, y, rem = run_gather(lib, Buf, Buf(GROOVES), Buf(np.array(IDX[3], np.int64)), opts_struct(OPTS["w112"]), state_buf(Buf, *STATES[0]),
                               want_removed=False)
    assert rc == 0
    wx, wy, _ = ref.gather_infill(GROOVES, IDX[3], OPTS["w112"], *STATES[0])
    assert np.array_equal(bits(x), bits(wx)) and np.array_equal(bits(y), bits(wy)) and (rem == -7).all()


REJECTED = {
    "null_set": dict(null="hvo"), "null_idx": dict(null="idx"), "null_io": dict(null="io"), "null_state": dict(null="state"),
    "null_x": dict(null="x"), "null_y": dict(null="y"), "batch_0": dict(batch=0), "batch_neg": dict(batch=-1), "n_seq_0": dict(n_seq=0),
    "mask_0": dict(o=(0, 1, 1, [1])), "mask_bit9": dict(o=(1 << 9 | 4, 1, 1, [1])), "mask_neg": dict(o=(-1, 1, 1, [1])),
    "min_0": dict(o=(4, 0, 1, [1, 1])), "max_lt_min": dict(o=(0x1FF, 3, 2, [1])), "max_10": dict(o=(0x1FF, 1, 10, [1] * 9)),
    "weight_neg": dict(o=(0x1FF, 1, 2, [1, -1])), "weight_big": dict(o=(0x1FF, 1, 2, [1025, 1])), "weights_0": dict(o=(0x1FF, 1, 3, [0, 0, 0, 5])),
}


def check_rejected(backend, case):
    lib, Buf = backend_of(backend)
    kw = REJECTED[case]
    B = 3
    bufs = dict(hvo=Buf(GROOVES), idx=Buf(np.array(IDX[3], np.int64)), state=state_buf(Buf, *STATES[0]),
                x=Buf(np.full((B, 32, 27), 7.25, np.float32)), y=Buf(np.full((B, 32, 27), 7.25, np.float32)))
    rem = Buf(np.full(B, -7, np.int32))
    io = opts_struct(kw.get("o", OPTS["w112"]))
    p = {k: (None if kw.get("null") == k else v.ptr) for k, v in bufs.items()}
    rc = lib.cdll.gt_gather_infill(p["hvo"], p["idx"], ctypes.c_int64(kw.get("n_seq", 7)), kw.get("batch", B),
                                   None if kw.get("null") == "io" else ctypes.byref(io), p["state"], p["x"], p["y"], rem.ptr, None)
    assert rc < 0 and b"gt_gather_infill" in lib.cdll.gt_last_error()
    assert (bufs["x"].numpy() == 7.25).all() and (bufs["y"].numpy() == 7.25).all() and (rem.numpy() == -7).all()


def merge_case():
    """2 sequences: in = a groove with voices removed, pred = hits in every voice (also where the input has one, and outside the mask)"""
    idx = [0, 5]
    x, y, rem = ref.gather_infill(GROOVES, idx, OPTS["w112"], *STATES[0])
    rng = np.random.RandomState(5)
    h = (rng.rand(2, 32, 9) < 0.4).astype(np.float32)
    pred = np.concatenate([h, (0.1 + rng.rand(2, 32, 9)) * h, np.where(h != 0, rng.rand(2, 32, 9) - 0.5, 0.0)], -1).astype(np.float32)
    inside = np.array([[bool(m >> c & 1) for c in range(9)] for m in rem])[:, None, :]
    ih, ph = x[..., :9] != 0, h != 0
    assert (rem != 0).all() and (rem != 0x1FF).all()
    assert (ih & ph).any() and (ih & ~ph).any() and (ph & ~inside).any() and (ph & inside).any()      # every kind of cell is there
    return pred, x, rem, GROOVES[idx], y


def run_merge(lib, Buf, pred, inp, rem, mode, alias=False):
    n = pred.shape[0]
    p, i = Buf(pred.copy()), Buf(inp)                                       # (a host buffer shares memory with the array it was made from)
    out = p if alias else Buf(np.full(pred.shape, 7.25, np.float32))
    r = Buf(np.asarray(rem, np.int32)) if rem is not None else None
    rc = lib.cdll.gt_infill_merge(p.ptr, i.ptr, r.ptr if r is not None else None, ctypes.c_int64(n), mode, out.ptr, None)
    return rc, out.numpy(), p.numpy()


def check_merge(backend, mode, masked, alias):
    lib, Buf = backend_of(backend)
    pred, inp, rem, _, _ = merge_case()
    rc, out, p_after = run_merge(lib, Buf, pred, inp, rem if masked else None, mode, alias)
    assert rc == 0, lib.cdll.gt_last_error()
    want = ref.merge(pred, inp, rem if masked else None, mode)
    assert np.array_equal(bits(out), bits(want))
    if not alias:
        assert np.array_equal(bits(p_after), bits(pred))                    # the prediction is only read
    hit = inp[..., :9] != 0
    assert np.array_equal(out[..., :9][hit], inp[..., :9][hit])             # the input's hits are all preserved
    if masked:
        outside = ~np.array([[bool(m >> c & 1) for c in range(9)] for m in rem])[:, None, :] & np.ones((1, 32, 1), bool)
        assert np.array_equal(out[..., :9][outside], inp[..., :9][outside])  # nothing is filled outside the removed voices


def check_round_trip(backend):
    """merge(mode 1, pred = y, in = x, removed) gives back the source groove, eligible or not"""
    lib, Buf = backend_of(backend)
    idx = IDX[7]
    rc, x, y, rem = run_gather(lib, Buf, Buf(GROOVES), Buf(np.array(idx, np.int64)), opts_struct(OPTS["w112"]), state_buf(Buf, *STATES[2]))
    assert rc == 0 and (rem != 0).any() and (rem == 0).any()
    rc, out, _ = run_merge(lib, Buf, y, x, rem, 1)
    assert rc == 0 and np.array_equal(bits(out), bits(GROOVES))


MERGE_REJECTED = {"null_pred": dict(null="pred"), "null_in": dict(null="in"), "null_out": dict(null="out"), "n_seq_0": dict(n=0),
                  "n_seq_neg": dict(n=-2), "mode_2": dict(mode=2), "mode_neg": dict(mode=-1)}


def check_merge_rejected(backend, case):
    lib, Buf = backend_of(backend)
    kw = MERGE_REJECTED[case]
    pred, inp, rem, _, _ = merge_case()
    b = {"pred": Buf(pred), "in": Buf(inp), "out": Buf(np.full(pred.shape, 7.25, np.float32))}
    p = {k: (None if kw.get("null") == k else v.ptr) for k, v in b.items()}
    rc = lib.cdll.gt_infill_merge(p["pred"], p["in"], Buf(rem).ptr, ctypes.c_int64(kw.get("n", 2)), kw.get("mode", 1), p["out"], None)
    assert rc < 0 and b"gt_infill_merge" in lib.cdll.gt_last_error()
    assert (b["out"].numpy() == 7.25).all() and np.array_equal(b["pred"].numpy(), pred)


# ---- the emulator runs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES, ids=["s3", "s4", "seed2"])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("optname", list(OPTS))
def test_gather_infill_against_restatement(optname, B, state):
    check_gather("emu", optname, B, state)


def test_removed_may_be_null():
    check_without_removed("emu")


def test_the_two_steps_and_the_two_seeds_draw_differently():
    """(the inputs of the RNG cases tell a working step / seed dependence from a constant draw)"""
    for optname in ("all_1_9", "w112"):
        m = [ref.gather_infill(GROOVES, IDX[7], OPTS[optname], *s)[2] for s in STATES]
        assert (m[0] != m[1]).any() and (m[0] != m[2]).any()
    assert (ref.gather_infill(GROOVES, IDX[5], OPTS["w112"], *STATES[0])[2] != ref.gather_infill(GROOVES, IDX[5], OPTS["w112"], *STATES[1])[2]).any()


@pytest.mark.parametrize("case", list(REJECTED))
def test_gather_rejected_before_any_launch(case):
    check_rejected("emu", case)


@pytest.mark.parametrize("alias", [False, True], ids=["out", "alias"])
@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("mode", [0, 1])
def test_merge_against_restatement(mode, masked, alias):
    check_merge("emu", mode, masked, alias)


def test_round_trip_gives_back_the_groove():
    check_round_trip("emu")


@pytest.mark.parametrize("case", list(MERGE_REJECTED))
def test_merge_rejected_before_any_launch(case):
    check_merge_rejected("emu", case)


def test_restatement_hash_is_the_oracles():
    from oracle import numpy_groove as ng
    v = np.array([0, 1, 0x9E3779B1, 0xFFFFFFFF, 123456789], np.uint64)
    assert [ref.fmix32(int(a)) for a in v] == [int(a) for a in ng._fmix32(v)]


def test_distribution_of_the_specified_draw():
    """The specification, not the kernel: over 20 000 source indices of an all-voices-active groove, weights [1, 1, 2] on sizes 1..3, the size
    frequencies match W_k / T and every candidate's inclusion frequency its expectation sum_k p_k k / n_act, within 4 sigma of the binomial
    standard error."""
    o = (0x1FF, 1, 3, [1, 1, 2])
    n = 20000
    key = ref.infill_key(1234, 99, 0)
    masks = [ref.draw(0x1FF, src, key, o) for src in range(n)]
    W = {k: o[3][k - 1] * math.comb(9, k) for k in (1, 2, 3)}
    T = sum(W.values())
    sizes = np.array([popcount(m) for m in masks])
    assert set(sizes) == {1, 2, 3}
    for k in (1, 2, 3):
        p = W[k] / T
        assert abs((sizes == k).mean() - p) <= 4 * math.sqrt(p * (1 - p) / n), (k, (sizes == k).mean(), p)
    p_in = sum(W[k] / T * k / 9 for k in (1, 2, 3))
    for c in range(9):
        f = np.mean([(m >> c) & 1 for m in masks])
        assert abs(f - p_in) <= 4 * math.sqrt(p_in * (1 - p_in) / n), (c, f, p_in)


# ---- host side -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optname", list(OPTS))
def test_infill_eligible_agrees_with_the_kernel(optname):
    import torch
    from transformergrooveinfilling_amd import infill
    lib, Buf = backend_of("emu")
    rc, _, _, rem = run_gather(lib, Buf, Buf(GROOVES), Buf(np.arange(7, dtype=np.int64)), opts_struct(OPTS[optname]), state_buf(Buf, *STATES[0]))
    assert rc == 0
    got = infill.infill_eligible(torch.from_numpy(GROOVES), opts_struct(OPTS[optname])).tolist()
    assert got == np.nonzero(rem)[0].tolist() == ref.eligible(GROOVES, OPTS[optname]).tolist() == ELIGIBLE[optname]
    o = OPTS[optname]
    voices = [c for c in range(9) if o[0] >> c & 1]
    assert infill.infill_eligible(torch.from_numpy(GROOVES), dict(voices=voices, min_remove=o[1], max_remove=o[2], prob=o[3])).tolist() == got


@pytest.mark.parametrize("optname", ["closed_hh", "w010"])
def test_loader_never_yields_an_ineligible_index(optname):
    import torch
    from transformergrooveinfilling_amd import parallel
    o = OPTS[optname]
    ld = parallel.DeviceBatchLoader.infilling(GROOVES, opts_struct(o), 2, "cpu", seed=3, lib=emu_lib())
    assert ld.n == len(ELIGIBLE[optname]) and len(ld) == (ld.n + 1) // 2
    seen = []
    for ep in range(3):
        ld.set_epoch(ep)
        got = torch.cat(list(ld.index_batches())).tolist()
        assert sorted(got) == ELIGIBLE[optname]                                # a permutation of the eligible grooves, nothing else
        seen.append(got)
    assert seen[0] != seen[1] or seen[0] != seen[2]
    masks = []
    for x, y, idx in ld:                                                       # iteration: the pairs drawn by gt_gather_infill
        assert set(idx.tolist()) <= set(ELIGIBLE[optname])
        assert torch.equal(x + y, torch.from_numpy(GROOVES)[idx])
        assert all(bool(y[b].any()) and bool(x[b].any()) for b in range(len(idx)))
        masks.append(y)
    assert masks
    two = parallel.DeviceBatchLoader(GROOVES[:, :, :16], GROOVES, 2, "cpu")    # the two-tensor form: every index, as before
    assert sorted(torch.cat(list(two.index_batches())).tolist()) == list(range(7)) and two.infill_opts is None
    with pytest.raises(ValueError):
        parallel.DeviceBatchLoader.infilling(GROOVES[[1, 3]], opts_struct(o), 2, "cpu")


def _train_py():
    sys.path.insert(0, ROOT)
    import train
    return train


def test_train_py_parses_the_infill_flags():
    train = _train_py()
    args = train.build_parser().parse_args(["--experiment", "InfillingClosedHH_Symbolic", "--infill-npz", "g.npz", "--infill_voices", "2,4,5",
                                            "--infill_min", "1", "--infill_max", "3", "--infill_prob", "1,1,2"])
    hp = train.load_hyperparameters(args)
    assert hp["infill_npz"] == "g.npz" and hp["infill"] == dict(voices=[2, 4, 5], min_remove=1, max_remove=3, prob=[1, 1, 2])
    io = _lib.make_infill_opts(**hp["infill"])
    assert _lib.infill_opts_tuple(io) == (0x34, 1, 3, 1, 1, 2, 0, 0, 0, 0, 0, 0)
    hp = train.load_hyperparameters(train.build_parser().parse_args(["--experiment", "InfillingClosedHH_Symbolic", "--infill-npz", "g.npz"]))
    assert hp["infill"] == dict(voices=[2], min_remove=1, max_remove=1, prob=None)       # the ClosedHH default
    assert train.load_hyperparameters(train.build_parser().parse_args(["--experiment", "InfillingClosedHH_Symbolic"]))["infill"] is None


def test_train_py_reads_the_infill_yaml_keys(tmp_path):
    train = _train_py()
    cfg = tmp_path / "c.yaml"
    cfg.write_text("experiment: InfillingClosedHH_Symbolic\ninfill_npz: grooves.npz\ninfill_voices: [0, 2]\ninfill_min: 1\ninfill_max: 2\n"
                   "infill_prob: '3,1'\n")
    hp = train.load_hyperparameters(train.build_parser().parse_args(["--config", str(cfg)]))
    assert hp["infill_npz"] == "grooves.npz" and hp["infill"] == dict(voices=[0, 2], min_remove=1, max_remove=2, prob=[3, 1])


@pytest.mark.parametrize("argv, why", [
    (["--experiment", "InfillingClosedHH", "--infill-npz", "g.npz"], "symbolic"),
    (["--experiment", "InfillingRandom", "--infill_voices", "2"], "symbolic"),
    (["--experiment", "InfillingClosedHH_Symbolic", "--infill_voices", "2"], "need --infill-npz"),                       # no grooves
    (["--experiment", "InfillingClosedHH_Symbolic", "--infill-npz", "g.npz", "--infill_voices", "9"], "infill options"),
    (["--experiment", "InfillingClosedHH_Symbolic", "--infill-npz", "g.npz", "--infill_max", "2", "--infill_prob", "1"], "infill options"),
    (["--experiment", "InfillingClosedHH_Symbolic", "--infill-npz", "g.npz", "--infill_prob", "a"], "comma-separated integers")])
def test_train_py_refuses_bad_infill_flags(argv, why):
    train = _train_py()
    args = train.build_parser().parse_args(argv)                    # (the flags themselves parse: the refusal is load_hyperparameters')
    with pytest.raises(SystemExit, match=why):
        train.load_hyperparameters(args)


def test_train_py_refuses_infill_yaml_keys_for_a_non_symbolic_experiment(tmp_path):
    train = _train_py()
    cfg = tmp_path / "c.yaml"
    cfg.write_text("experiment: InfillingKicksAndSnares\ninfill_npz: grooves.npz\n")
    with pytest.raises(SystemExit, match="symbolic"):
        train.load_hyperparameters(train.build_parser().parse_args(["--config", str(cfg)]))


def test_make_infill_opts_refuses_what_the_library_refuses():
    for kw in (dict(voices=[]), dict(voices=[9]), dict(min_remove=0), dict(min_remove=2, max_remove=1), dict(max_remove=10),
               dict(max_remove=2, prob=[1]), dict(prob=[1025]), dict(prob=[0]), dict(prob=[1.5])):
        with pytest.raises(ValueError):
            _lib.make_infill_opts(**kw)
    assert ctypes.sizeof(_lib.GtInfillOpts) == 48
