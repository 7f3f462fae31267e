"""tests/isolation.py on the host emulator at its small shapes, and the negative controls of its three detectors (host memory: nothing can
fault).  The tile choices where the properties can really break exist on the GPU only: tests/test_isolation_gpu.py."""
import ctypes

import numpy as np
import pytest

import isolation as iso
from harness import Runner, cfg_dict
from oracle import numpy_groove as ng

D32 = cfg_dict(32, 4, 16, 1)
CASES = {"d32": (D32, 2, 0.1), "d32-encdec": (cfg_dict(32, 4, 16, 1, 1), 2, 0.1), "d48-h3-S27": (cfg_dict(48, 3, 40, 1, embedding_size_src=27), 3, 0.1)}


@pytest.mark.parametrize("case", list(CASES))
def test_fill_independence(case):
    cfg, B, p = CASES[case]
    assert iso.check_fill_independence("emu", cfg, B, p) == ["qnan", "all-ones", "+inf", "one", "prefill", "other"]
    if case == "d32":                                # the default mode (on the emulator the same arithmetic: it pins compare()'s other branch)
        iso.check_fill_independence("emu", cfg, B, p, fills=("qnan",), deterministic=False, prefill=False, other=False)


@pytest.mark.parametrize("case", list(CASES))
def test_history_independence(case):
    cfg, B, p = CASES[case]
    assert iso.check_history_independence("emu", cfg, B, p) >= 2        # ... forms ran on packs a folded update left (0 off the sequence path)


def test_history_independence_default_mode():
    cfg, B, p = CASES["d32"]
    iso.check_history_independence("emu", cfg, B, p, deterministic=False, seed=1)


@pytest.mark.parametrize("case", list(CASES))
def test_redzones(case):
    cfg, B, p = CASES[case]
    iso.check_redzones("emu", cfg, B, p)


# ---- negative controls: a detector that cannot fail these is not done ---------------------------------------------------------------------
def test_control_write_past_the_end_names_the_buffer():
    """gt_optimizer_step over one element more than the buffers hold, zero_grads = 1: the element behind grads is cleared"""
    cfg = dict(D32, dropout=0.0)
    r = Runner(cfg, 2, "emu", guard=iso.QNAN)
    r.set_params(ng.init_params(cfg, seed=3, perturb=0.05))
    assert r.redzones_intact() == []
    r.lib.call("gt_optimizer_step", 0, r.params.ptr, r.grads.ptr, None, None, ctypes.c_int64(r.total), r.state.ptr, 1, r.stream)
    assert r.redzones_intact() == []
    r.lib.call("gt_optimizer_step", 0, r.params.ptr, r.grads.ptr, None, None, ctypes.c_int64(r.total + 1), r.state.ptr, 1, r.stream)
    assert "grads" in r.redzones_intact()


def test_control_guard_keeps_a_buffers_bytes_and_alignment():
    r, g = Runner(D32, 2, "emu"), Runner(D32, 2, "emu", guard=iso.BASE, ws_fill=iso.BASE)
    for name in ("ws", "pe", "hvo", "grads", "stats", "d_hvo", "tgt", "state"):
        a, b = getattr(r, name), getattr(g, name)
        assert a.numpy().tobytes() == b.numpy().tobytes(), name
        assert b.ptr.value % 64 == b.full.ctypes.data % 64, name          # the red zone is a multiple of 256 bytes


def test_control_read_past_the_end_reaches_a_result():
    """x handed over one row short: the last token row is read from the red zone behind it, and the guard pattern shows in the results"""
    with pytest.raises(AssertionError, match="red zones of NaN against red zones of 7.25"):
        iso.check_redzones("emu", D32, 2, 0.1, forms=("eval", "step"), x_short=1)


def test_control_stale_workspace_read_is_seen():
    """the op path (no exchange region: gt_workspace_init zeroes nothing) -- a backward without its forward reads the fill"""
    with pytest.raises(AssertionError, match="workspace fill qnan against 7.25"):
        iso.check_fill_independence("emu", D32, 2, 0.1, seq=False, forms=("bare_backward",), fills=("qnan",), prefill=False, other=False)
    r = Runner(D32, 2, "emu", seq=False)
    with pytest.raises(Exception):
        r.lib.ws_find(r.c, "seq_xchg", 0)


def test_compare_bars():
    """compare(): bitwise by default; gradients within the accumulation bar only where asked, never a NaN, never the forward side"""
    a = {"f.grads": np.array([1.0, 0.5], np.float32), "f.hvo": np.array([0.25], np.float32)}
    b = {k: v.copy() for k, v in a.items()}
    iso.compare(a, b, "same")
    b["f.grads"][1] = np.nextafter(np.float32(0.5), np.float32(1))
    iso.compare(a, b, "one ulp", exact=False)
    with pytest.raises(AssertionError):
        iso.compare(a, b, "one ulp", exact=True)
    b["f.grads"][1] = 0.5 + 1e-5
    with pytest.raises(AssertionError):
        iso.compare(a, b, "1e-5", exact=False)
    b = {k: v.copy() for k, v in a.items()}
    b["f.hvo"][0] = np.nextafter(np.float32(0.25), np.float32(1))
    with pytest.raises(AssertionError):
        iso.compare(a, b, "forward side", exact=False)
    n = {k: v.copy() for k, v in a.items()}
    n["f.grads"][0] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        iso.compare(n, n, "nan", exact=False)
