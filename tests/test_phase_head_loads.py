"""The head of a two-workgroups-per-sequence (SPLIT) or four-workgroups-per-sequence (QUAD) phase that begins with a state load: the EXACT
d_model-128 kernels request all of a thread's 16-byte pieces of the phase's tiles as one group and store them to LDS afterwards
(csrc/gt_seq.h, seq_tile_request / seq_tile_store; seq_fwd_body for a forward phase l > 0, seq_bwd_body for a backward phase > 0 of head_dim
16 / 32 / 64).  The same words reach the same LDS addresses in front of the same barrier, so everything downstream is as it was.
On the host emulator, two layers -- a forward phase with a state load, backward phases 1 and 2 --, 8 / 4 / 2 heads (head_dim 16 / 32 / 64)
and 16 heads (head_dim 8, whose backward head keeps the tile loops), batch 2 and 3 (odd: the tail of the block map), on the schedule the
library chooses at these batches (QUAD forward, QUAD backward phase 0, SPLIT backward phases) and all SPLIT (CFG_NO_QUAD): three train steps
(parity.check_train_step) and one step with the saved tiles the heads read compared too (parity.check_step, check_ws).  One d_model-64 and
one d_model-32 case: their kernels share the lambdas and keep the loops.  Every case asserts from the GT_TRACE_DISPATCH lines which
schedule ran.  Bars: parity.py's own.
Left out on the emulator: the dropout-0 runs of 8 and 2 heads; they run on the GPU (test_phase_head_loads_gpu.py).  A d_model-128 case
takes the emulator 30-45 s (four steps of up to twelve 512-thread workgroups), the file three and a half minutes on four workers."""
import pytest

import harness
import parity
from harness import cfg_dict, dispatched, trace_dispatch
from transformergrooveinfilling_amd import _lib

L = 2
HEADS = (8, 4, 2, 16)
BATCHES = (2, 3)
DROPOUT = (0.0, 0.1)
SCHEDULES = {"quad": 0, "split": _lib.CFG_NO_QUAD}
EMU_RUNS = [(H, B, p, s) for H in HEADS for B in BATCHES for p in DROPOUT for s in SCHEDULES if not (H in (8, 2) and p == 0.0)]
SMALL = {"d64": cfg_dict(64, 2, 32, 2), "d32": cfg_dict(32, 2, 16, 2)}


@pytest.fixture(autouse=True)
def _switches_back(request):
    yield
    lib = _lib.get_lib() if request.node.get_closest_marker("gpu") else harness.emu_lib()
    lib.cdll.gt_set_seq(1)
    lib.cdll.gt_set_seq_split(-1)
    lib.cdll.gt_set_seq_quad(-1)
    lib.cdll.gt_set_seq_ride(-1)


def ran_heads(trace, sched, steps, fused):
    """the forward phase with a state load and backward phases 1 and 2 ran, `steps` times each, on the schedule asked for"""
    fwd, bwd = dispatched(trace, "seq_fwd"), dispatched(trace, "seq_bwd")
    quad = 1 if sched == "quad" else 0
    assert fwd and all(d["split"] == 1 and d["quad"] == quad for d in fwd), fwd
    assert len([d for d in fwd if d["phase"] == L - 1]) == steps, fwd
    assert len(dispatched(trace, "seq_fwd", fuse_b0=1)) == (steps if fused else 0), fwd
    for ph in (1, 2):
        got = [d for d in bwd if d["phase"] == ph]
        assert len(got) == steps and all(d["split"] == 1 and d["quad"] == 0 for d in got), bwd
    b0 = [d for d in bwd if d["phase"] == 0]
    assert len(b0) == (0 if fused else steps) and all(d["quad"] == quad for d in b0), bwd


def run_d128(backend, H, B, p, sched):
    cfg, flags = cfg_dict(128, H, 64, L), SCHEDULES[sched]
    _, trace = trace_dispatch(lambda: parity.check_train_step(backend, cfg, B, p, flags=flags))
    print("%s H %d B %d p %.2f %s train step: %s" % (backend, H, B, p, sched, dict(parity.FIGURES)))
    ran_heads(trace, sched, 3, fused=sched == "quad" and H == 4)
    _, trace = trace_dispatch(lambda: parity.check_step(backend, cfg, B, p=p, check_ws=True, flags=flags))
    print("%s H %d B %d p %.2f %s step: %s" % (backend, H, B, p, sched, dict(parity.FIGURES)))
    ran_heads(trace, sched, 1, fused=False)


def run_small(backend, case, p):
    cfg = SMALL[case]
    _, trace = trace_dispatch(lambda: parity.check_train_step(backend, cfg, 2, p, seq="split"))
    print("%s %s p %.2f train step: %s" % (backend, case, p, dict(parity.FIGURES)))
    bwd = dispatched(trace, "seq_bwd")
    assert {d["phase"] for d in bwd} == {0, 1, 2} and all(d["split"] == 1 for d in bwd), bwd
    _, trace = trace_dispatch(lambda: parity.check_step(backend, cfg, 2, p=p, check_ws=True, seq="split"))
    print("%s %s p %.2f step: %s" % (backend, case, p, dict(parity.FIGURES)))
    bwd = dispatched(trace, "seq_bwd")
    assert {d["phase"] for d in bwd} == {0, 1, 2} and all(d["split"] == 1 for d in bwd), bwd


@pytest.mark.parametrize("H,B,p,sched", EMU_RUNS)
def test_phase_heads_d128_emu(H, B, p, sched):
    run_d128("emu", H, B, p, sched)


@pytest.mark.parametrize("p", DROPOUT)
@pytest.mark.parametrize("case", list(SMALL))
def test_phase_heads_small_emu(case, p):
    run_small("emu", case, p)
