"""The fused launch of the four-workgroups-per-sequence (QUAD) train step -- last forward phase + backward phase 0, seq_fb_kernel in
csrc/gt_seq.h -- hands over in LDS what the backward body used to reload: the last layer's hact half stays in sU, dlogits go from the loss
tail straight into the output-layer dgrad's A tile in sC, and the loss ticket is taken inside the backward body by one wave that nobody
waits for; the last arriver finishes the statistics on that wave, two stages later.  On the host emulator: three consecutive train steps per case (parity.check_train_step:
the ticket is re-armed by each launch, and taken exactly once per output-layer workgroup although the emulator runs a workgroup whose
partner's granules are missing again from its first instruction), one and two layers, an even and an odd batch, without and with
dropout; every case asserts from the GT_TRACE_DISPATCH lines that the fused launch ran.  parity.check_step drives forward, loss and
backward one by one: there backward phase 0 is a launch of its own on the same schedule and loads from global memory what the hand-over
skips -- asserted from the trace as well.  Bars: parity.py's own."""
import pytest

import harness
import parity
from harness import cfg_dict, dispatched, trace_dispatch

LAYERS = (1, 2)
BATCHES = (2, 3)
DROPOUT = (0.0, 0.1)


@pytest.fixture(autouse=True)
def _switches_back():
    yield
    lib = harness.emu_lib()
    lib.cdll.gt_set_seq(1)
    lib.cdll.gt_set_seq_split(-1)
    lib.cdll.gt_set_seq_quad(-1)
    lib.cdll.gt_set_seq_ride(-1)


@pytest.mark.parametrize("p", DROPOUT)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("L", LAYERS)
def test_fused_train_step_emu(L, B, p):
    _, trace = trace_dispatch(lambda: parity.check_train_step("emu", cfg_dict(128, 4, 64, L), B, p))
    print("emu L %d B %d p %.2f train step: %s" % (L, B, p, dict(parity.FIGURES)))
    fused = dispatched(trace, "seq_fwd", fuse_b0=1)
    assert len(fused) == 3 and all(d["quad"] == 1 and d["phase"] == L - 1 for d in fused), fused        # one per step
    assert not dispatched(trace, "seq_bwd", phase=0), trace                                                # phase 0 ran inside them


@pytest.mark.parametrize("p", DROPOUT)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("L", LAYERS)
def test_unfused_phase0_emu(L, B, p):
    """forward, loss and backward as calls of their own: backward phase 0 of the QUAD schedule from global memory"""
    _, trace = trace_dispatch(lambda: parity.check_step("emu", cfg_dict(128, 4, 64, L), B, p=p, check_ws=True))
    print("emu L %d B %d p %.2f step: %s" % (L, B, p, dict(parity.FIGURES)))
    assert dispatched(trace, "seq_fwd", quad=1) and not dispatched(trace, "seq_fwd", fuse_b0=1), trace
    b0 = dispatched(trace, "seq_bwd", phase=0)
    assert b0 and all(d["quad"] == 1 and d["fuse_b0"] == 0 for d in b0), b0
