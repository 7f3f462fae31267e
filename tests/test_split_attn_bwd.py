"""The attention backward of the two-workgroups-per-sequence (SPLIT) backward phases: each workgroup computes its own 16 rows only -- one
wave per (head, role), the row sums rd_i = dctx_i . ctx_i from the phase's state load (csrc/gt_seq.h, seq_attn_bwd1 / seq_bwd_body).
(head_dim < 16 at d_model 32 / 64 keeps the two-role form over the whole sequence: those kernels hold the reference's head_dim-2 passes.)
Every head_dim class the SPLIT dispatch instantiates (groove_seq_bwd.hip, groove_seq64.hip), at two layers -- a middle phase with a chain
behind the stage and the last phase -- and three sequences (odd: nothing leans on the batch being a multiple of eight), without and with
dropout (the attention dropout is inside ctx); whole step (parity.check_step, saved activations included) and each sequence's / row
half's share of the gradients (parity.check_grad_probes), bars unchanged: 2e-4 of the tensor's largest entry.  Each case asserts from the
GT_TRACE_DISPATCH lines that a backward phase >= 1 ran SPLIT.  Once on the emulator, once on the GPU."""
import pytest

import harness
import parity
from harness import cfg_dict, dispatched, trace_dispatch
from transformergrooveinfilling_amd import _lib

B = 3
ALL_SPLIT = _lib.CFG_NO_QUAD | _lib.CFG_NO_LN_XCHG          # no four-workgroup phases: every phase of the step runs SPLIT
# probes: the two row halves of the middle sequence (rows 15 | 16: one per workgroup of a pair); on the GPU, where a backward costs nothing, a
# whole sequence at either end as well
HALVES = [("row", 32 * (B // 2) + 15), ("row", 32 * (B // 2) + 16)]
PLACES = {"emu": HALVES, "hip": HALVES + [("seq", 0), ("seq", B - 1)]}

#        name: (cfg, Runner's seq, gt_config.flags)
CASES = {
    "d128-h4": (cfg_dict(128, 4, 512, 2), True, 0),                    # head_dim 32, the headline class: QUAD phase 0 + riders
    "d128-h4-all-split": (cfg_dict(128, 4, 512, 2), True, ALL_SPLIT),
    "d128-h16": (cfg_dict(128, 16, 512, 2), True, 0),                  # head_dim 8: zero-padded operands, four rounds of heads
    "d128-h2": (cfg_dict(128, 2, 512, 2), True, 0),                    # head_dim 64: a round with idle wave pairs
    "d128-h8": (cfg_dict(128, 8, 512, 2), True, 0),                    # head_dim 16: two full rounds
    "d64-h4": (cfg_dict(64, 4, 256, 2), "split", 0),                   # head_dim 16
    "d64-h2": (cfg_dict(64, 2, 256, 2), "split", 0),                   # head_dim 32
    "d64-h1": (cfg_dict(64, 1, 256, 2), "split", 0),                   # head_dim 64: one head, three idle wave pairs
    "d64-h8": (cfg_dict(64, 8, 256, 2), "split", 0),                   # head_dim 8 at d_model 64
    "d32-h4": (cfg_dict(32, 4, 256, 2), "split", 0),                   # head_dim 8
    "d32-h2": (cfg_dict(32, 2, 256, 2), "split", 0),                   # head_dim 16
    "d32-h1": (cfg_dict(32, 1, 256, 2), "split", 0),                   # head_dim 32
}
DROPOUT = (0.0, 0.24)
# (a d_model-128 case takes the emulator a minute: the one this file adds to the issue's table, d128-h8, runs there with dropout only)
EMU_RUNS = [(c, p) for c in CASES for p in DROPOUT if not (c == "d128-h8" and p == 0.0)]


@pytest.fixture(autouse=True)
def _switches_back(request):
    """the process-wide schedule switches a Runner(seq=...) sets are put back whatever happens (in the library the test ran on)"""
    yield
    lib = _lib.get_lib() if request.node.get_closest_marker("gpu") else harness.emu_lib()
    lib.cdll.gt_set_seq(1)
    lib.cdll.gt_set_seq_split(-1)
    lib.cdll.gt_set_seq_quad(-1)
    lib.cdll.gt_set_seq_ride(-1)


def _ran_split(trace, flags):
    bwd = dispatched(trace, "seq_bwd")
    assert [d for d in bwd if d["split"] == 1 and d["phase"] >= 1], bwd
    assert {d["phase"] for d in bwd} == {0, 1, 2}, bwd
    if flags == ALL_SPLIT:
        assert all(d["split"] == 1 and d["quad"] == 0 for d in bwd), bwd
        assert all(d["split"] == 1 and d["quad"] == 0 for d in dispatched(trace, "seq_fwd")), trace


def _run(backend, case, p):
    cfg, seq, flags = CASES[case]
    _, trace = trace_dispatch(lambda: parity.check_step(backend, cfg, B, p=p, check_ws=True, seq=seq, flags=flags))
    print("%s %s p %.2f step: %s" % (backend, case, p, dict(parity.FIGURES)))
    _ran_split(trace, flags)
    _, trace, places = parity.check_grad_probes(backend, cfg, B, p, PLACES[backend], seq=seq, flags=flags)
    print("%s %s p %.2f probes: %s" % (backend, case, p, dict(parity.FIGURES)))
    _ran_split(trace, flags)
    assert places == PLACES[backend]


@pytest.mark.parametrize("case,p", EMU_RUNS)
def test_split_attn_bwd_emu(case, p):
    _run("emu", case, p)


@pytest.mark.gpu
@pytest.mark.parametrize("p", DROPOUT)
@pytest.mark.parametrize("case", list(CASES))
def test_split_attn_bwd_gpu(case, p):
    _run("hip", case, p)
