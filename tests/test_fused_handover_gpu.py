"""The fused launch of the QUAD train step (last forward phase + backward phase 0, seq_fb_kernel in csrc/gt_seq.h) with its LDS hand-over
-- the last layer's hact half, dlogits -- and its loss ticket, taken inside the backward body by a wave nobody waits for, on the GPU: d_model 128 / 4 heads, dim_feedforward 64
and 512, one and three layers, without and with dropout, 8 and 40 sequences (40: 80 output-layer workgroups, so the last arriver's strided
sum covers more than 64 partials, and 160 workgroups are resident at once).  Three train steps against the oracle
(parity.check_train_step); five steps on two fresh engines from one seed, statistics and parameters bitwise equal (the ticket's
fixed-order sum, re-armed every step); both assert from the GT_TRACE_DISPATCH lines that the fused launch ran.  parity.check_grad_probes
drives forward and backward as calls of their own -- backward phase 0 of the same schedule as a launch, which loads from global memory
what the hand-over skips: asserted from the trace -- with probes on rows 15 and 16 of a sequence, the boundary between the row halves.
Bars: parity.py's own."""
import numpy as np
import pytest

import parity
from harness import Runner, cfg_dict, dispatched, trace_dispatch
from oracle import numpy_groove as ng
from transformergrooveinfilling_amd import _lib

pytestmark = pytest.mark.gpu

CASES = [(F, L, p, B) for F in (64, 512) for L in (1, 3) for p in (0.0, 0.24) for B in (8, 40)]
IDS = ["F%d-L%d-p%g-B%d" % c for c in CASES]


@pytest.fixture(autouse=True)
def _switches_back():
    yield
    lib = _lib.get_lib()
    lib.cdll.gt_set_seq(1)
    lib.cdll.gt_set_seq_split(-1)
    lib.cdll.gt_set_seq_quad(-1)
    lib.cdll.gt_set_seq_ride(-1)


def _fused(trace, L, steps):
    fused = dispatched(trace, "seq_fwd", fuse_b0=1)
    assert len(fused) == steps and all(d["quad"] == 1 and d["phase"] == L - 1 for d in fused), fused
    assert not dispatched(trace, "seq_bwd", phase=0), dispatched(trace, "seq_bwd")


@pytest.mark.parametrize("F,L,p,B", CASES, ids=IDS)
def test_fused_train_step_gpu(F, L, p, B):
    _, trace = trace_dispatch(lambda: parity.check_train_step("hip", cfg_dict(128, 4, F, L), B, p))
    print("hip F %d L %d p %.2f B %d train step: %s" % (F, L, p, B, dict(parity.FIGURES)))
    _fused(trace, L, 3)


@pytest.mark.parametrize("F,L,p,B", CASES, ids=IDS)
def test_row_half_probes_gpu(F, L, p, B):
    places = [("row", 32 * (B // 2) + 15), ("row", 32 * (B // 2) + 16)]
    _, trace, ran = parity.check_grad_probes("hip", cfg_dict(128, 4, F, L), B, p, places)
    print("hip F %d L %d p %.2f B %d probes: %s" % (F, L, p, B, dict(parity.FIGURES)))
    assert ran == places
    b0 = dispatched(trace, "seq_bwd", phase=0)
    assert b0 and all(d["quad"] == 1 and d["fuse_b0"] == 0 for d in b0), b0


@pytest.mark.parametrize("F,L,p,B", CASES, ids=IDS)
def test_fused_steps_bitwise_gpu(F, L, p, B):
    cfg = dict(cfg_dict(128, 4, F, L), dropout=p)
    P = ng.init_params(cfg, seed=9, perturb=0.05)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=4)

    def five():
        r = Runner(cfg, B, "hip", rng=(77, 5, 0), lr=0.05)
        r.set_params(P)
        stats = [np.array(r.train_step(x, y, 0.38, skip_update=4 if step else 0), np.float32).copy() for step in range(5)]
        return np.stack(stats), r.params.numpy().copy()

    (s0, p0), t0 = trace_dispatch(five)
    (s1, p1), t1 = trace_dispatch(five)
    _fused(t0, L, 5)
    _fused(t1, L, 5)
    assert np.isfinite(s0).all() and s0[0, 0] != s0[4, 0], s0[:, 0]
    assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)), (s0, s1)
    assert np.array_equal(p0.view(np.uint32), p1.view(np.uint32))
