"""The phase heads that request their state tiles as one group (csrc/gt_seq.h, seq_tile_request / seq_tile_store: the EXACT d_model-128
kernels, forward phase l > 0 and backward phases > 0 of head_dim 16 / 32 / 64) on the GPU: test_phase_head_loads.py's cases in full -- two
layers, 8 / 4 / 2 / 16 heads, batch 2 and 3, dropout 0 and 0.1, the library's own schedule (QUAD) and all SPLIT (CFG_NO_QUAD); three train
steps and one step with the saved tiles compared (check_ws) per case, the d_model-64 and d_model-32 cases beside them.  Every case asserts
from the GT_TRACE_DISPATCH lines which schedule ran.  Bars: parity.py's own."""
import pytest

from test_phase_head_loads import BATCHES, DROPOUT, HEADS, SCHEDULES, SMALL, _switches_back, run_d128, run_small  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("p", DROPOUT)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("H", HEADS)
def test_phase_heads_d128_gpu(H, B, p, sched):
    run_d128("hip", H, B, p, sched)


@pytest.mark.parametrize("p", DROPOUT)
@pytest.mark.parametrize("case", list(SMALL))
def test_phase_heads_small_gpu(case, p):
    run_small("hip", case, p)
