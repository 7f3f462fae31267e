"""Oracle parity away from initialisation, on the host emulator: every regime of tests/regimes.py (peaked softmax, score rows shifted by
hundreds, saturated heads, LayerNorm variances at eps) on the smallest shape of every path -- whole-sequence d32 (head_dim 8 and 2), d128
SPLIT, d64 SPLIT, encoder-decoder (causal and cross attention), one kernel per operation.  parity.check_step(regime=...): the suite's fixed
bars, and every quantity within 8 x the fp32 oracle's own distance from the fp64 oracle.  Predict (the decode-step softmax) in the
saturated and shift regimes, the fused train step (its own loss code) in peaked and saturated.  tests/test_regimes_gpu.py runs the same
through the HIP library, and the wide shapes only there (profiles/regimes.txt: both tables and the mutation record)."""
import pytest

import harness
import parity
import regimes
from harness import cfg_dict

#        name: (cfg, B, dropout, Runner's seq)
CASES = {
    "d32-h4": (cfg_dict(32, 4, 16, 2), 3, 0.0, True),                  # whole-sequence d32, head_dim 8
    "d32-h16-drop": (cfg_dict(32, 16, 64, 2), 2, 0.1, True),           # head_dim 2: vector-ALU attention, keep bits
    "d128-h4-split-drop": (cfg_dict(128, 4, 64, 1), 2, 0.1, "split"),
    "d64-h16": (cfg_dict(64, 16, 256, 1), 2, 0.0, True),               # d64 SPLIT, head_dim 4
    "encdec-d32-h4": (cfg_dict(32, 4, 16, 1, 1), 2, 0.0, True),        # causal and cross attention
    "d32-h4-per-op-drop": (cfg_dict(32, 4, 16, 2), 3, 0.1, False),     # one kernel per operation
}
SEED = 8                         # of the parameters and the batch: the fp64 oracle alone meets every regime's condition on every shape here and in
#                                  tests/test_regimes_gpu.py (shift is the narrow one: layer 0's row maxima run from -96 to +92 at worst)
PREDICT_CASES = {"d32-h4": (cfg_dict(32, 4, 16, 2), 3), "encdec-d32-h4": (cfg_dict(32, 4, 16, 1, 1), 2)}
PREDICT_SEED = 24                # the conditions hold, and the oracle's decision margins leave every decode step of the encoder-decoder comparable
#        name: (cfg, B, Runner's seq, steps on the emulator -- a d_model-128 step takes it 12 s; the GPU runs check_train_step's three everywhere)
TRAIN_CASES = {"d32-h4": (cfg_dict(32, 4, 16, 2), 4, True, 3), "d128-h4-split": (cfg_dict(128, 4, 64, 1), 4, "split", 1)}
# check_train_step also follows the free-running fp64 trajectory.  Adam moves every live element by about lr per step whatever its gradient:
# at lr 0.05 the fp32 ORACLE's own three-step trajectory leaves the bars (d128 peaked: 6.8 x the live-element bar, 49 x the well-conditioned
# one, 15 x the loss bar; d32 saturated: 1.2 x the live-element bar), at 0.005 it stays under 0.21 of every bar on both shapes and in both
# regimes.  SGD at 0.05 stays under 0.02 of its bars everywhere and keeps it.  The teacher-forced per-element update check, the proof here,
# does not depend on the trajectory.
TRAIN_LR = {0: 0.05, 1: 0.005}
TRAIN_REGIMES = ("peaked", "saturated")


@pytest.fixture(autouse=True)
def _switches_back(request):
    """the process-wide schedule switches a Runner(seq=...) sets are put back whatever happens (in the library the test ran on)"""
    yield
    from transformergrooveinfilling_amd import _lib
    lib = _lib.get_lib() if request.node.get_closest_marker("gpu") else harness.emu_lib()
    lib.cdll.gt_set_seq(1)
    lib.cdll.gt_set_seq_split(-1)
    lib.cdll.gt_set_seq_quad(-1)
    lib.cdll.gt_set_seq_ride(-1)


def run_step(backend, cases, case, regime):
    cfg, B, p, seq = cases[case]
    try:
        parity.check_step(backend, cfg, B, p, seed=SEED, seq=seq, regime=regime)
    finally:
        f = parity.FIGURES
        print("%s %s %s: noise ratio %.2f at %s; out %.3f grad %.3f of the fixed bars; %s"
              % (backend, case, regime, f.get("noise", -1), f.get("noise_at"), f.get("out", -1), f.get("grad", -1), f.get("regime")))


@pytest.mark.parametrize("regime", list(regimes.REGIMES))
@pytest.mark.parametrize("case", list(CASES))
def test_step_in_regime(case, regime):
    run_step("emu", CASES, case, regime)


@pytest.mark.parametrize("regime", ["saturated", "shift"])
@pytest.mark.parametrize("case", list(PREDICT_CASES))
def test_predict_in_regime(case, regime):
    cfg, B = PREDICT_CASES[case]
    parity.check_predict("emu", cfg, B, regime=regime, seed=PREDICT_SEED)


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("regime", TRAIN_REGIMES)
@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_train_step_in_regime(case, regime, algo):
    cfg, B, seq, steps = TRAIN_CASES[case]
    parity.check_train_step("emu", cfg, B, 0.1, algo=algo, seq=seq, regime=regime, lr=TRAIN_LR[algo], steps=steps)
