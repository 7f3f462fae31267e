"""Oracle parity away from initialisation through the HIP library: the cases of tests/test_regimes.py, and the shapes the emulator is too
slow for -- d_model 128 on the whole-sequence and on the library's own schedule (QUAD and the fused launch), and the
one-kernel-per-operation attention kernels of csrc/gt_attn.h at head_dim 128, 64, 32 and 16 (the last as an encoder-decoder).  The real
expf / tanhf / log1pf, the MFMA accumulation order and the fp32 atomics of the weight gradients exist only here; bars as on the emulator
(parity.check_step_regime).  profiles/regimes.txt holds the table of ratios this file printed on an MI355X."""
import pytest

import parity
import regimes
import test_regimes as T
from harness import cfg_dict
from test_regimes import _switches_back  # noqa: F401  (autouse: the schedule switches are put back after every test)

pytestmark = pytest.mark.gpu

CASES = dict(T.CASES)
CASES.update({
    "d128-h4-whole-drop": (cfg_dict(128, 4, 64, 1), 2, 0.1, "whole"),
    "d128-h4-library-drop": (cfg_dict(128, 4, 64, 1), 2, 0.1, True),       # the library's choice: QUAD forward, fused launch
    "d256-h2-drop": (cfg_dict(256, 2, 64, 1), 2, 0.1, True),               # gt_attn.h, head_dim 128
    "d512-h8": (cfg_dict(512, 8, 64, 1), 2, 0.0, True),                    # head_dim 64
    "encdec-d256-h16-drop": (cfg_dict(256, 16, 64, 1, 1), 2, 0.1, True),   # head_dim 16, causal and cross attention
    "d64-h2-per-op-drop": (cfg_dict(64, 2, 64, 1), 2, 0.1, False),         # head_dim 32
})


@pytest.mark.parametrize("regime", list(regimes.REGIMES))
@pytest.mark.parametrize("case", list(CASES))
def test_step_in_regime_hip(case, regime):
    T.run_step("hip", CASES, case, regime)


@pytest.mark.parametrize("regime", ["saturated", "shift"])
@pytest.mark.parametrize("case", list(T.PREDICT_CASES))
def test_predict_in_regime_hip(case, regime):
    cfg, B = T.PREDICT_CASES[case]
    parity.check_predict("hip", cfg, B, regime=regime, seed=T.PREDICT_SEED)
    print("hip predict %s %s: %s" % (case, regime, {k: v for k, v in parity.FIGURES.items() if k != "regime"}))


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("regime", T.TRAIN_REGIMES)
@pytest.mark.parametrize("case", list(T.TRAIN_CASES))
def test_train_step_in_regime_hip(case, regime, algo):
    cfg, B, seq, _ = T.TRAIN_CASES[case]
    parity.check_train_step("hip", cfg, B, 0.1, algo=algo, seq=seq, regime=regime, lr=T.TRAIN_LR[algo])
    print("hip train %s %s algo %d: update %.3f of its bar" % (case, regime, algo, parity.FIGURES["update"]))
