"""The closed per-operation walk of the bf16 modes away from initialisation, through the HIP library: the cases of tests/test_bf16_ops.py,
the attention kernels of csrc/gt_attn.h at head_dim 128 with a causal mask and across the encoder memory, and precision 2 in force at the
smallest shape the shipped threshold admits (d_model 512 at 2048 tokens: GT_T128H_MIN 64).  The MFMA accumulation order, the real expf and
the fp32 atomics of the weight gradients exist only here; bars as on the emulator (parity.check_ops_bf16).  profiles/bf16_ops.txt holds
the ratios this file printed on an MI355X."""
import pytest

import test_bf16_ops as T
from harness import cfg_dict

pytestmark = pytest.mark.gpu

CASES = dict(T.CASES)
CASES["encdec-d256-h2"] = (cfg_dict(256, 2, 64, 1, 1), 2, 0.1)        # gt_attn.h at head_dim 128: self, causal and cross
P2_CASES = {"d512-h8-b64": (cfg_dict(512, 8, 512, 1), 64, 0.1)}       # precision 2 in force (run_walk asserts it)
RUNS = [(c, g) for c in CASES for g in T.REGIMES] + [("d32-h4", "saturated")]


@pytest.mark.parametrize("case,regime", RUNS)
def test_walk_in_regime_hip(case, regime):
    T.run_walk("hip", CASES, case, regime)


@pytest.mark.parametrize("regime", T.REGIMES)
def test_walk_in_regime_precision_2_hip(regime):
    T.run_walk("hip", P2_CASES, "d512-h8-b64", regime, precision=2)
