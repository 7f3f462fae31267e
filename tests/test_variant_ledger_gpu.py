"""Oracle cases for the kernel variants no other GPU test launches (profiles/variant_ledger.txt, section [before]; DESIGN.md 4a "Variant
ledger").  Each case is one of the project's parity checks with its bars unchanged, at the smallest shape of the sweep grid that reaches
the variant, and asserts from its own dispatch trace that every signature it is listed for ran.

GT_VARIANT_LEDGER_TIMES=<file>: append "case <tab> seconds" per case (the [cases] section of the record)."""
import os
import time

import pytest

import parity
import seq_variants as sv
import variant_ledger as vl
from harness import cfg_dict, dispatched, trace_dispatch
from transformergrooveinfilling_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switches_back():
    """the process-wide schedule switches a Runner(seq=...) sets are put back whatever happens"""
    yield
    lib = _lib.get_lib()
    lib.cdll.gt_set_seq(1)
    lib.cdll.gt_set_seq_split(-1)
    lib.cdll.gt_set_seq_quad(-1)
    lib.cdll.gt_set_seq_ride(-1)


ran = sv.ran


def step(cfg, B, p=0.1, **kw):
    return lambda: parity.check_step("hip", cfg, B, p, **kw)


def bf16(cfg, B, p=0.1, **kw):
    return lambda: parity.check_step_bf16("hip", cfg, B, p, **kw)


def train_bf16(cfg, B, p=0.1, **kw):
    return lambda: parity.check_train_step_bf16("hip", cfg, B, p, **kw)


def probes(cfg, B, p=0.1, **kw):
    """six probes on the token-chunk boundaries read from the trace; returns the trace check_grad_probes took of its own calls"""
    places = lambda trace, M: parity.probe_places(M // 32, parity.chunk_rows(trace, M), split_rows=False, limit=6)
    return lambda: parity.check_grad_probes("hip", cfg, B, p, places, **kw)[1]


G32 = "gemm32 BM 128 BN 128 form %s epi %d prec 1 src fp32 rowx %d"
GEN = "gemm_cfg BM %d BN %d BK %d form %s epi %d prec %d splitk 1 row %d rowx %d edge %d"
LNB = "ln_bwd variant %s d %d rpw %d in16 0"
D64_LM, D32_LM, D16_LM = cfg_dict(64, 1, 2048, 1), cfg_dict(32, 1, 2048, 1), cfg_dict(16, 1, 2048, 1)
D64_ENCDEC, D16_ENCDEC = cfg_dict(64, 1, 16, 1, 1), cfg_dict(16, 1, 16, 1, 1)
D128_H2, D256_H2 = cfg_dict(128, 2, 16, 1), cfg_dict(256, 2, 16, 1)
CLS1 = ["wgrad_queue cls 1 splitk 2 prec 0 tail 0"]
GEN64_FFN = [GEN % (64, 64, 32, "NT", 3, 0, 0, 0, 0), GEN % (64, 64, 32, "NN", 5, 0, 0, 0, 0)]
ROW_D64 = [GEN % (32, 64, 64, "NN", 8, 0, 1, 0, 0), GEN % (32, 64, 64, "NN", 8, 0, 1, 0, 1), GEN % (32, 64, 64, "NT", 7, 0, 1, 0, 1)]
LN_D16 = [LNB % ("generic", 16, 8), LNB % ("two_norms", 16, 8)]
G32_FFN = [G32 % ("NT", 3, 0), G32 % ("NT", 5, 0)]
G64_LNBWD = ["gemm64 BM 64 BN 64 form NT epi 8 prec 1 src fp32 rowx 1"]

# name: (the check, the signatures it is the oracle case of).  Dropout 0.1 everywhere: the FFN epilogues (epi 3 / 5) and the residual ones
# (7 ... 10) draw their masks.  "-peaked" / "-flat": the same shape in a regime of tests/regimes.py, one per kernel family -- peaked where the
# variant multiplies what the softmax produced or feeds it, flat where it computes or differentiates a LayerNorm.
CASES = {
    # ---- bf16 operands (precision 1) from fp32 sources: the small models have no operand shadows ----
    "bf16-d64-F2048-B64": (bf16(D64_LM, 64), G32_FFN),
    "bf16-d64-F2048-B64-peaked": (bf16(D64_LM, 64, regime="peaked"), G32_FFN),
    "bf16-encdec-d64-F2048-B64": (bf16(cfg_dict(64, 1, 2048, 1, 1), 64), [G32 % ("NN", 5, 0)]),
    # batch 512 (16384 tokens) is the first of the grid at which the 128x128 ring tile takes these d_model 256 / 512 GEMMs under precision 1:
    # the fp64 walk over that many tokens is what these four cost, 7 ... 16 s each.  (An encoder-decoder of one layer each reaches the three d_model 256 signatures at once, in 31 s.)
    "bf16-d512-F16-B512": (bf16(cfg_dict(512, 8, 16, 1), 512), [G32 % ("NN", 0, 0), G32 % ("NN", 6, 0), GEN % (128, 128, 32, "NN", 0, 1, 0, 0, 1)]),
    "bf16-d512-F64-B512": (bf16(cfg_dict(512, 8, 64, 1), 512), [G32 % ("NT", 6, 0)]),
    "bf16-d256-F16-L2-B512": (bf16(cfg_dict(256, 8, 16, 2), 512), [G32 % ("NN", 8, 1), G32 % ("NT", 7, 1)]),
    "bf16-d256-F64-B512": (bf16(cfg_dict(256, 8, 64, 1), 512), [G32 % ("NT", 8, 1)]),
    "bf16-d256-F256-B128": (bf16(cfg_dict(256, 1, 256, 1), 128), G64_LNBWD),
    "bf16-d256-F256-B128-flat": (bf16(cfg_dict(256, 1, 256, 1), 128, regime="flat"), G64_LNBWD),
    "bf16-d32-F2048-B128": (bf16(D32_LM, 128), [GEN % (128, 128, 32, "NT", 3, 1, 0, 0, 0), GEN % (128, 128, 32, "NT", 5, 1, 0, 0, 0)]),
    "bf16-encdec-d32-F2048-B128": (bf16(cfg_dict(32, 1, 2048, 1, 1), 128), [GEN % (128, 128, 32, "NN", 5, 1, 0, 0, 0)]),
    "bf16-d16-F2048-B128": (bf16(D16_LM, 128), [GEN % (128, 128, 32, "NN", 5, 1, 0, 0, 1)]),
    "bf16-d16-F2048-B32": (bf16(D16_LM, 32), [GEN % (64, 64, 64, "NT", 3, 1, 0, 0, 1), GEN % (64, 64, 64, "NN", 5, 1, 0, 0, 1)]),
    "bf16-d32-F2048-B32": (bf16(D32_LM, 32), [GEN % (64, 64, 64, "NT", 5, 1, 0, 0, 1)]),
    "bf16-d256-F16-L2-B16": (bf16(cfg_dict(256, 1, 16, 2), 16), [GEN % (32, 32, 64, "NN", 10, 1, 0, 1, 0)]),
    "bf16-d32-F64-B16": (bf16(cfg_dict(32, 1, 64, 1), 16), [GEN % (32, 32, 64, "NT", 5, 1, 0, 0, 1), GEN % (32, 32, 64, "NT", 6, 1, 0, 0, 1)]),
    "bf16-d64-F16-B512": (bf16(cfg_dict(64, 1, 16, 1), 512), [GEN % (64, 64, 64, "NT", 0, 1, 0, 0, 0)]),
    "bf16-d16-F16-B16": (bf16(cfg_dict(16, 1, 16, 1), 16), [LNB % ("generic", 16, 2), LNB % ("two_norms", 16, 2), "ln_fwd variant two_norms d 16 in16 0"]),
    # ---- weight-gradient class 1 (64x64 tiles, 256-token chunks) without a token tail ----
    "wgrad-cls1-d64-F2048-B128": (probes(D64_LM, 128), CLS1),
    "wgrad-cls1-d64-F2048-B128-peaked": (step(D64_LM, 128, regime="peaked"), CLS1),
    "wgrad-cls1-bf16-d64-F2048-B128": (probes(D64_LM, 128, precision=1), ["wgrad_queue cls 1 splitk 2 prec 1 tail 0", "wgrad_flush cls 1 prec 1"]),
    # ---- the output heads behind bf16 storage, alone and with the loss in the launch ----
    "heads-d128-prec2": (bf16(D128_H2, 16, precision=2), ["heads d 128 prec 2 loss 0"]),
    "heads-d128-prec2-flat": (bf16(D128_H2, 16, precision=2, regime="flat"), ["heads d 128 prec 2 loss 0"]),
    "heads-loss-d128-prec2": (train_bf16(D128_H2, 16, precision=2), ["heads d 128 prec 2 loss 1"]),
    "heads-loss-d256-prec1": (train_bf16(D256_H2, 16, precision=1), ["heads d 256 prec 1 loss 1"]),
    "heads-loss-d256-prec2": (train_bf16(D256_H2, 16, precision=2), ["heads d 256 prec 2 loss 1"]),
    # ---- fp32: generic tiles without an edge, the row-owning tiles of the narrow models, LayerNorm backward at 8 rows per wave ----
    "d32-F2048-B128": (step(D32_LM, 128), [GEN % (128, 128, 32, "NN", 5, 0, 0, 0, 0)]),
    "d32-F2048-B32": (step(D32_LM, 32), GEN64_FFN),
    "d32-F2048-B32-peaked": (step(D32_LM, 32, regime="peaked"), GEN64_FFN),
    "d128-H1-F16-L2-B256": (step(cfg_dict(128, 1, 16, 2), 256), [GEN % (32, 128, 64, "NN", 8, 0, 1, 0, 0), GEN % (32, 128, 64, "NN", 8, 0, 1, 0, 1),
                                                                GEN % (32, 128, 64, "NT", 7, 0, 1, 0, 1)]),
    "encdec-d32-F64-B256": (step(cfg_dict(32, 1, 64, 1, 1), 256), [GEN % (32, 32, 64, "NN", 8, 0, 1, 0, 0), GEN % (32, 32, 64, "NN", 8, 0, 1, 0, 1),
                                                                 LNB % ("generic", 32, 8), LNB % ("two_norms", 32, 8)]),
    "encdec-d16-F16-B256": (step(D16_ENCDEC, 256), LN_D16),
    "encdec-d16-F16-B256-flat": (step(D16_ENCDEC, 256, regime="flat"), LN_D16),
    "encdec-d64-F16-B256": (step(D64_ENCDEC, 256), ROW_D64 + [LNB % ("generic", 64, 8), LNB % ("two_norms", 64, 8)]),
    "encdec-d64-F16-B256-flat": (step(D64_ENCDEC, 256, regime="flat"), ROW_D64),
    "d256-F64-B256": (step(cfg_dict(256, 1, 64, 1), 256), [GEN % (64, 64, 32, "NN", 0, 0, 0, 0, 0)]),
    "d512-F16-B256": (step(cfg_dict(512, 8, 16, 1), 256), [LNB % ("v4", 512, 8)]),
}

# signature: why it may stay without a case (profiles/variant_ledger.txt, section [remaining]) -- none does
MAY_STAY = {}


@pytest.mark.parametrize("case", list(CASES))
def test_variant(case):
    check, sigs = CASES[case]
    t0 = time.time()
    own, trace = trace_dispatch(check)
    if isinstance(own, list):                     # (check_grad_probes traces its own forward and backward: those lines do not reach this trace)
        trace = trace + own
    missing = [s for s in sigs if not ran(trace, s)]
    assert not missing, "not launched: %s\nlaunched: %s" % (missing, sorted(set(vl.signatures(trace))))
    _time(case, t0)


def _time(case, t0):
    times = os.environ.get("GT_VARIANT_LEDGER_TIMES")
    if times:
        with open(times, "a") as f:
            f.write("%s\t%.1f\n" % (case, time.time() - t0))


# ---- the sequence-resident kernels by head class, form and fused loss (section [seq-universe] of the record): tests/seq_variants.py holds the
# table -- its small cases run on the emulator build too (tests/test_seq_variants.py) -------------------------------------------------------
@pytest.mark.parametrize("case", list(sv.CASES))
def test_seq_variant(case):
    t0 = time.time()
    sv.check_trace(case, sv.run("hip", case))
    _time("seq:" + case, t0)


# the signatures of [seq-before] that table does not reach, each at the smallest shape of the enumeration that does (seq_variants.before_cases)
BEFORE = sv.before_cases()


@pytest.mark.parametrize("case", list(BEFORE))
def test_seq_before(case):
    spec, sigs = BEFORE[case]
    t0 = time.time()
    trace = sv.run("hip", spec, case)
    for sig in sigs:
        sv.check_lines(trace, sig)
    _time("seq:" + case, t0)
