"""The CPU twins of the sequence-resident kernels' oracle cases (tests/seq_variants.py): the cases with d_model <= 64 (seq_variants.EMU_TWINS
says which were dropped for time) on the emulator build -- the same checks with the same bars and the same asserted trace as tests/test_variant_ledger_gpu.py
runs on the GPU, so that this suite fails first when a host rule moves.  (The emulator's kernels are the GT_EMU twins of the GPU code: what a
given instantiation computes on the GPU is the GPU suite's to show.)"""
import pytest

import seq_variants as sv


@pytest.mark.parametrize("case", sv.EMU_TWINS)
def test_seq_variant_on_the_emulator(case):
    sv.check_trace(case, sv.run("emu", case))


# the cases written from the recording ([seq-before] of profiles/variant_ledger.txt), d_model <= 32: dim_feedforward 16, one or two layers, batch 2
BEFORE = {k: v for k, v in sv.before_cases().items() if v[0][1]["d_model"] <= 32}


@pytest.mark.parametrize("case", list(BEFORE))
def test_seq_before_on_the_emulator(case):
    spec, sigs = BEFORE[case]
    trace = sv.run("emu", spec, case)
    for sig in sigs:
        sv.check_lines(trace, sig)
