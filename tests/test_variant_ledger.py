"""The variant ledger on the CPU (tests/variant_ledger.py): profiles/variant_ledger.txt lists exactly the launch signatures the sweep grid
can reach, every test it names exists, signature() keeps what names a kernel and drops the sizes, and the GT_VARIANT_LEDGER recording
writes what trace_dispatch sees."""
import os
import re

import pytest

import parity
import variant_ledger as vl
from harness import ROOT, cfg_dict, parse_dispatch, trace_dispatch


def _ledger_message(missing, stale):
    return ("profiles/variant_ledger.txt and the sweep grid's dry trace differ.\n%d signatures the grid reaches have no line (a new kernel variant or "
            "dispatch rule: record which oracle case runs each):\n  %s\n%d lines name a signature the grid no longer reaches:\n  %s\nre-record: %s"
            % (len(missing), "\n  ".join(missing) or "-", len(stale), "\n  ".join(stale) or "-", vl.RERECORD))


def check_record_is_the_universe(path):
    rec = vl.read_record(path)
    sigs = [ln[0] for ln in rec["universe"]]
    assert len(sigs) == len(set(sigs)), "a signature has two lines"
    missing, stale = vl.compare(sigs, vl.universe())
    assert not missing and not stale, _ledger_message(missing, stale)
    return rec


def test_record_is_the_universe():
    """every signature a grid configuration can launch has a line -- covered or UNCOVERED with its reason -- and no line is stale"""
    rec = check_record_is_the_universe(vl.RECORD)
    left = [ln for ln in rec["universe"] if ln[2] == "UNCOVERED"]
    assert all(len(ln) == 5 and ln[4] and ln[4] != "NO REASON" for ln in left), [ln for ln in left if len(ln) != 5 or ln[4] == "NO REASON"]
    assert sorted(ln[0] for ln in left) == sorted(ln[0] for ln in rec["remaining"])
    before = {ln[0] for ln in rec["before"]}
    assert before == {ln[0] for ln in rec["closed"]} | {ln[0] for ln in rec["remaining"]}


def test_a_removed_line_fails_by_name(tmp_path):
    """negative control: a copy of the record without one covered line fails, and the message names that signature and the command"""
    lines = open(vl.RECORD).read().splitlines(True)
    start = lines.index("[universe]\n")
    drop = next(i for i in range(start + 1, len(lines)) if " | " in lines[i] and "UNCOVERED" not in lines[i] and not lines[i].startswith("#"))
    gone = lines[drop].split(" | ")[0]
    copy = tmp_path / "variant_ledger.txt"
    copy.write_text("".join(lines[:drop] + lines[drop + 1:]))
    with pytest.raises(AssertionError) as e:
        check_record_is_the_universe(str(copy))
    assert gone in str(e.value) and "1 signatures the grid reaches have no line" in str(e.value) and vl.RERECORD in str(e.value)


def _seq_message(missing, stale):
    return ("profiles/variant_ledger.txt [seq-universe] and the dry trace of the sequence-resident enumeration (variant_ledger.seq_trace) differ.\n"
            "%d signatures the enumeration reaches have no line (a new instantiation, attention form or schedule rule: record which oracle case runs "
            "each):\n  %s\n%d lines name a signature it no longer reaches:\n  %s\nre-record: %s"
            % (len(missing), "\n  ".join(missing) or "-", len(stale), "\n  ".join(stale) or "-", vl.RERECORD))


def check_record_is_the_seq_universe(path):
    rec = vl.read_record(path)
    sigs = [ln[0] for ln in rec["seq-universe"]]
    assert len(sigs) == len(set(sigs)), "a signature has two lines"
    missing, stale = vl.compare(sigs, vl.seq_universe())
    assert not missing and not stale, _seq_message(missing, stale)
    return rec


def test_record_is_the_seq_universe():
    """the same for the sequence-resident kernels at the resolution at which they are instantiated: every seq_* signature of the enumeration
    -- every (d_model, heads) seq_supported admits, off the grid too, each schedule forced and not, every entry-point form -- has a line"""
    rec = check_record_is_the_seq_universe(vl.RECORD)
    left = [ln for ln in rec["seq-universe"] if ln[2] == "UNCOVERED"]
    assert all(len(ln) == 5 and ln[4] and ln[4] != "NO REASON" for ln in left), [ln for ln in left if len(ln) != 5 or ln[4] == "NO REASON"]
    assert sorted(ln[0] for ln in left) == sorted(ln[0] for ln in rec["seq-remaining"])
    before = {ln[0] for ln in rec["seq-before"]}
    assert before == {ln[0] for ln in rec["seq-closed"]} | {ln[0] for ln in rec["seq-remaining"]}
    assert before <= {ln[0] for ln in rec["seq-universe"]}
    # the second universe holds the first one's share of these kernels: no seq_* signature of the sweep grid is missing from the enumeration
    assert {s for s in vl.universe() if s.split()[0] in ("seq_fwd", "seq_bwd")} <= vl.seq_universe()
    # the enumeration names every (d_model, heads) pair the issue of record lists: the widths off the grid and their odd head counts
    assert {(48, 3), (48, 16), (80, 5), (96, 3), (112, 7), (128, 16), (16, 16)} <= set(vl.seq_models()) and (128, 1) not in vl.seq_models()


def test_generated_cases_cover_the_seq_before_list():
    """tests/test_variant_ledger_gpu.py::test_seq_before takes its cases from the record (seq_variants.before_cases): every [seq-before]
    signature is the table's -- the case [seq-closed] names for it exists in seq_variants.CASES -- or has a generated case, and there are some"""
    import seq_variants as sv
    rec = vl.read_record()
    closed = {ln[0]: ln[1] for ln in rec["seq-closed"]}
    table = {s for s, t in closed.items() if "::test_seq_variant[" in t}
    assert all(closed[s].split("[", 1)[1][:-1] in sv.CASES for s in table), [closed[s] for s in table if closed[s].split("[", 1)[1][:-1] not in sv.CASES]
    gen = sv.before_cases()
    generated = {s for spec, sigs in gen.values() for s in sigs}
    assert generated and generated == {ln[0] for ln in rec["seq-before"]} - table
    assert all(closed[s].split("[", 1)[1][:-1] in gen for s in generated if "::test_seq_before[" in closed[s])


def test_a_removed_seq_line_fails_by_name(tmp_path):
    """negative control for the second universe: without one of its lines the check fails and names the signature"""
    lines = open(vl.RECORD).read().splitlines(True)
    start = lines.index("[seq-universe]\n")
    drop = next(i for i in range(start + 1, len(lines)) if " | " in lines[i] and not lines[i].startswith("#"))
    gone = lines[drop].split(" | ")[0]
    copy = tmp_path / "variant_ledger.txt"
    copy.write_text("".join(lines[:drop] + lines[drop + 1:]))
    with pytest.raises(AssertionError) as e:
        check_record_is_the_seq_universe(str(copy))
    assert gone in str(e.value) and "1 signatures the enumeration reaches have no line" in str(e.value) and vl.RERECORD in str(e.value)


def test_named_tests_exist():
    """every test id of the record is a file under tests/ and a function of that name in it"""
    rec = vl.read_record()
    ids = {ln[2] for ln in rec["universe"] if ln[2] != "UNCOVERED"} | {ln[1] for ln in rec["closed"]} | {ln[2] for ln in rec["off-grid"]}
    ids |= {ln[2] for ln in rec["seq-universe"] if ln[2] != "UNCOVERED"} | {ln[1] for ln in rec["seq-closed"]}
    assert len(ids) > 20
    src = {}
    for tid in sorted(ids):
        path, _, func = tid.partition("::")
        func = func.split("[")[0]
        assert path.startswith("tests/") and os.path.isfile(os.path.join(ROOT, path)), tid
        if path not in src:
            src[path] = open(os.path.join(ROOT, path)).read()
        assert re.search(r"^def %s\(" % re.escape(func), src[path], re.M), tid


def _sig(line):
    (fam, kv), = parse_dispatch("[dispatch] " + line)
    return vl.signature(fam, kv)


GEMM = "gemm_cfg BM 64 BN 64 BK 32 M %d N %d K %d form NT epi %d prec %d splitk %d row 0 rowx %d edge %d"


def test_signature_drops_sizes_and_keeps_what_names_a_kernel():
    base = _sig(GEMM % (2048, 512, 256, 3, 0, 1, 0, 0))
    assert base == "gemm_cfg BM 64 BN 64 BK 32 form NT epi 3 prec 0 splitk 1 row 0 rowx 0 edge 0"
    assert _sig(GEMM % (1056, 2048, 128, 3, 0, 1, 0, 0)) == base                  # M N K alone
    others = [_sig(GEMM % (2048, 512, 256, 5, 0, 1, 0, 0)), _sig(GEMM % (2048, 512, 256, 3, 0, 1, 0, 1)),
              _sig(GEMM % (2048, 512, 256, 3, 1, 1, 0, 0)), _sig(GEMM % (2048, 512, 256, 3, 0, 1, 1, 0))]      # epi, edge, prec, rowx
    assert len(set(others + [base])) == 5
    many = _sig(GEMM % (2048, 512, 256, 3, 0, 5, 0, 0))
    assert many == _sig(GEMM % (2048, 512, 256, 3, 0, 33, 0, 0)) and many != base  # split-K or not, not how far
    assert _sig("kernel grid 4 gy 1 gz 1 block 256") is None
    assert _sig("ln_fwd variant one_norm M 512 d 128 in16 0") == "ln_fwd variant one_norm d 128 in16 0"
    assert _sig("ln_fwd variant one_norm M 512 d 256 in16 0") != _sig("ln_fwd variant one_norm M 512 d 128 in16 0")
    bwd = "seq_bwd phase %d split 1 quad 0 ride 1 riders %d fuse_b0 0 B 4 d 128 F 64 L 2 hc 32 exact 1 attn mfma loss 0"
    assert _sig(bwd % (1, 24)) == _sig(bwd % (3, 7)) != _sig(bwd % (0, 24))
    assert _sig(bwd % (1, 24)) != _sig(bwd % (1, 0))
    assert _sig(bwd % (1, 24)) == "seq_bwd phase 1 split 1 quad 0 ride 1 riders 1 fuse_b0 0 d 128 hc 32 exact 1 attn mfma loss 0"
    fwd = "seq_fwd phase 0 split %d quad 0 ride 0 fuse_b0 0 B 3 d %d F 64 L 2 hc %d exact %d attn %s loss %d"
    whole = _sig(fwd % (0, 32, 0, 1, "mfma-pad", 0))                                # the instantiation, the attention form and the fused loss
    assert whole == "seq_fwd phase 0 split 0 quad 0 ride 0 fuse_b0 0 d 32 hc 0 exact 1 attn mfma-pad loss 0"
    assert len({whole, _sig(fwd % (1, 32, 0, 1, "valu", 0)), _sig(fwd % (1, 32, 0, 1, "mfma-pad", 0)), _sig(fwd % (0, 32, 16, 1, "mfma", 0)),
                _sig(fwd % (0, 48, 0, 0, "mfma-pad", 0)), _sig(fwd % (0, 32, 0, 1, "mfma-pad", 1))}) == 6
    assert _sig("wgrad_queue cls 2 M 2048 N 256 K 4128 k_chunk 512 splitk 9 prec 0 tail 1") == "wgrad_queue cls 2 splitk 2 prec 0 tail 1"
    assert _sig("attn_fwd kernel mfma32 pairs 64") == "attn_fwd kernel mfma32"


CFG, B, P_DROP = cfg_dict(32, 4, 16, 1), 2, 0.1


def test_level_1_trace_is_the_level_2_trace_without_the_instantiation_keys(capfd, monkeypatch):
    """GT_TRACE_DISPATCH=1 prints the lines as they were before the sequence-resident ones named their instantiation -- what a reader outside
    this harness parses key by key; level 2 -- harness.TRACE_LEVEL, the one parse_dispatch reads -- prints the same launches in the same order
    with " hc .. exact .. attn .. loss .." behind the seq_fwd / seq_bwd keys, and nothing else differs"""
    monkeypatch.delenv("GT_VARIANT_LEDGER", raising=False)
    texts = {}
    for level in ("1", "2"):
        monkeypatch.setenv("GT_TRACE_DISPATCH", level)
        capfd.readouterr()
        parity.check_step("emu", CFG, B, P_DROP)
        texts[level] = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[dispatch] ")]
    tail = re.compile(r" hc \d+ exact [01] attn [a-z-]+ loss [01]$")
    seq = [ln for ln in texts["2"] if ln.split()[1] in ("seq_fwd", "seq_bwd")]
    assert seq and all(tail.search(ln) for ln in seq) and not [ln for ln in texts["1"] if tail.search(ln)]
    assert [tail.sub("", ln) if ln in seq else ln for ln in texts["2"]] == texts["1"]
    assert parse_dispatch("\n".join(texts["2"]))


def test_recording_on_the_emulator(tmp_path, monkeypatch):
    """one small check_step with GT_VARIANT_LEDGER set writes exactly the signatures trace_dispatch sees for the same calls, each with this
    test's id; unset, no file appears"""
    path = tmp_path / "ledger.tsv"
    monkeypatch.delenv("GT_VARIANT_LEDGER", raising=False)
    monkeypatch.delenv("GT_TRACE_DISPATCH", raising=False)
    _, trace = trace_dispatch(lambda: parity.check_step("emu", CFG, B, P_DROP))
    assert not path.exists() and "GT_TRACE_DISPATCH" not in os.environ
    want = set(vl.signatures(trace))
    assert len(want) >= 5
    monkeypatch.setenv("GT_VARIANT_LEDGER", str(path))
    parity.check_step("emu", CFG, B, P_DROP)
    assert "GT_TRACE_DISPATCH" not in os.environ
    seen = vl.read_recording(str(path))
    assert set(seen) == want, (sorted(set(seen) ^ want))
    me = os.environ["PYTEST_CURRENT_TEST"]
    assert all(list(t) == [me] for t in seen.values()), seen
    assert vl.node_id(me) == "tests/test_variant_ledger.py::test_recording_on_the_emulator"
    # trace_dispatch appends too, and the lines an enclosing trace reads still reach it
    os.remove(str(path))
    _, again = trace_dispatch(lambda: parity.check_step("emu", CFG, B, P_DROP))
    assert vl.signatures(again) == vl.signatures(trace)
    assert set(vl.read_recording(str(path))) == want
