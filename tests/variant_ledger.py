"""The ledger of kernel variants: which launch signatures a configuration of the sweep grid can make the library launch, and which
oracle case has run each of them on the GPU (profiles/variant_ledger.txt; DESIGN.md 4a "Variant ledger").

A SIGNATURE is a parsed "[dispatch]" line (harness.parse_dispatch) without its sizes: the family plus every key that names a kernel
instantiation or a branch the host chose.  signature() is the one statement of that rule.  The anonymous "kernel" family (a launch nobody
described: loss, optimizer, predict head, voice select, metrics, gather, infill and hit-curve kernels) carries no name and is left out;
each of those kernels has an exact test of its own.  "wgrad_queue" lines are queued problems, not launches; they stay in, because the
class, the split and the token tail of a problem pick the code that wgrad_flush's workgroups run.

The UNIVERSE is the set of signatures of a dry trace (emulator build, GT_EMU_DRY=1: host rules only) of tools/dispatch_trace.py's sweep
grid.  RECORDING: with GT_VARIANT_LEDGER=<file> set, harness.Runner and harness.trace_dispatch append "signature <tab> test id" for every
launch they make (harness.ledger_call).  The record file is written from such a recording of the whole GPU suite:

    GT_VARIANT_LEDGER=ledger.tsv GT_VARIANT_LEDGER_TIMES=times.tsv python -m pytest tests -m gpu          # on an MI355X
    python tests/variant_ledger.py ledger.tsv times.tsv > profiles/variant_ledger.txt

What a signature says: this variant ran inside a comparison with the oracle at least once.  It says nothing of every data regime or of
every shape edge within the variant; the rule -> boundary -> test table of DESIGN.md 4a keeps that job."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "variant_ledger.txt")
RERECORD = ("GT_VARIANT_LEDGER=<file> GT_VARIANT_LEDGER_TIMES=<times> python -m pytest tests -m gpu (on an MI355X), then "
            "python tests/variant_ledger.py <file> <times> > profiles/variant_ledger.txt")
GAP_TESTS = "tests/test_variant_ledger_gpu.py"          # the cases written for the gaps: a signature only they run was uncovered before them
SEQ_TESTS = GAP_TESTS + "::test_seq_"                   # ... and the ones written for the seq universe (test_seq_variant, test_seq_before)

KEEP = ("BM", "BN", "BK", "form", "epi", "prec", "src", "splitk", "row", "rowx", "edge", "cls", "tail", "variant", "in16", "rpw", "kernel", "kind",
        "algo", "split", "quad", "ride", "fuse_b0", "loss", "riders", "phase", "hc", "exact", "attn")
KEEP_D = ("ln_fwd", "ln_bwd", "ln_param_reduce", "heads", "seq_pack", "seq_fwd", "seq_bwd", "seq_tail")
COLLAPSE = dict(splitk=1, riders=0, phase=0)             # key -> the largest value that stays itself; anything above becomes that + 1


def signature(family, keys):
    """(family, {key: value}) of one [dispatch] line -> its size-free signature, a string "family key value ..." (keys in the line's
    order); None for the anonymous "kernel" family.  Dropped: M N K B L F n wgs pairs jobs k_chunk and the grid; d stays for the LayerNorm,
    heads and sequence-resident families; splitk becomes 1 or 2 (more than one), riders and phase 0 or 1 (more than none)."""
    if family == "kernel":
        return None
    out = [family]
    for k, v in keys.items():
        if k in KEEP or (k == "d" and family in KEEP_D):
            if k in COLLAPSE:
                v = min(int(v), COLLAPSE[k] + 1)
            out += [k, str(v)]
    return " ".join(out)


def signatures(trace):
    """the signatures of a parsed trace, in order, without the anonymous launches"""
    return [s for s in (signature(f, kv) for f, kv in trace) if s is not None]


# ---- the universe ------------------------------------------------------------------------------------------------------------------
def shape_key(name):
    """sort key of a dispatch_trace.py case name ("d256 H2 F512 L2+0 S16 B64 prec 0 flags 0 ..."): tokens, then d_model, then the rest"""
    f = dict((t[0], t[1:]) for t in name.split()[:6] if t[0] in "dHFSB")
    return (32 * int(f["B"]), int(f["d"]), int(f["F"]), int(f["H"]), name)


_grid = None


def grid_trace():
    """{signature: smallest case name that reaches it} over tools/dispatch_trace.py --grid --dry (cached per process; about 12 s)"""
    global _grid
    if _grid is None:
        from harness import emu_lib, parse_dispatch
        emu_lib()                                 # (re)builds the emulator library when a source is newer
        text = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dispatch_trace.py"), "--dry", "--grid"], check=True,
                              stdout=subprocess.PIPE, universal_newlines=True, env=dict(os.environ, PYTHONPATH=ROOT)).stdout
        found, name, memo = {}, None, {}
        for ln in text.splitlines():
            if ln.startswith("## "):
                name = ln[3:].split(" | ")[0]
            elif ln.startswith("[dispatch] "):
                if ln not in memo:
                    (fam, kv), = parse_dispatch(ln)
                    memo[ln] = signature(fam, kv)
                s = memo[ln]
                if s is not None and (s not in found or shape_key(name) < shape_key(found[s])):
                    found[s] = name
        assert len(found) > 100, len(found)
        _grid = found
    return _grid


def universe():
    """the set of signatures a configuration of the sweep grid can launch (dry trace: the emulator's 256 CUs, an MI355X's count)"""
    return set(grid_trace())


# ---- the seq universe: the sequence-resident kernels at the resolution at which they are instantiated, off the sweep grid too ------------
# The grid has no d_model 48 / 80 / 96 / 112 and forces no schedule, yet the C ABI reaches every instantiation the launchers of
# groove_seq_fwd.hip / groove_seq_bwd.hip / groove_seq64.hip name.  Every (d_model, n_heads) seq_supported admits x the sizes below x the
# library's schedule, SPLIT forced and SPLIT forbidden x every entry-point form that launches these kernels.
SEQ_D = tuple(range(16, 129, 16))
SEQ_F = (16, 48, 256, 512)
SEQ_L = (1, 2)
SEQ_B = (2, 65, 129)                              # 65 / 129: the far sides of the QUAD (4 B <= CUs) and SPLIT (2 B <= CUs) rules at 256 CUs
SEQ_FORCE = ((), (("split", 1),), (("split", 0),))


def seq_models():
    """(d_model, n_heads) of every width 16 ... 128 and head count 1 ... 16 dividing it whose head_dim seq_supported admits"""
    return [(d, H) for d in SEQ_D for H in range(1, 17) if d % H == 0 and (d // H < 16 or d // H in (16, 32, 64))]


def seq_case_name(d, H, F, L, B, force=(), S=16):
    return "d%d H%d F%d L%d+0 S%d B%d prec 0 flags 0%s" % (d, H, F, L, S, B, "".join(" %s %d" % kv for kv in force))


def _seq_child():
    """(child process: GT_EMU_DRY=1 GT_TRACE_DISPATCH=2) "## case" and the seq_* lines of every form, for every case of the enumeration"""
    import ctypes
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    import dispatch_trace as dt
    from transformergrooveinfilling_amd import _lib
    lib = _lib.GrooveLib(os.environ.get("GT_EMU_LIB_PATH") or os.path.join(ROOT, "tests", "emu", "libgroove_emu.so"))
    lib.cdll.gt_set_seq(1)                        # what harness.Runner sets
    drv, s0, pen = dt.Driver(lib, True), ctypes.c_void_p(0), ctypes.c_float(0.5)
    for d, H in seq_models():
        for F in SEQ_F:
            for L in SEQ_L:
                for B in SEQ_B:
                    cfg = _lib.make_config(B, 16, d, H, F, L, 0, dt.DROPOUT, 0, 0)
                    cp, M = ctypes.byref(cfg), 32 * B
                    total, _ = lib.param_layout(cfg)
                    ws, state = drv.buf(lib.workspace_floats(cfg)), drv.state()
                    params, grads, m, v = (drv.buf(total) for _ in range(4))
                    pe, x, y, hvo, d_hvo, tgt, stats = drv.buf(32 * d), drv.buf(M * 16), drv.buf(M * 27), drv.buf(M * 27), drv.buf(M * 27), drv.buf(M * 27), drv.buf(8)
                    c = lib.cdll
                    step = lambda algo, skip: c.gt_train_step(cp, algo, params, grads, m, v, pe, x, y, pen, hvo, stats, tgt, ws, state, skip, s0)
                    for force in SEQ_FORCE:
                        for k, val in force:
                            getattr(c, dt.SETTERS[k])(val)
                        two = len(lib.grad_buckets(cfg)) == 2

                        def forms():
                            rc = [c.gt_workspace_init(cp, ws, s0), c.gt_forward(cp, params, pe, x, None, hvo, ws, state, 1, s0),
                                  c.gt_loss(cp, hvo, y, pen, stats, d_hvo, s0), c.gt_backward(cp, params, grads, x, None, hvo, d_hvo, ws, state, 1, 0, s0),
                                  c.gt_backward(cp, params, grads, x, None, hvo, d_hvo, ws, state, 1, 1, s0), step(0, 0), step(1, 0)]
                            return rc + ([step(1, 2), step(1, 3)] if two else [])
                        rcs, text = dt.traced(forms)
                        for k, _ in force:
                            getattr(c, dt.SETTERS[k])(-1)
                        assert not any(rcs), (d, H, F, L, B, force, rcs, c.gt_last_error())
                        print("## " + seq_case_name(d, H, F, L, B, force))
                        print("\n".join(sorted({ln for ln in text.splitlines() if ln.startswith("[dispatch] seq_")})))
                    drv.keep = []


_seq = None


def seq_trace():
    """{seq_* signature: smallest case name that reaches it} over the enumeration above (dry: the emulator's 256 CUs; cached per process)"""
    global _seq
    if _seq is None:
        from harness import emu_lib, parse_dispatch
        emu_lib()
        text = subprocess.run([sys.executable, os.path.abspath(__file__), "--seq-child"], check=True, stdout=subprocess.PIPE, universal_newlines=True,
                              env=dict(os.environ, PYTHONPATH=ROOT, GT_EMU_DRY="1", GT_TRACE_DISPATCH="2")).stdout
        found, name, memo = {}, None, {}
        for ln in text.splitlines():
            if ln.startswith("## "):
                name = ln[3:]
            elif ln.startswith("[dispatch] seq_"):
                if ln not in memo:
                    (fam, kv), = parse_dispatch(ln)
                    memo[ln] = signature(fam, kv)
                s = memo[ln]
                if s not in found or shape_key(name) < shape_key(found[s]):
                    found[s] = name
        assert len(found) > 50, len(found)
        _seq = found
    return _seq


def seq_universe():
    """the set of seq_* signatures some configuration of the enumeration launches"""
    return set(seq_trace())


# ---- the record file ---------------------------------------------------------------------------------------------------------------
def read_recording(path):
    """a GT_VARIANT_LEDGER file -> {signature: {test id: launches}}"""
    seen = {}
    with open(path) as f:
        for ln in f:
            sig, _, test = ln.rstrip("\n").partition("\t")
            if sig:
                t = seen.setdefault(sig, {})
                t[test] = t.get(test, 0) + 1
    return seen


def node_id(current):
    """$PYTEST_CURRENT_TEST ("tests/test_x.py::test_y[case] (call)", or without "tests/" where that directory is pytest's root) ->
    "tests/test_x.py::test_y[case]" """
    tid = current.rsplit(" (", 1)[0]
    tid = re.sub(r"\[/[^\]]*/", "[", tid)       # (a file parameter: its name without the directory it lay in)
    return tid if tid.startswith("tests/") or not tid else "tests/" + tid


def read_record(path=RECORD):
    """profiles/variant_ledger.txt -> {section: [fields of each line]}; a line is "signature | field | ..." under a "[section]" header"""
    out, sec = {}, None
    with open(path) as f:
        for ln in f:
            ln = ln.rstrip("\n")
            if ln.startswith("[") and ln.endswith("]"):
                sec = out.setdefault(ln[1:-1], [])
            elif ln and not ln.startswith("#") and sec is not None:
                sec.append([x.strip() for x in ln.split(" | ")])
    return out


def compare(record_sigs, uni):
    """(missing, stale): universe signatures the record lacks, record signatures the universe lacks -- both sorted"""
    return sorted(uni - set(record_sigs)), sorted(set(record_sigs) - uni)


def write_record(recording, reasons, times, out):
    """the record file's sections from a recording of the whole GPU suite; reasons: {signature: why it may stay uncovered}; times:
    {case name: seconds} of the gap cases"""
    grid = grid_trace()
    seen = read_recording(recording)
    tests = lambda s: sorted({node_id(t) for t in seen.get(s, {}) if t})
    before = [s for s in sorted(grid) if not [t for t in tests(s) if not t.startswith(GAP_TESTS)]]
    left = [s for s in before if not tests(s)]
    p = lambda *a: out.write(" | ".join(str(x) for x in a) + "\n")
    out.write("[universe]\n# signature | tests that ran it | one of them, or UNCOVERED | (UNCOVERED: smallest grid shape that reaches it | why it stays)\n")
    for s in sorted(grid):
        t = tests(s)
        if t:
            p(s, len(t), t[0])
        else:
            p(s, 0, "UNCOVERED", grid[s], reasons.get(s, "NO REASON"))
    out.write("\n[before]\n# %d of %d signatures had no oracle case before tests/test_variant_ledger_gpu.py: signature | smallest grid shape that reaches it\n" % (len(before), len(grid)))
    for s in before:
        p(s, grid[s])
    out.write("\n[closed]\n# %d of them closed: signature | the case that runs it\n" % (len(before) - len(left)))
    for s in before:
        if tests(s):
            p(s, tests(s)[0])
    out.write("\n[remaining]\n# %d remain: signature | smallest grid shape | reason\n" % len(left))
    for s in left:
        p(s, grid[s], reasons.get(s, "NO REASON"))
    off = [s for s in sorted(seen) if s not in grid]
    out.write("\n[off-grid]\n# %d signatures the suite ran that the grid cannot reach (forced switches, off-grid widths and batches): signature | tests | one of them\n" % len(off))
    for s in off:
        p(s, len(tests(s)), tests(s)[0] if tests(s) else "-")
    out.write("\n[cases]\n# wall time of each gap case on an MI355X (\"seq:\": a case of the seq universe): case | seconds\n")
    for k in sorted(times):
        p(k, "%.1f" % times[k])
    # ---- the seq universe: the same four sections.  "Before": no test but the cases written for it (test_seq_variant, test_seq_before) ran it
    seq = seq_trace()
    mine = lambda t: t.startswith(SEQ_TESTS)
    sbefore = [s for s in sorted(seq) if not [t for t in tests(s) if not mine(t)]]
    sleft = [s for s in sbefore if not tests(s)]
    out.write("\n[seq-universe]\n# signature | tests that ran it | one of them, or UNCOVERED | (UNCOVERED: smallest shape of the enumeration that reaches it | why it stays)\n")
    for s in sorted(seq):
        t = tests(s)
        if t:
            p(s, len(t), ([x for x in t if not mine(x)] or t)[0])
        else:
            p(s, 0, "UNCOVERED", seq[s], reasons.get(s, "NO REASON"))
    out.write("\n[seq-before]\n# %d of %d signatures had no oracle case before %s*: signature | smallest shape that reaches it\n" % (len(sbefore), len(seq), SEQ_TESTS))
    for s in sbefore:
        p(s, seq[s])
    out.write("\n[seq-closed]\n# %d of them closed: signature | the case that runs it\n" % (len(sbefore) - len(sleft)))
    for s in sbefore:
        if tests(s):
            t = tests(s)
            p(s, ([x for x in t if "::test_seq_variant[" in x] or t)[0])
    out.write("\n[seq-remaining]\n# %d remain: signature | smallest shape | reason\n" % len(sleft))
    for s in sleft:
        p(s, seq[s], reasons.get(s, "NO REASON"))


HEADER = """Variant ledger: every launch signature a configuration of the sweep grid can make the library launch, and the oracle case that ran it on an MI355X.
Written by  python tests/variant_ledger.py <recording> [<times>]  from a GT_VARIANT_LEDGER recording of the whole GPU suite (tests/variant_ledger.py
says what a signature is, DESIGN.md 4a what the ledger is for); tests/test_variant_ledger.py holds this file to the dry trace of the grid.

A signature is a [dispatch] line without its sizes.  The universe is the dry trace (emulator build, 256 CUs assumed) of tools/dispatch_trace.py --grid:
d_model 16 ... 512 x heads 1 ... 16 x dim_feedforward 16 ... 2048 x batch 16 ... 512, 2+0 and 2+2 layers, precision 1 / 2 at dim_feedforward >= 512 and
batch 64 / 512, and per model one point each of S 27, of flags = NO_QUAD | NO_LN_XCHG and of gt_set_seq(0) -- 3003 shapes, every entry-point form.
Only launches made through harness.Runner or harness.trace_dispatch count: the ones a parity check compares (StepEngine tests do not).

Limits.  A line says the variant ran inside a comparison with the oracle at least once; it says nothing of every data regime or shape edge within the
variant (DESIGN.md 4a's rule -> boundary -> test table keeps that).  The anonymous "kernel" launches (loss, optimizer, predict head, voice select,
metrics, gather, infill, hit curve) carry no name and are not in the ledger; each has an exact test of its own.

Sections: "universe", one line per signature; "before", the signatures no test ran before tests/test_variant_ledger_gpu.py existed -- the finding;
"closed", the case that now runs each; "remaining", what still has none, with the reason; "off-grid", signatures the suite runs that no grid shape
reaches (forced switches, off-grid widths and batches, SGD: the grid's driver steps with Adam); "cases", the wall time of each new case.

The seq universe ("seq-universe", "seq-before", "seq-closed", "seq-remaining": the same four sections) is the second universe, for the
sequence-resident kernels alone at the resolution at which they are instantiated.  A seq_fwd / seq_bwd signature also names the head-dim class
(hc), whether d_model equals its class 32 / 64 / 128 (exact), the attention form (attn: mfma, mfma-pad, valu) and whether the fused loss rides
in the launch (loss).  Its shapes (tests/variant_ledger.py seq_trace(), dry): every (d_model, heads) pair the path admits -- d_model 16 ... 128
in steps of 16, heads 1 ... 16 dividing it, head_dim < 16 or 16 / 32 / 64: 38 pairs, the widths 48 / 80 / 96 / 112 no grid has among them --
x dim_feedforward 16 / 48 / 256 / 512 x 1 / 2 layers x batch 2 / 65 / 129 (the far sides of the QUAD and SPLIT rules at 256 CUs) x the
library's schedule, gt_set_seq_split(1) and (0) x forward + loss + backward, gt_backward(accumulate 1), gt_train_step under SGD and Adam and
the bucketed step (skip_update 2, 3) where gt_grad_buckets returns 2.  "seq-before": what no test but tests/test_variant_ledger_gpu.py's
test_seq_variant (the table of tests/seq_variants.py) and test_seq_before (one case per remaining signature, at the smallest shape) had run.

Whether those cases bite -- two mutations of csrc/gt_seq.h and what they did to them -- is in profiles/README.md, at this file's line.

"""


def main(argv):
    import importlib
    if argv[1:] == ["--seq-child"]:
        return _seq_child()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    gaps = importlib.import_module("test_variant_ledger_gpu")
    times = {}
    if len(argv) > 2:                             # GT_VARIANT_LEDGER_TIMES file of the same run: "case <tab> seconds"
        for ln in open(argv[2]):
            k, _, v = ln.rstrip("\n").partition("\t")
            times[k] = float(v)
    sys.stdout.write(HEADER)
    write_record(argv[1], gaps.MAY_STAY, times, sys.stdout)


if __name__ == "__main__":
    main(sys.argv)
