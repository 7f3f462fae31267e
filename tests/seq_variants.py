"""Oracle cases for the sequence-resident kernels (csrc/gt_seq.h) at the resolution at which they are instantiated: head-dim class, d_model
against its class, attention form, fused loss (profiles/variant_ledger.txt, section [seq-universe]; DESIGN.md 4a "Variant ledger").  ONE table
for both backends: tests/test_variant_ledger_gpu.py runs every case on the GPU, tests/test_seq_variants.py the small ones on the emulator build
-- the same checks with their bars unchanged, the same asserted trace, so that the non-GPU suite fails first when a host rule moves.

A case is (form, cfg, B, dropout, keywords, want).  form: "step" (parity.check_step), "peaked" (the same through check_step_regime), "sgd" /
"adam" (parity.check_train_step, three fused steps), "probes" (check_grad_probes on the rider cuts, as tests/test_grad_probes_gpu.py's d128
rider case places them), "accumulate" (check_accumulate).  want: what EVERY seq_fwd / seq_bwd line of the case's own trace must say -- split,
quad, ride, hc, exact, attn -- or None: the shape must leave the sequence-resident path (no seq_* line at all).  The batch boundaries assume
256 CUs, an MI355X's count and the emulator's."""
import re

import parity
import variant_ledger as vl
from harness import cfg_dict, dispatched, trace_dispatch

SEQ_FAMILIES = ("seq_pack", "seq_fwd", "seq_bwd", "seq_tail")
# check_train_step's step size.  The check also follows the free-running fp64 trajectory, and Adam moves every live element by about lr per step
# whatever its gradient: an element whose gradient is wrong by e of itself lands lr x e off, so at the default lr 0.05 the free-running bars
# (live elements 1e-3, well-conditioned ones 1e-4, loss 2e-5, ReLU decisions within 1e-5 of the kink) ask more of a small element than GRAD_TOL
# (2e-4 of the tensor's LARGEST entry) grants it.  How much of those bars fp32 arithmetic alone uses is measured per case by
# tools/adam_trajectory_noise.py: ADAM_ORACLE is the fp32 ORACLE's own three-step trajectory at lr 0.05 as its worst fraction of a bar (a ReLU
# decision off the kink counts in units of 1e-5).  A device sums in another order: at d128 / 2 heads / one layer / batch 2 the oracle stands at
# 0.31 of the live-element bar and the kernels -- GPU and emulator alike, an element at 0.35 % of the tensor's largest gradient -- at 2.3.  So a
# case keeps 0.05 where the oracle stays under a TENTH of every bar, and runs at 0.005 (tests/test_regimes.py's TRAIN_LR, for this reason; the
# same measurement there: under 0.77 of every bar at d128 / 16 heads / batch 2, under 0.21 elsewhere) otherwise.  SGD keeps 0.05 everywhere.
# The teacher-forced per-element update check, the proof of a step, does not depend on the trajectory; no bar changes.
ADAM_ORACLE = {
    "fused-d128-H8-B65-adam": 163, "valu-d64-adam": 14, "d128-H8-F16-L1-B129-split1-adam": 10, "fused-d128-H2-B65-adam": 10,
    "d128-H2-F16-L2-B129-split1-adam": 8.11, "d128-H4-F16-L2-B129-split1-adam": 7.98, "fused-d128-H16-B2-adam": 7.68,
    "d128-H16-F256-L1-B2-adam": 3.31, "fused-d128-H16-B65-adam": 2.81, "d128-H8-F16-L1-B2-adam": 2.13, "d128-H8-F16-L1-B2-split0-adam": 2.13,
    "d64-H4-F16-L2-B2-split1-adam": 2.11, "fused-d128-H8-B2-adam": 2.03, "inexact-d96-H3-adam": 1.41, "d128-H16-F16-L1-B2-adam": 1.13,
    "d128-H16-F16-L1-B2-split0-adam": 1.13, "d128-H2-F256-L1-B2-adam": 1.1, "d128-H16-F16-L2-B129-split1-adam": 1.02,
    "d128-H8-F16-L2-B129-split1-adam": 0.77, "valu-d32-adam": 0.54, "fused-d128-H2-B2-adam": 0.52, "inexact-d112-H7-adam": 0.47,
    "d128-H8-F256-L1-B2-adam": 0.42, "inexact-d48-H3-adam": 0.41, "d128-H2-F16-L1-B2-adam": 0.31, "d128-H2-F16-L1-B2-split0-adam": 0.31,
    "d112-H8-F16-L1-B2-adam": 0.19, "d64-H2-F16-L1-B2-adam": 0.18, "d64-H2-F16-L1-B2-split1-adam": 0.18, "d96-H6-F16-L1-B2-adam": 0.17,
    "d64-H1-F16-L2-B2-split1-adam": 0.16, "inexact-d80-H5-adam": 0.15, "d128-H16-F16-L1-B129-split1-adam": 0.14,
    "d128-H2-F16-L1-B129-split1-adam": 0.1, "d96-H8-F16-L1-B2-adam": 0.08, "d64-H8-F16-L1-B2-split1-adam": 0.07, "d80-H8-F16-L1-B2-adam": 0.06,
    "d32-H4-F16-L2-B2-split1-adam": 0.04, "d64-H4-F16-L1-B2-split1-adam": 0.03, "d32-H1-F16-L1-B2-adam": 0.03, "d32-H1-F16-L1-B2-split1-adam": 0.03,
    "d48-H4-F16-L1-B2-adam": 0.02, "d64-H16-F16-L1-B2-adam": 0.02, "d32-H1-F16-L2-B2-split1-adam": 0.02, "d32-H4-F16-L1-B2-split1-adam": 0.02,
    "d32-H2-F16-L1-B2-adam": 0.02, "d32-H2-F16-L1-B2-split1-adam": 0.02, "d32-H16-F16-L1-B2-adam": 0.02, "d64-H8-F16-L2-B2-split1-adam": 0.01,
    "d64-H1-F16-L1-B2-adam": 0.01, "d64-H1-F16-L1-B2-split1-adam": 0.01, "d16-H1-F16-L1-B2-adam": 0,
}
ADAM_ORACLE_MAX = 0.1


def train_lr(case_id, form):
    if form != "adam":
        return 0.05
    assert case_id in ADAM_ORACLE, "%s: no fp32-oracle figure -- run tools/adam_trajectory_noise.py and add it to ADAM_ORACLE" % case_id
    return 0.05 if ADAM_ORACLE[case_id] < ADAM_ORACLE_MAX else 0.005


def want(hc, exact, attn, split=0, quad=0, ride=0):
    return dict(hc=hc, exact=exact, attn=attn, split=split, quad=quad, ride=ride)


def _cases():
    c = {}

    def add(name, form, cfg, B, w, p=0.1, **kw):
        assert name not in c, name
        c[name] = (form, cfg, B, p, kw, w)

    # ---- the fused train step at d_model 128 outside head-dim class 32: no seq_fb_kernel -- the loss rides in a QUAD forward launch with
    # riders behind it and backward phase 0 is a launch of its own (batch 2), or in a two-workgroup SPLIT launch (batch 65: 4 x 65 > 256 CUs)
    # (batch 2 under SGD: tests/test_phase_head_loads_gpu.py::test_phase_heads_d128_gpu[<heads>-2-<dropout>-quad] is this very case -- the recording
    # names it for these signatures -- so only Adam is added there)
    for H, hc, attn in ((16, 0, "mfma-pad"), (8, 16, "mfma"), (2, 64, "mfma")):
        cfg = cfg_dict(128, H, 64, 2)
        for B, quad in ((2, 1), (65, 0)):
            for form in ("sgd", "adam")[int(B == 2):]:
                add("fused-d128-H%d-B%d-%s" % (H, B, form), form, cfg, B, want(hc, 1, attn, 1, quad, 1))
    add("fused-d128-H16-B2-probes", "probes", cfg_dict(128, 16, 64, 2), 2, want(0, 1, "mfma-pad", 1, 1, 1))
    add("fused-d128-H8-B65-probes", "probes", cfg_dict(128, 8, 64, 2), 65, want(16, 1, "mfma", 1, 0, 1))
    add("fused-d128-H2-B2-accumulate", "accumulate", cfg_dict(128, 2, 64, 2), 2, want(64, 1, "mfma", 1, 1, 1))
    add("d128-H1-leaves", "step", cfg_dict(128, 1, 64, 2), 2, None)                      # head_dim 128: not a sequence-resident shape
    # ---- the vector-ALU attention (16 heads of 2 / 4: SPLIT at every dim_feedforward) under the fused step; dropout 0: the keep bits are read and overruled
    for d in (32, 64):
        cfg, w = cfg_dict(d, 16, 64, 2), want(0, 1, "valu", 1)
        add("valu-d%d-sgd" % d, "sgd", cfg, 3, w)
        add("valu-d%d-adam" % d, "adam", cfg, 3, w)
        add("valu-d%d-sgd-p0" % d, "sgd", cfg, 3, w, p=0.0)
        add("valu-d%d-peaked" % d, "peaked", cfg, 3, w)
        add("valu-d%d-peaked-p0" % d, "peaked", cfg, 3, w, p=0.0)
    # ---- zero-padded heads that are no power of two (3, 5, 6, 7, 12), d_model off its class: whole-sequence kernels only (SPLIT: 32 / 64 / 128)
    for d, H in ((48, 16), (80, 16), (96, 16), (112, 16), (48, 4), (96, 8)):
        for L in (1, 2):
            add("pad-d%d-H%d-L%d" % (d, H, L), "step", cfg_dict(d, H, 64, L), 3, want(0, 0, "mfma-pad"))
    # ---- d_model off its class with an exact head class: kernel<DP, 16 / 32, false>
    for d, H, hc in ((96, 3, 32), (48, 3, 16), (80, 5, 16), (112, 7, 16)):
        for form in ("step", "sgd", "adam"):
            add("inexact-d%d-H%d-%s" % (d, H, form), form, cfg_dict(d, H, 64, 2), 3, want(hc, 0, "mfma"))
    # ---- edges inside one instantiation: class 32 at d_model 128 (QUAD, riders, seq_fb_kernel), class 0 at d_model 32 (whole; SPLIT from F 256)
    q128 = lambda quad=1: want(32, 1, "mfma", 1, quad, 1)
    w32 = want(0, 1, "mfma-pad")
    for tag, H, full, part, wide in (("d128", 4, q128(), q128(0), q128()), ("d32", 4, w32, w32, want(0, 1, "mfma-pad", 1))):
        d = int(tag[1:])
        add("edge-%s-L1" % tag, "step", cfg_dict(d, H, 64, 1), 2, full)                  # one layer: pstride = the layer's span, wstride 0
        add("edge-%s-L1-sgd" % tag, "sgd", cfg_dict(d, H, 64, 1), 2, full)
        add("edge-%s-F16" % tag, "step", cfg_dict(d, H, 16, 2), 2, part)                 # (d_model 128: QUAD needs dim_feedforward % 32 == 0)
        add("edge-%s-F48" % tag, "step", cfg_dict(d, H, 48, 2), 2, part)
        add("edge-%s-F512" % tag, "step", cfg_dict(d, H, 512, 2), 2, wide)               # GT_SEQ_FMAX
        add("edge-%s-F528-leaves" % tag, "step", cfg_dict(d, H, 528, 2), 2, None)
        add("edge-%s-S1" % tag, "step", cfg_dict(d, H, 64, 2, embedding_size_src=1), 2, full)
        add("edge-%s-S32" % tag, "step", cfg_dict(d, H, 64, 2, embedding_size_src=32), 2, full)
        add("edge-%s-S33-leaves" % tag, "step", cfg_dict(d, H, 64, 2, embedding_size_src=33), 2, None)
        add("edge-%s-B1" % tag, "step", cfg_dict(d, H, 64, 2), 1, full)
    return c


CASES = _cases()

# the twins the emulator build runs (tests/test_seq_variants.py): d_model <= 64.  Dropped to keep that file under a minute, the largest first:
# every d_model-128 case (the emulator takes 15 ... 40 s for a fused step, the probes or the accumulation at batch 2 and 3 ... 14 s for a plain
# step), and of the 4 ... 5 s ones valu-d64-adam and valu-d64-sgd-p0 (valu-d64-sgd stays) and inexact-d48-H3-sgd / -adam (-step stays).  Of the
# cases written from the recording (before_cases) that file keeps d_model <= 32; the d48 / d64 ones take 1.3 ... 4 s each, 60 s together.
EMU_DROPPED = ("valu-d64-adam", "valu-d64-sgd-p0", "inexact-d48-H3-sgd", "inexact-d48-H3-adam")
EMU_TWINS = [k for k, (form, cfg, B, p, kw, w) in CASES.items() if cfg["d_model"] <= 64 and k not in EMU_DROPPED]


def _rider_places(trace, M):
    return parity.probe_places(M // 32, parity.rider_rows(M))


def shape_case(shape, form):
    """a case of this module's form from a case name of variant_ledger.seq_trace() ("d128 H16 F16 L1+0 S16 B129 prec 0 flags 0 split 1"): the
    enumeration's dropout (0.1) and its forcing -- gt_set_seq_split(1 / 0) is harness.Runner's seq="split" / "whole"."""
    m = re.match(r"d(\d+) H(\d+) F(\d+) L(\d+)\+0 S(\d+) B(\d+) prec 0 flags 0(?: split ([01]))?$", shape)
    assert m, shape
    d, H, F, L, S, B = (int(v) for v in m.groups()[:6])
    kw = {} if m.group(7) is None else dict(seq="split" if m.group(7) == "1" else "whole")
    return (form, cfg_dict(d, H, F, L, embedding_size_src=S), B, 0.1, kw, None)


def shape_id(shape, form):
    t = shape.split()
    return "-".join(t[:2] + [t[2], t[3].split("+")[0], t[5]] + ["%s%s" % kv for kv in zip(t[10::2], t[11::2])] + [form])


def forms_of(sig):
    """the forms that run a signature of the seq universe: the fused step, under SGD and Adam, where the launch carries the loss or follows the
    fused forward / backward-phase-0 launch; forward, loss and backward as three calls otherwise"""
    return ("sgd", "adam") if (" loss 1" in sig or " fuse_b0 1" in sig) else ("step",)


def before_cases():
    """The cases written from the recording: id -> (case, signatures it is the oracle case of).  One per smallest shape (and form, forms_of) of
    the signatures in [seq-before] of profiles/variant_ledger.txt that no case of CASES runs -- the record's [seq-closed] names the case that
    does, so a re-recording of the whole suite reproduces this list."""
    rec = vl.read_record()
    fixed = {ln[0] for ln in rec["seq-closed"] if "::test_seq_variant[" in ln[1]}        # (a missing or renamed section is a KeyError, not an empty list)
    out = {}
    for ln in rec["seq-before"]:
        sig, shape = ln[0], ln[1]
        if sig not in fixed:
            for form in forms_of(sig):
                out.setdefault(shape_id(shape, form), (shape_case(shape, form), []))[1].append(sig)
    assert out, "no generated case: [seq-before] of the record is empty or every line of it is closed by the table"
    return out


QUAD_B0 = dict(hc=32, attn="none")                       # what the QUAD launch of backward phase 0 says: seq_bwd_kernel<128, 32, true, true, true>


def check_lines(trace, sig):
    """a generated case's trace: the signature ran, and EVERY seq_fwd / seq_bwd line of the trace names the signature's instantiation, attention
    form and split -- a case runs one model on one schedule -- but for the QUAD launch of backward phase 0, which says QUAD_B0"""
    assert ran(trace, sig), "not launched: %s\nlaunched: %s" % (sig, sorted(set(vl.signatures(trace))))
    tok = sig.split()
    kv = {k: (int(v) if v.isdigit() else v) for k, v in zip(tok[1::2], tok[2::2])}
    if tok[0] not in ("seq_fwd", "seq_bwd") or (tok[0] == "seq_bwd" and kv["quad"]):
        return
    want = {k: kv[k] for k in ("hc", "exact", "attn", "split", "d")}
    for fam, d in trace:
        if fam in ("seq_fwd", "seq_bwd") and not (fam == "seq_bwd" and d["quad"]):
            assert {k: d[k] for k in want} == want, (d, want)


def ran(trace, sig):
    """the trace's lines with this signature: harness.dispatched on the keys the signature keeps as they are, signature() on the rest"""
    tok = sig.split()
    fam, kv = tok[0], {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in zip(tok[1::2], tok[2::2])}
    exact = {k: v for k, v in kv.items() if k not in vl.COLLAPSE}
    return [d for d in dispatched(trace, fam, **exact) if vl.signature(fam, d) == sig]


def run(backend, case, case_id=None):
    """the case's check (a name of CASES, or a case itself with its id) under a dispatch trace -> the trace of every launch it made"""
    form, cfg, B, p, kw, w = CASES[case] if isinstance(case, str) else case
    case_id = case if isinstance(case, str) else case_id
    if form == "step":
        fn = lambda: parity.check_step(backend, cfg, B, p, **kw)
    elif form == "peaked":
        fn = lambda: parity.check_step(backend, cfg, B, p, regime="peaked", **kw)
    elif form in ("sgd", "adam"):
        fn = lambda: parity.check_train_step(backend, cfg, B, p, algo=int(form == "adam"), lr=train_lr(case_id, form), **kw)
    elif form == "probes":
        fn = lambda: parity.check_grad_probes(backend, cfg, B, p, _rider_places, **kw)[1]
    else:
        fn = lambda: parity.check_accumulate(backend, cfg, B, p, **kw)
    own, trace = trace_dispatch(fn)
    return trace + own if form == "probes" else trace      # (check_grad_probes traces its own full step: those lines do not reach this trace)


def check_trace(name, trace):
    """the case's trace says what the table says: the instantiation, the attention form and the schedule on every seq_fwd / seq_bwd line, the
    fused loss exactly on the launches of a fused step that run the output layer -- or no seq_* line at all.  Returns the seq_* signatures."""
    form, cfg, B, p, kw, w = CASES[name]
    seq = dispatched(trace, SEQ_FAMILIES)
    if w is None:
        assert not seq, seq
        return set()
    fwd, bwd, L = dispatched(trace, "seq_fwd"), dispatched(trace, "seq_bwd"), cfg["num_encoder_layers"]
    assert fwd and bwd, sorted({f for f, _ in trace})
    inst = {k: w[k] for k in ("hc", "exact", "attn")}
    for d in fwd:
        assert {k: d[k] for k in w} == w and d["d"] == cfg["d_model"], (d, w)
    for d in bwd:
        quad_b0 = d["phase"] == 0 and w["quad"]               # ONE instantiation for every class, and no attention in that phase
        assert {k: d[k] for k in inst} == (dict(QUAD_B0, exact=1) if quad_b0 else inst) and d["split"] == w["split"] and d["ride"] == w["ride"], (d, w)
        assert d["quad"] == (w["quad"] if d["phase"] == 0 else 0), (d, w)
    last = [d for d in fwd if d["phase"] == (L - 1 if w["split"] else 0)]
    fused = form in ("sgd", "adam")
    assert last and all(d["loss"] == int(fused) for d in last) and not [d for d in fwd if d["loss"] and d not in last], fwd
    fb = bool(fused and w["quad"] and w["ride"] and w["hc"] == 32)       # seq_fb_kernel: class 32 alone
    assert all(d["fuse_b0"] == int(fb) for d in last) and all(d["fuse_b0"] == int(fb) for d in bwd), (fwd, bwd)
    return {s for s in vl.signatures(trace) if s.split()[0] in SEQ_FAMILIES}
