#!/usr/bin/env python3
"""dispatch_trace.py -- the host dispatch of every entry-point form, over the shapes the dispatch rules split on, as one text.

Drives the C ABI directly (no engine, no parity check) with GT_TRACE_DISPATCH=2 GT_TRACE_GEMM64=1 and prints, per shape and form, a
"## shape | form" marker followed by the library's trace lines.  Two builds that print the same text make the same launches in the same
order: a change of host code that is meant to move no launch is checked by comparing this output before and after.

    python tools/dispatch_trace.py --dry [--digest] > trace.txt     # emulator build, GT_EMU_DRY=1: no kernel body runs (no GPU needed)
    python tools/dispatch_trace.py > trace.txt                      # the HIP library (GT_LIB_PATH: another build) on the current device
    python tools/dispatch_trace.py --dry --grid > grid.txt          # the sweep grid (grid_groups) in full: tests/variant_ledger.py's universe

--dry assumes the emulator's 256 CUs; the numbers left in the buffers are garbage either way (nothing here reads them).  A block that
repeats an earlier block line for line, of whichever shape, is printed as "= <that block's marker>".  --digest prints one line per shape
instead -- for each form in order its line count and the head of the sha256 of its lines: what profiles/host_pick_trace.txt keeps and
tests/test_host_pick_trace.py compares (the whole text is 1.3 MB; it takes about a second to print again).

Groups run in child processes: GT_SEQ and the shape-by-measurement default of gt_set_seq are per process."""
import argparse
import ctypes
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from transformergrooveinfilling_amd import _lib  # noqa: E402

FALLBACK = _lib.CFG_NO_QUAD | _lib.CFG_NO_LN_XCHG
DROPOUT = 0.1


def shape(d, H, F, L, Ld=0, S=16):
    return dict(d=d, H=H, F=F, L=L, Ld=Ld, S=S)


C4_1 = shape(512, 8, 512, 1)
KS_1 = shape(256, 2, 512, 1)
LM_1 = shape(256, 2, 2048, 1)
ENCDEC_1 = shape(256, 2, 512, 1, 1)
D128 = shape(128, 4, 64, 2)
BASELINE = [(C4_1, 64), (C4_1, 256), (C4_1, 512), (ENCDEC_1, 256)]
YAMLS = [(KS_1, 32), (shape(32, 16, 64, 1), 16)]


def case(sh, B, precision=0, flags=0, **switch):
    """switch: split / quad / ride / ln_xchg / shadows -> the gt_set_* of that name (put back to -1 after the case)"""
    return dict(sh=sh, B=B, precision=precision, flags=flags, switch=switch)


def edge_cases(cus):
    """every shape and switch / flag combination of tests/test_dispatch_edges_gpu.py, then the row-exchange cases of tests/test_hip_parity.py"""
    c = [case(shape(128, 4, 512, 3), 64, flags=FALLBACK), case(shape(128, 4, 512, 3), 64, split=1, quad=0)]
    c += [case(C4_1, 64, precision=p, flags=FALLBACK) for p in (0, 1, 2)]
    c += [case(KS_1, B, flags=FALLBACK) for B in (256, 512, 32)] + [case(ENCDEC_1, 64, flags=FALLBACK)]
    c += [case(LM_1, B) for B in (33, 129, 130, 131)] + [case(C4_1, B) for B in (43, 65, 66)] + [case(KS_1, 513)]
    c += [case(shape(96, 2, 2048, 1), 63), case(LM_1, 129, precision=1), case(C4_1, 65, precision=1), case(C4_1, 65, precision=2)]
    c += [case(D128, B) for B in (cus // 4, cus // 4 + 1, (cus - 96) // 2, (cus - 96) // 2 + 1, cus // 2, cus // 2 + 1)]
    c += [case(dict(D128, S=27), cus // 4 + 1)]
    c += [case(sh, cus // 2 + past) for sh in (shape(32, 16, 64, 2), shape(64, 16, 256, 2)) for past in (0, 1)]
    c += [case(shape(32, 4, 16, 2), 4), case(shape(32, 4, 16, 2, 2), 3)]
    # row exchange: 64x64 tiles (forced on), the big tile, the generic kernel's 32x32 tiles
    c += [case(C4_1, 64, ln_xchg=1), case(shape(256, 2, 512, 2), 64, ln_xchg=1), case(dict(C4_1, S=27), 64, precision=1, ln_xchg=1)]
    c += [case(C4_1, 256), case(C4_1, 512), case(dict(C4_1, S=27), 256, precision=1), case(C4_1, 256, precision=2)]
    c += [case(shape(256, 2, 512, 6), 32), case(shape(256, 16, 64, 2), 16), case(shape(256, 2, 512, 2), 32)]
    return c


def groups(cus):
    """name -> (environment, gt_set_seq argument or None, cases)"""
    g = {}
    g["edges"] = ({}, 1, edge_cases(cus))
    g["precision"] = ({}, None, [case(sh, B, precision=p) for sh, B in BASELINE for p in (0, 1, 2)] + [case(sh, B) for sh, B in YAMLS])
    g["shadows"] = ({}, None, [case(sh, B, precision=p, shadows=lv) for sh, B in BASELINE for p in (1, 2) for lv in (0, 1, 2)])
    g["exchange"] = ({}, None, [case(sh, B, ln_xchg=v) for sh, B in BASELINE for v in (-1, 0, 1)] +
                     [case(sh, B, flags=FALLBACK) for sh, B in BASELINE])
    g["GT_SEQ=0"] = ({"GT_SEQ": "0"}, None, [case(sh, B) for sh, B in BASELINE + YAMLS])
    return g


GRID_D = (16, 32, 64, 128, 256, 512)
GRID_H = (1, 2, 4, 8, 16)
GRID_F = (16, 64, 256, 512, 2048)
GRID_B = (16, 32, 64, 128, 256, 512)


def grid_groups():
    """The reference's sweep grid for tests/variant_ledger.py's universe(), one group per d_model (--grid runs them side by
    side): d_model x heads x dim_feedforward x batch, encoder-only (2+0) and encoder-decoder (2+2), precision 1 / 2 at dim_feedforward >= 512
    and batch 64 / 512, and per model (d_model, heads, dim_feedforward, layers) one point each of S 27 and of the time-out fall-back flags,
    both at batch 64.  gt_set_seq(1), what tests/harness.py's Runner sets; "grid-seq0" is gt_set_seq(0) at batch 64 of every model.
    Same form: name -> (environment, gt_set_seq argument, cases).  A dry run assumes 256 CUs (an MI355X's count): the batch boundaries of
    the sequence-resident schedules are where that count puts them."""
    g = {}
    models = lambda d: [shape(d, H, F, 2, Ld) for H in GRID_H if d % H == 0 for F in GRID_F for Ld in (0, 2)]
    for d in GRID_D:
        c = [case(sh, B) for sh in models(d) for B in GRID_B]
        c += [case(sh, B, precision=p) for sh in models(d) if sh["F"] >= 512 for B in (64, 512) for p in (1, 2)]
        c += [case(dict(sh, S=27), 64) for sh in models(d)] + [case(sh, 64, flags=FALLBACK) for sh in models(d)]
        g["grid-d%d" % d] = ({}, 1, c)
    g["grid-seq0"] = ({}, 0, [case(sh, 64) for d in GRID_D for sh in models(d)])
    return g


SETTERS = dict(split="gt_set_seq_split", quad="gt_set_seq_quad", ride="gt_set_seq_ride", ln_xchg="gt_set_ln_exchange",
               shadows="gt_set_operand_shadows")


class Driver:
    def __init__(self, lib, dry):
        self.lib, self.dry, self.keep = lib, dry, []
        if not dry:
            import torch
            self.torch = torch

    def buf(self, n, dtype="f4"):
        """n elements the library may read or write; returns the pointer (the holder lives until the case ends)"""
        if self.dry:
            import numpy as np
            a = np.empty(max(int(n), 1), dtype)       # (never touched by a dry launch: no page is committed)
            self.keep.append(a)
            return ctypes.c_void_p(a.ctypes.data)
        t = self.torch.zeros(max(int(n), 1), dtype={"f4": self.torch.float32, "u1": self.torch.uint8}[dtype], device="cuda")
        self.keep.append(t)
        return ctypes.c_void_p(t.data_ptr())

    def state(self):
        st = bytes(_lib.GtStepState(1234, 99, 0, 0, 0.01, 1.0, 0.9, 0.999, 1e-8))
        if self.dry:
            b = ctypes.create_string_buffer(st, len(st))
            self.keep.append(b)
            return ctypes.cast(b, ctypes.c_void_p)
        t = self.torch.frombuffer(bytearray(st), dtype=self.torch.uint8).cuda()
        self.keep.append(t)
        return ctypes.c_void_p(t.data_ptr())

    def run_case(self, c):
        lib, sh, B = self.lib.cdll, c["sh"], c["B"]
        cfg = _lib.make_config(B, sh["S"], sh["d"], sh["H"], sh["F"], sh["L"], sh["Ld"], DROPOUT, c["precision"], c["flags"])
        for k, v in c["switch"].items():
            getattr(lib, SETTERS[k])(v)
        name = "d%d H%d F%d L%d+%d S%d B%d prec %d flags %d%s" % (sh["d"], sh["H"], sh["F"], sh["L"], sh["Ld"], sh["S"], B, c["precision"], c["flags"],
                                                                "".join(" %s %d" % kv for kv in sorted(c["switch"].items())))
        try:
            self.forms(name, cfg, sh, B)
        finally:
            for k in c["switch"]:
                getattr(lib, SETTERS[k])(-1)
            if not self.dry:
                self.torch.cuda.synchronize()
            self.keep = []

    def forms(self, name, cfg, sh, B):
        lib, M, cp, s0 = self.lib, 32 * B, ctypes.byref(cfg), ctypes.c_void_p(0)
        total, _ = lib.param_layout(cfg)
        ws = self.buf(lib.workspace_floats(cfg))
        params, grads, m, v = (self.buf(total) for _ in range(4))
        pe, x, y, hvo, d_hvo, tgt = self.buf(32 * sh["d"]), self.buf(M * sh["S"]), self.buf(M * 27), self.buf(M * 27), self.buf(M * 27), self.buf(M * 27)
        stats, vstats, scratch = self.buf(8), self.buf(64), self.buf(lib.cdll.gt_loss_scratch_floats(cp))
        state, lo = self.state(), _lib.make_loss_opts()
        tgt_in = tgt if sh["Ld"] else None
        step = lambda skip: lib.cdll.gt_train_step(cp, 1, params, grads, m, v, pe, x, y, ctypes.c_float(0.5), hvo, stats, tgt, ws, state, skip, s0)
        forms = [
            ("gt_workspace_init + gt_forward", lambda: [lib.cdll.gt_workspace_init(cp, ws, s0), lib.cdll.gt_forward(cp, params, pe, x, tgt_in, hvo, ws, state, 1, s0)]),
            ("gt_loss", lambda: [lib.cdll.gt_loss(cp, hvo, y, ctypes.c_float(0.5), stats, d_hvo, s0)]),
            ("gt_backward accumulate 0", lambda: [lib.cdll.gt_backward(cp, params, grads, x, tgt_in, hvo, d_hvo, ws, state, 1, 0, s0)]),
            ("gt_backward accumulate 1", lambda: [lib.cdll.gt_backward(cp, params, grads, x, tgt_in, hvo, d_hvo, ws, state, 1, 1, s0)]),
            ("gt_train_step", lambda: [step(0)]),
            ("gt_train_step skip_update 1 + gt_optimizer_step_ws", lambda: [step(1), lib.cdll.gt_optimizer_step_ws(cp, 1, params, grads, m, v, ws, state, 1, s0)]),
            ("gt_train_step skip_update 2, 3", lambda: [step(2), step(3)]),
            ("gt_train_step_loss", lambda: [lib.cdll.gt_train_step_loss(cp, 1, params, grads, m, v, pe, x, y, ctypes.byref(lo), vstats, scratch, hvo, stats, tgt, ws, state, 0, s0)]),
        ]
        if sh["Ld"]:
            forms.append(("gt_predict", lambda: [lib.cdll.gt_predict(cp, params, pe, x, hvo, ctypes.c_float(0.5), 1, tgt, ws, s0)]))
        for form, fn in forms:
            rcs, text = traced(fn)
            print("## %s | %s" % (name, form))
            for ln in text.splitlines():
                if ln.startswith("["):
                    print(ln)
            for rc in rcs:
                if rc != 0:
                    print("rc %d: %s" % (rc, lib.cdll.gt_last_error().decode()))
        sys.stdout.flush()


def traced(fn):
    """fn() with file descriptor 2 in a temporary file (the library writes its trace with fprintf); returns (fn's result, the text)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")


def fold(text, seen, digest):
    """print a group's output.  A block whose lines repeat an earlier block's (of any shape or group) becomes "= <that block's marker>";
    digest: ONE line per shape instead, "## shape | <lines>:<first 16 hex digits of their sha256>" for each of its forms in order"""
    blocks = []
    for ln in text.splitlines():
        if ln.startswith("#"):
            blocks.append([ln])
        else:
            blocks[-1].append(ln)
    case = None
    for b in blocks:
        body = "\n".join(b[1:])
        if digest and b[0].startswith("## "):
            name = b[0].split(" | ")[0]
            sys.stdout.write(("" if name == case else ("\n" if case else "") + name + " |") + " %d:%s" % (len(b) - 1, hashlib.sha256(body.encode()).hexdigest()[:16]))
            case = name
        elif not b[0].startswith("## "):
            print("\n".join(b))
        elif body and body in seen:
            print("%s\n= %s" % (b[0], seen[body]))
        else:
            seen[body] = b[0]
            print("\n".join(b))
    if case:
        print()
    sys.stdout.flush()


def run_group(name, dry):
    if dry:
        path = os.environ.get("GT_EMU_LIB_PATH") or os.path.join(ROOT, "tests", "emu", "libgroove_emu.so")
        lib, cus = _lib.GrooveLib(path), 256
    else:
        import torch
        lib, cus = _lib.get_lib(), torch.cuda.get_device_properties(0).multi_processor_count
    _, seq, cases = (grid_groups() if name.startswith("grid-") else groups(cus))[name]
    if seq is not None:
        lib.cdll.gt_set_seq(seq)
    print("# group %s: CUs %d%s" % (name, cus, "" if seq is None else ", gt_set_seq(%d)" % seq))
    drv = Driver(lib, dry)
    for c in cases:
        drv.run_case(c)


def run_grid(dry):
    """every group of grid_groups(), each in a child process; dry: all of them at once (host code only, one CPU each)"""
    e = dict(os.environ, GT_TRACE_DISPATCH="2", GT_TRACE_GEMM64="1", **({"GT_EMU_DRY": "1"} if dry else {}))
    cmd = lambda name: [sys.executable, os.path.abspath(__file__), "--group", name] + (["--dry"] if dry else [])
    names = list(grid_groups())
    if not dry:
        for name in names:
            sys.stdout.write(subprocess.run(cmd(name), env=e, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout)
        return
    outs = [tempfile.TemporaryFile(mode="w+") for _ in names]
    procs = [subprocess.Popen(cmd(name), env=e, stdout=f) for name, f in zip(names, outs)]
    for name, pr, f in zip(names, procs, outs):
        if pr.wait() != 0:
            raise SystemExit("group %s: exit status %d" % (name, pr.returncode))
        f.seek(0)
        sys.stdout.write(f.read())
        f.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dry", action="store_true", help="the emulator build with GT_EMU_DRY=1")
    ap.add_argument("--digest", action="store_true", help="one line per shape: line count and head of the sha256 of each form's block")
    ap.add_argument("--grid", action="store_true", help="the sweep grid of grid_groups() instead of the groups above, every block in full")
    ap.add_argument("--group", help="(internal) run one group in this process")
    a = ap.parse_args()
    if a.group:
        return run_group(a.group, a.dry)
    if a.grid:
        return run_grid(a.dry)
    seen = {}
    for name, (env, _, _) in groups(256).items():
        e = dict(os.environ, GT_TRACE_DISPATCH="2", GT_TRACE_GEMM64="1", **env)
        if a.dry:
            e["GT_EMU_DRY"] = "1"
        cmd = [sys.executable, os.path.abspath(__file__), "--group", name] + (["--dry"] if a.dry else [])
        fold(subprocess.run(cmd, env=e, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout, seen, a.digest)


if __name__ == "__main__":
    main()
