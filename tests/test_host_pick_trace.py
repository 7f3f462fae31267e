"""The host dispatch, pinned: tools/dispatch_trace.py --dry (emulator build, no kernel body runs) against profiles/host_pick_trace.txt, and the
per-call record of a refused bf16-only store."""
import ctypes
import os
import subprocess
import sys

import numpy as np

from harness import ROOT, emu_lib
from transformergrooveinfilling_amd import _lib

PROFILE = os.path.join(ROOT, "profiles", "host_pick_trace.txt")


def _body(text):
    """the trace below the file's header: from the first group's line on"""
    return text[text.index("# group "):]


def test_dry_dispatch_trace_matches_the_committed_one():
    """Every launch of every entry-point form over the dispatch-edge, row-exchange, BASELINE (precisions, shadow levels, exchange and flag
    variants, GT_SEQ=0) and reference-YAML shapes, in order, as one line of digests per shape: a change of a dispatch rule has to
    change profiles/host_pick_trace.txt on purpose (regenerate it as its header says; without --digest the tool prints the lines)."""
    emu_lib()                                     # (re)builds the emulator library when a source is newer
    got = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "dispatch_trace.py"), "--dry", "--digest"], check=True,
                         stdout=subprocess.PIPE, universal_newlines=True, env=dict(os.environ, PYTHONPATH=ROOT)).stdout
    g, w = got.splitlines(), _body(open(PROFILE).read()).splitlines()
    assert len(g) > 100, len(g)
    differ = [(a, b) for a, b in zip(g, w) if a != b]
    assert not differ and len(g) == len(w), "%d of %d / %d shapes differ; the first: got %r, the profile has %r" % (
        len(differ), len(g), len(w), differ[0][0] if differ else None, differ[0][1] if differ else None)


def test_refused_store_does_not_outlive_its_call():
    """A call records that a bf16-only tensor met a kernel that cannot take it (a workspace off the 16-byte grid: no bf16-source kernel) and
    then fails on something else before it reports; the next call on the thread, which has nothing to do with either, succeeds."""
    lib = emu_lib()
    os.environ["GT_EMU_DRY"] = "1"                # host side only: no kernel body reads the misplaced workspace
    try:
        c = _lib.make_config(128, 16, 256, 2, 256, 1, 1, 0.1, 1, 0)       # d_model 256 at 4096 tokens, precision 1: operand shadows at level 2
        cp = ctypes.byref(c)
        assert lib.cdll.gt_operand_shadow_level(cp) == 2
        total, _ = lib.param_layout(c)
        ws = np.empty(lib.workspace_floats(c) + 1, np.float32)[1:]
        assert ws.ctypes.data % 16 == 4
        ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
        params, pe, x, hvo, y, stats = (np.zeros(n, np.float32) for n in (total, 32 * 256, 4096 * 16, 4096 * 27, 4096 * 27, 8))
        # the refusal is real: a forward over this workspace reports it
        assert lib.cdll.gt_forward(cp, ptr(params), ptr(pe), ptr(x), ptr(y), ptr(hvo), ptr(ws), None, 0, None) == -1
        assert b"has no bf16-source kernel" in lib.cdll.gt_last_error()
        # gt_predict runs the same encoder, then stops at the missing tgt_scratch: before its launch_status
        assert lib.cdll.gt_predict(cp, ptr(params), ptr(pe), ptr(x), ptr(hvo), ctypes.c_float(0.5), 1, None, ptr(ws), None) == -1
        assert b"needs tgt_scratch" in lib.cdll.gt_last_error()
        rc = lib.cdll.gt_loss(cp, ptr(hvo), ptr(y), ctypes.c_float(0.5), ptr(stats), None, None)
        assert rc == 0, lib.cdll.gt_last_error()
    finally:
        del os.environ["GT_EMU_DRY"]
