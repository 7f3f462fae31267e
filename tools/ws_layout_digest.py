#!/usr/bin/env python
"""Digest of everything gt_workspace_bytes / gt_ws_find answer over a grid of configurations (host functions only: runs on the
emulator library as well as on the HIP one).  Two builds lay the workspace out alike iff their digests are equal:

    tests/emu/build_emu.sh && python tools/ws_layout_digest.py tests/emu/libgroove_emu.so

"numbers": the workspace size of every configuration and the return code, offset and count of every (name, layer) asked.
"texts": the error text of every failing lookup whose layer is one of the model's (outside that range only the return code is part of
the contract).  --dump writes one line per record, for diffing two builds that disagree."""
import argparse
import ctypes
import hashlib
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformergrooveinfilling_amd import _lib  # noqa: E402

SHAPES = [(32, 4, 16), (32, 16, 64), (64, 16, 256), (128, 4, 512), (128, 4, 40), (256, 4, 512), (256, 16, 1024), (512, 8, 2048),
          (512, 4, 512), (96, 6, 96)]                          # d_model, heads, dim_ff
BATCH_SRC = [(1, 16), (3, 16), (16, 16), (64, 16), (512, 16), (3, 27), (3, 40)]
LAYERS = [(1, 0), (2, 0), (6, 0), (2, 2)]
PUBLIC = ("x0 a0 enc_xhat enc_rstd memory y0 b0 dec_final dlogits dmem dctx seq_xchg rowx amask pack_f pack_b stamps "
          "dzA dzAm dzB dzBm dzC dzCm dhid dqkv dqkvx "
          "qkv P ctx xhat1 rstd1 x1 qx kvx Px ctxx xhatx rstdx x2 hact xhat2 rstd2 xout").split()
PRIVATE = "loss_part ln_part da0_dec hvo_tmp dec_xhat dec_rstd seq_dctx kbits wT".split()
NAMES = PUBLIC + [n + "16" for n in PUBLIC] + ["w16", "w16t", "xchg_err", "xchg_err16"] + PRIVATE + ["nope", "", "16"]
ASK_LAYERS = (-1, 0, 1, 2, 5, 6)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lib", help="libgroove_hip.so or the emulator build")
    ap.add_argument("--dump", help="write every record to this file")
    a = ap.parse_args()
    lib = _lib.GrooveLib(a.lib)
    numbers, texts = hashlib.sha256(), hashlib.sha256()
    dump = open(a.dump, "w") if a.dump else None
    n_cfg = n_ask = n_ok = 0
    off, cnt = ctypes.c_int64(), ctypes.c_int64()
    for level in (0, 1, 2):
        lib.cdll.gt_set_operand_shadows(level)
        for (d, H, F), (B, S), (L, Ld), prec, drop in itertools.product(SHAPES, BATCH_SRC, LAYERS, (0, 1, 2), (0.0, 0.1)):
            c = _lib.make_config(B, S, d, H, F, L, Ld, drop, prec)
            key = "s%d d%d H%d F%d B%d S%d L%d+%d p%d drop%g" % (level, d, H, F, B, S, L, Ld, prec, drop)
            rec = "%s bytes %d\n" % (key, lib.cdll.gt_workspace_bytes(ctypes.byref(c)))
            numbers.update(rec.encode())
            if dump:
                dump.write(rec)
            n_cfg += 1
            for name, layer in itertools.product(NAMES, ASK_LAYERS):
                off.value = cnt.value = -7
                rc = lib.cdll.gt_ws_find(ctypes.byref(c), name.encode(), layer, ctypes.byref(off), ctypes.byref(cnt))
                rec = "%s %r %d -> %d %d %d\n" % (key, name, layer, rc, off.value, cnt.value)
                numbers.update(rec.encode())
                n_ask += 1
                n_ok += rc == 0
                err = ""
                if rc != 0 and 0 <= layer < L + Ld:
                    err = "%s %r %d: %s\n" % (key, name, layer, lib.cdll.gt_last_error().decode())
                    texts.update(err.encode())
                if dump:
                    dump.write(rec + err)
    lib.cdll.gt_set_operand_shadows(-1)
    print("configurations %d (x 3 shadow levels included)  names %d  layers %d  lookups %d  answered %d" %
          (n_cfg, len(NAMES), len(ASK_LAYERS), n_ask, n_ok))
    print("numbers sha256 %s" % numbers.hexdigest())
    print("texts   sha256 %s" % texts.hexdigest())


if __name__ == "__main__":
    main()
