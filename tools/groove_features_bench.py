"""What the groove-descriptor pass costs (gt_groove_features; include/groove_hip.h), over 1024 and 16384 sequences:
  gt_groove_features, buffer a only (one record per sequence)
  gt_groove_features, a + b, all three outputs (two records and the pair words)
  gt_groove_features, a + b with feat_b NULL (the ground truth's records are known: the per-epoch call of train.py --eval_descriptors)
  gt_group_metrics with 1 group and seq_out on the same two buffers  -- the yardstick: the existing pass that reads the same bytes
HIP events around each timed sample, the median of --reps samples after warm-up, the compared calls alternating; a sample is --inner
back-to-back calls (one call is tens of microseconds).
usage: python tools/groove_features_bench.py [--out FILE]   (one GPU)"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tools.group_metrics_bench import grooves  # noqa: E402
from tools.voice_select_bench import _ptr, timed  # noqa: E402
from transformergrooveinfilling_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls per timed sample")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    lib = _lib.get_lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = ["groove_features_bench: median of %d samples (HIP events), %d back-to-back calls per sample" % (args.reps, args.inner),
             "device: %s" % torch.cuda.get_device_name(0)]
    for n in (1024, 16384):
        p_np, g_np = grooves(n)
        pred, gt = torch.from_numpy(p_np).cuda(), torch.from_numpy(g_np).cuda()
        fa, fb = (torch.empty(n, _lib.GF_WORDS, dtype=torch.int64, device="cuda") for _ in range(2))
        pw = torch.empty(n, _lib.GF_PAIR_WORDS, dtype=torch.int64, device="cuda")
        acc = torch.zeros(_lib.gm_acc_words(1), dtype=torch.int64, device="cuda")
        seq = torch.empty(n, 4, dtype=torch.int32, device="cuda")
        scratch = torch.empty(int(lib.cdll.gt_group_metrics_scratch_words(ctypes.c_int64(n), 1)), dtype=torch.int64, device="cuda")

        def features(b, want_fb, want_pair):
            return lambda: lib.call("gt_groove_features", _ptr(pred), _ptr(gt) if b else None, ctypes.c_int64(n), _ptr(fa),
                                    _ptr(fb) if want_fb else None, _ptr(pw) if want_pair else None, stream)

        def group_metrics():
            lib.call("gt_group_metrics", _ptr(pred), _ptr(gt), None, None, ctypes.c_int64(n), 1, _ptr(acc), _ptr(seq), _ptr(scratch), stream)

        t = timed({"a": features(False, False, False), "ab": features(True, True, True), "ab_no_fb": features(True, False, True),
                   "yardstick": group_metrics}, args.reps, args.inner)
        read = n * 2.0 * 32 * 27 * 4
        lines += ["%d sequences (the two buffers: %.1f MB):" % (n, read / 1e6)]
        for key, what, nbuf in (("a", "a only                  ", 1), ("ab", "a + b, all three outputs", 2), ("ab_no_fb", "a + b, feat_b NULL      ", 2)):
            lines += ["  gt_groove_features, %s %9.4f ms/call   (%.2f of the yardstick; %.2f TB/s of input)" % (
                what, t[key], t[key] / t["yardstick"], read * nbuf / 2 / t[key] / 1e9)]
        lines += ["  gt_group_metrics, 1 group, seq_out, same buffers %9.4f ms/call   (the yardstick)" % t["yardstick"]]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
