"""What the per-group counting pass costs (gt_group_metrics; include/groove_hip.h), over 1024 and 16384 sequences:
  gt_group_metrics with 1 and with 64 groups, without and with a cell mask (random words), with seq_out
  gt_voice_metrics on the same two buffers           \\  the yardstick: the two existing passes over the same buffers whose numbers
  gt_hit_curve at one threshold on the same buffers  /  (hit accuracy, MSEs; TP / FP / FN at one threshold) this pass can stand in for
All of them read the same 2 x 27 floats per row.  HIP events around each timed sample, the median of --reps samples after warm-up, the
compared calls alternating; a sample is --inner back-to-back calls (one call is tens of microseconds).
usage: python tools/group_metrics_bench.py [--out FILE]   (one GPU)"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.voice_select_bench import _ptr, timed  # noqa: E402
from transformergrooveinfilling_amd import _lib  # noqa: E402

HIT_RATES = [.25, .2, .5, .05, .02, .02, .02, .01, 0]


def grooves(n_seq, seed=0):
    """(hvo_pred, hvo_gt) (n_seq * 32, 27): the construction of tests/test_group_metrics.py without the planted values"""
    rng = np.random.default_rng(seed)
    M = n_seq * 32
    y = rng.random((M, 9)) < np.array(HIT_RATES)[None, :]
    ph = np.where(y, rng.random((M, 9)) < 0.7, rng.random((M, 9)) < np.array(HIT_RATES)[None, :] * 0.5)
    gt, pred = np.zeros((M, 27), np.float32), np.zeros((M, 27), np.float32)
    gt[:, :9], pred[:, :9] = y, ph
    gt[:, 9:18] = rng.random((M, 9)) * y
    gt[:, 18:] = (rng.random((M, 9)) - 0.5) * y
    pred[:, 9:18] = rng.random((M, 9))
    pred[:, 18:] = rng.random((M, 9)) - 0.5
    return pred, gt


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
    cgrid = (ctypes.c_float * 1)(0.5)
    lines = ["group_metrics_bench: median of %d samples (HIP events), %d back-to-back calls per sample" % (args.reps, args.inner),
             "device: %s" % torch.cuda.get_device_name(0)]
    for n in (1024, 16384):
        M = n * 32
        p_np, g_np = grooves(n)
        pred, gt = torch.from_numpy(p_np).cuda(), torch.from_numpy(g_np).cuda()
        rng = np.random.default_rng(1)
        tag = {k: torch.from_numpy(rng.integers(0, k, n).astype(np.int32)).cuda() for k in (1, 64)}
        cells = torch.from_numpy(rng.integers(0, 1 << 32, (n, 9), dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
        seq = torch.empty(n, 4, dtype=torch.int32, device="cuda")
        acc = {k: torch.zeros(_lib.gm_acc_words(k), dtype=torch.int64, device="cuda") for k in (1, 64)}
        words = {k: int(lib.cdll.gt_group_metrics_scratch_words(ctypes.c_int64(n), k)) for k in (1, 64)}
        scratch = {k: torch.empty(words[k], dtype=torch.int64, device="cuda") for k in (1, 64)}
        counts = torch.zeros(9 * 2 * 2, dtype=torch.int64, device="cuda")
        hc_scratch = torch.empty(int(lib.cdll.gt_hit_curve_scratch_words(ctypes.c_int64(M), 1)), dtype=torch.int32, device="cuda")
        out30 = torch.empty(30, device="cuda")
        vm_scratch = torch.empty(int(lib.cdll.gt_voice_metrics_scratch_floats(ctypes.c_int64(M))), device="cuda")

        def group_metrics(k, masked):
            return lambda: lib.call("gt_group_metrics", _ptr(pred), _ptr(gt), _ptr(tag[k]), _ptr(cells) if masked else None, ctypes.c_int64(n), k,
                                    _ptr(acc[k]), _ptr(seq), _ptr(scratch[k]), stream)

        def voice_metrics():
            lib.call("gt_voice_metrics", _ptr(pred), _ptr(gt), ctypes.c_int64(M), _ptr(out30), _ptr(vm_scratch), stream)

        def hit_curve():
            lib.call("gt_hit_curve", _ptr(pred), 27, _ptr(gt), ctypes.c_int64(M), cgrid, 1, _ptr(counts), _ptr(hc_scratch), stream)

        t = timed({"g1": group_metrics(1, False), "g1m": group_metrics(1, True), "g64": group_metrics(64, False), "g64m": group_metrics(64, True),
                   "voice_metrics": voice_metrics, "hit_curve": hit_curve}, args.reps, args.inner)
        both = t["voice_metrics"] + t["hit_curve"]
        read = n * 2.0 * 32 * 27 * 4
        lines += ["%d sequences (%d rows; the two buffers: %.1f MB):" % (n, M, read / 1e6)]
        for key, what, k in (("g1", " 1 group,  every cell ", 1), ("g1m", " 1 group,  cell mask  ", 1), ("g64", "64 groups, every cell ", 64),
                             ("g64m", "64 groups, cell mask  ", 64)):
            lines += ["  gt_group_metrics, %s %9.4f ms/call   (%.2f of the two existing passes; %.2f TB/s of input; partials: %.2f MB)" % (
                what, t[key], t[key] / both, read / t[key] / 1e9, words[k] * 8 / 1e6)]
        lines += ["  gt_voice_metrics, same buffers            %9.4f ms/call" % t["voice_metrics"],
                  "  gt_hit_curve, 1 threshold, same buffers   %9.4f ms/call   (the two existing passes together: %.4f ms)" % (t["hit_curve"], both)]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
