"""What the threshold-curve counting pass costs (gt_hit_curve; include/groove_hip.h), at 99 thresholds over 1024 and 8192 sequences:
  gt_hit_curve on skewed probabilities (the construction of tests/test_hit_curve.py: most of a voice's elements in a few bins)
  gt_hit_curve with every probability equal (the one-bin case: every element of a voice and class meets on one counter)
  gt_voice_metrics on the same rows  -- the yardstick: an existing two-kernel pass over the same order of bytes
  gt_predict on the headline shape (d_model 128, 4 heads, F 512, L 3)  -- the call that produces such probabilities
HIP events around each timed sample, the median of --reps samples after warm-up, the compared calls alternating; a sample of the small
passes is --inner back-to-back calls (one call is a few microseconds: below what an event pair resolves).
usage: python tools/hit_curve_bench.py [--out FILE]   (one GPU)"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.voice_select_bench import DIMS, _ptr, timed  # noqa: E402
from transformergrooveinfilling_amd import _lib, layout  # noqa: E402

HIT_RATES = [.25, .2, .5, .05, .02, .02, .02, .01, 0]


def skewed(n_seq, seed=0):
    rng = np.random.default_rng(seed)
    M = n_seq * 32
    y = rng.random((M, 9)) < np.array(HIT_RATES)[None, :]
    logit = rng.normal(-2.0, 1.5, (M, 9)) + 3.0 * y * rng.random((M, 9))
    gt = np.zeros((M, 27), np.float32)
    gt[:, :9] = y
    return (1.0 / (1.0 + np.exp(-logit))).astype(np.float32), gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls per timed sample of the small passes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    lib = _lib.get_lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    grid = [float(np.float32(k) / np.float32(100)) for k in range(1, 100)]
    cgrid = (ctypes.c_float * 99)(*grid)
    lines = ["hit_curve_bench: 99 thresholds, median of %d samples (HIP events), %d back-to-back calls per sample of the small passes" % (
        args.reps, args.inner), "device: %s" % torch.cuda.get_device_name(0)]
    for n in (1024, 8192):
        M = n * 32
        p_np, gt_np = skewed(n)
        prob, gt = torch.from_numpy(p_np).cuda(), torch.from_numpy(gt_np).cuda()
        flat = torch.full((M, 9), 0.015, device="cuda")
        hvo = torch.zeros(M, 27, device="cuda")
        hvo[:, :9] = prob
        counts = torch.zeros(9 * 2 * 100, dtype=torch.int64, device="cuda")
        scratch = torch.empty(int(lib.cdll.gt_hit_curve_scratch_words(ctypes.c_int64(M), 99)), dtype=torch.int32, device="cuda")
        out30 = torch.empty(30, device="cuda")
        vm_scratch = torch.empty(int(lib.cdll.gt_voice_metrics_scratch_floats(ctypes.c_int64(M))), device="cuda")

        def curve(p, stride):
            return lambda: lib.call("gt_hit_curve", _ptr(p), stride, _ptr(gt), ctypes.c_int64(M), cgrid, 99, _ptr(counts), _ptr(scratch), stream)

        def voice_metrics():
            lib.call("gt_voice_metrics", _ptr(hvo), _ptr(gt), ctypes.c_int64(M), _ptr(out30), _ptr(vm_scratch), stream)

        t = timed({"skewed": curve(prob, 9), "one_bin": curve(flat, 9), "skewed27": curve(hvo, 27), "voice_metrics": voice_metrics},
                  args.reps, args.inner)
        # the predict call that produces the probabilities of such a chunk
        cfg = _lib.make_config(n, 16, DIMS["d_model"], DIMS["n_heads"], DIMS["dim_feedforward"], DIMS["num_encoder_layers"], 0, DIMS["dropout"])
        total, entries = lib.param_layout(cfg)
        host = torch.zeros(total)
        P = layout.init_params(DIMS, seed=0)
        for (name, _), (off, size, _, _) in zip(layout.param_names(DIMS["d_model"], DIMS["dim_feedforward"], 16, DIMS["num_encoder_layers"], 0), entries):
            host[off:off + size] = torch.from_numpy(P[name]).reshape(-1)
        params = host.cuda()
        pe = torch.from_numpy(layout.positional_encoding(DIMS["d_model"])).cuda()
        x = torch.from_numpy(layout.synthetic_batch(n, 16, seed=2)[0]).cuda()
        ws = torch.empty(lib.workspace_floats(cfg), dtype=torch.float32, device="cuda")
        lib.call("gt_workspace_init", ctypes.byref(cfg), _ptr(ws), stream)
        pred_out = torch.empty(M, 27, device="cuda")

        def predict():
            lib.call("gt_predict", ctypes.byref(cfg), _ptr(params), _ptr(pe), _ptr(x), _ptr(pred_out), ctypes.c_float(0.5), 0, None, _ptr(ws), stream)

        tp = timed({"gt_predict": predict}, args.reps, 1)
        del ws
        lines += ["%d sequences (%d rows, %d elements):" % (n, M, M * 9),
                  "  gt_hit_curve, skewed, stride 9      %9.4f ms/call" % t["skewed"],
                  "  gt_hit_curve, skewed, stride 27     %9.4f ms/call" % t["skewed27"],
                  "  gt_hit_curve, one bin, stride 9     %9.4f ms/call   (one bin / skewed = %.2f: the one-bin case costs %s)" % (
                      t["one_bin"], t["one_bin"] / t["skewed"], "MORE" if t["one_bin"] > 1.05 * t["skewed"] else "no more"),
                  "  gt_voice_metrics, same rows         %9.4f ms/call   (hit_curve skewed / voice_metrics = %.2f)" % (
                      t["voice_metrics"], t["skewed"] / t["voice_metrics"]),
                  "  gt_predict(use_thres = 0), headline %9.4f ms/call   (hit_curve skewed = %.1f %% of it)" % (
                      tp["gt_predict"], 100.0 * t["skewed"] / tp["gt_predict"])]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
