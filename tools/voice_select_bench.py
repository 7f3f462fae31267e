"""What the per-voice generation controls cost (gt_predict_voices, gt_voice_select; include/groove_hip.h), on the headline shape
(d_model 128, 4 heads, F 512, L 3) with one evaluation chunk of --n sequences:
  gt_predict                      against  gt_predict_voices with per-voice thresholds, caps, a temperature and the velocity / offset mask;
  gt_voice_select alone           against  gt_voice_metrics on the same rows (both stream the same (M,27) tiles: the yardstick for such a pass).
HIP events around each timed sample, the median of --reps samples after warm-up, the compared calls alternating; a sample of the two small
passes is --inner back-to-back calls (one call is a few microseconds: below what an event pair resolves).
usage: python tools/voice_select_bench.py [--n 1024] [--out FILE]   (one GPU)"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from transformergrooveinfilling_amd import _lib, layout  # noqa: E402

DIMS = dict(d_model=128, n_heads=4, dim_feedforward=512, num_encoder_layers=3, num_decoder_layers=0, dropout=0.24, embedding_size_src=16)
THRES = [0.5, 0.45, 0.55, 0.5, 0.4, 0.6, 0.5, 0.48, 0.52]
CAPS = [32, 4, 2, 0, 8, 1, 3, 32, 5]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def timed(fns, reps, inner, warmup=5):
    """{name: median ms per call}; the functions alternate inside every repetition"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    return {k: statistics.median(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024, help="sequences in the evaluation chunk")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls per timed sample of the two small passes")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    lib = _lib.get_lib()
    n, M = args.n, args.n * 32
    cfg = _lib.make_config(n, 16, DIMS["d_model"], DIMS["n_heads"], DIMS["dim_feedforward"], DIMS["num_encoder_layers"], 0, DIMS["dropout"])
    total, entries = lib.param_layout(cfg)
    flat = torch.zeros(total)
    names = layout.param_names(DIMS["d_model"], DIMS["dim_feedforward"], 16, DIMS["num_encoder_layers"], 0)
    P = layout.init_params(DIMS, seed=0)
    for (name, _), (off, size, _, _) in zip(names, entries):
        flat[off:off + size] = torch.from_numpy(P[name]).reshape(-1)
    params = flat.cuda()
    pe = torch.from_numpy(layout.positional_encoding(DIMS["d_model"])).cuda()
    x = torch.from_numpy(layout.synthetic_batch(n, 16, seed=2)[0]).cuda()
    gt = torch.from_numpy(layout.synthetic_batch(n, 16, seed=2)[1]).cuda()
    ws = torch.empty(lib.workspace_floats(cfg), dtype=torch.float32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.call("gt_workspace_init", ctypes.byref(cfg), _ptr(ws), stream)
    hvo = torch.empty(M, 27, device="cuda")
    prob = torch.empty(M, 9, device="cuda")
    out30 = torch.empty(30, device="cuda")
    scratch = torch.empty(int(lib.cdll.gt_voice_metrics_scratch_floats(ctypes.c_int64(M))), device="cuda")
    vs = _lib.make_voice_sampling(THRES, CAPS, 0.8, 0, True)

    def predict():
        lib.call("gt_predict", ctypes.byref(cfg), _ptr(params), _ptr(pe), _ptr(x), _ptr(hvo), ctypes.c_float(0.5), 1, None, _ptr(ws), stream)

    def predict_voices():
        lib.call("gt_predict_voices", ctypes.byref(cfg), _ptr(params), _ptr(pe), _ptr(x), _ptr(hvo), ctypes.byref(vs), ctypes.c_uint32(0),
                 ctypes.c_int64(0), _ptr(prob), None, _ptr(ws), stream)

    def select():
        lib.call("gt_voice_select", _ptr(sel_hvo), _ptr(prob), ctypes.byref(vs), ctypes.c_int64(n), stream)

    def metrics():
        lib.call("gt_voice_metrics", _ptr(sel_hvo), _ptr(gt), ctypes.c_int64(M), _ptr(out30), _ptr(scratch), stream)

    whole = timed({"gt_predict": predict, "gt_predict_voices": predict_voices}, args.reps, 1)
    # the select pass alone, on the uncapped decisions of this chunk (after the first call the hits are within their caps; every hit lane of
    # a capped voice still counts its rank, and the same columns are rewritten)
    free = _lib.make_voice_sampling(THRES, 32, 0.8)
    lib.call("gt_predict_voices", ctypes.byref(cfg), _ptr(params), _ptr(pe), _ptr(x), _ptr(hvo), ctypes.byref(free), ctypes.c_uint32(0),
             ctypes.c_int64(0), _ptr(prob), None, _ptr(ws), stream)
    sel_hvo = hvo.clone()
    hits = float(sel_hvo[:, :9].mean())
    passes = timed({"gt_voice_select": select, "gt_voice_metrics": metrics}, args.reps, args.inner)
    lines = ["voice_select_bench: d_model 128 / 4 heads / F 512 / L 3, %d sequences (%d rows), median of %d samples (HIP events)" % (n, M, args.reps),
             "device: %s" % torch.cuda.get_device_name(0),
             "gt_predict                     %9.4f ms/call" % whole["gt_predict"],
             "gt_predict_voices (caps, mask) %9.4f ms/call   (%.3fx gt_predict)" % (whole["gt_predict_voices"],
                                                                                  whole["gt_predict_voices"] / whole["gt_predict"]),
             "gt_voice_select alone          %9.4f ms/call   (%d back-to-back calls per sample; uncapped hit rate %.3f)" % (
                 passes["gt_voice_select"], args.inner, hits),
             "gt_voice_metrics, same rows    %9.4f ms/call   (select / metrics = %.2f)" % (
                 passes["gt_voice_metrics"], passes["gt_voice_select"] / passes["gt_voice_metrics"])]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
