"""Cost of global-norm gradient clipping in the train step (StepEngine(max_grad_norm=...)): ms/step with clipping off, with
max_norm = 1e30 (the norm pass; the scaling launch returns at once) and with max_norm = 1e-3 (every step scales), measured in the same
process and alternated, on the BASELINE / YAML shapes below; then one rocprofv3 --kernel-trace --stats run of the d_model-512 shape for the
two clipping kernels' own times and the norm pass's share of the HBM peak.  Each GPU step is a child process under its own time limit
(timeout -k 10); the first that fails or times out ends the tool.

usage: python tools/clip_bench.py [--out DIR] [--reps N]                 the two GPU steps, summary as the last JSON line
       python tools/clip_bench.py --inner [--shapes A,B] [--modes ...]   one timing run, one JSON line per shape
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (model dims, batch, precision, embedding_size_src)
SHAPES = {
    "C2_d128_bs64": (dict(d_model=128, n_heads=4, dim_feedforward=512, num_encoder_layers=3, dropout=0.24), 64, "fp32", 16),
    "ClosedHH_d32_H16_F512_L6_bs16": (dict(d_model=32, n_heads=16, dim_feedforward=512, num_encoder_layers=6, dropout=0.24), 16, "fp32", 16),
    "C4_d512_bs512_fp32": (dict(d_model=512, n_heads=8, dim_feedforward=512, num_encoder_layers=6, dropout=0.3), 512, "fp32", 16),
    "C5_d512_bs512_bf16": (dict(d_model=512, n_heads=8, dim_feedforward=512, num_encoder_layers=6, dropout=0.3), 512, "bf16", 27),
}
MODES = {"off": None, "norm_only": 1e30, "clip": 1e-3}
HBM_PEAK = 8.0e12               # bytes/s, MI355X HBM3E spec
PROFILED = "C4_d512_bs512_fp32"


def _dims(name):
    dims, B, prec, S = SHAPES[name]
    return dict(dims, num_decoder_layers=0, embedding_size_src=S), B, prec


def inner(args):
    import torch
    from transformergrooveinfilling_amd import layout
    from transformergrooveinfilling_amd.engine import StepEngine
    modes = args.modes.split(",")
    for name in args.shapes.split(","):
        d, B, prec = _dims(name)
        eng = StepEngine(batch_size=B, optimizer="sgd", learning_rate=0.07, hit_loss_penalty=0.38, seed=1, device="cuda", precision=prec, **d)
        eng.load_named(layout.init_params(d, seed=0))
        x, y = layout.synthetic_batch(B, d["embedding_size_src"], seed=1)
        eng.x.copy_(torch.from_numpy(x))
        eng.y.copy_(torch.from_numpy(y))
        steps = args.steps or (1000 if B <= 64 else 60)
        best = {}
        for _ in range(args.reps):
            for mode in modes:                     # alternated: every mode sees the same clocks and neighbours
                eng.max_grad_norm = MODES[mode]
                for _ in range(max(10, steps // 10)):
                    eng.train_step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    eng.train_step()
                torch.cuda.synchronize()
                best[mode] = min(best.get(mode, float("inf")), (time.perf_counter() - t0) / steps * 1e3)
        st = eng.stats.cpu().tolist()
        rec = {"shape": name, "batch": B, "grad_floats": eng.total, "steps": steps, "reps": args.reps,
               "ms_per_step": {k: round(v, 5) for k, v in best.items()}, "last_grad_norm": st[6], "last_clip_coef": st[7]}
        if "off" in best:
            rec.update({"ratio_" + k: round(v / best["off"], 4) for k, v in best.items() if k != "off"})
        print(json.dumps(rec), flush=True)
        del eng
        torch.cuda.empty_cache()


def _step(cmd, limit, log):
    """one GPU step as a child under its own time limit; stops the tool when it fails"""
    with open(log, "w") as f:
        rc = subprocess.call(["timeout", "-k", "10", str(limit)] + cmd, stdout=f, stderr=subprocess.STDOUT, cwd=ROOT)
    text = open(log).read()
    print(text[-3000:], flush=True)
    if rc != 0:
        sys.exit("clip_bench: step failed with exit status %d: %s (log %s)" % (rc, " ".join(cmd), log))
    return text


def driver(args):
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), "--inner"]
    text = _step(me + ["--shapes", ",".join(SHAPES), "--reps", str(args.reps)], 900, os.path.join(args.out, "timing.log"))
    rows = [json.loads(l) for l in text.splitlines() if l.startswith("{")]
    prof = os.path.join(args.out, "prof")
    _step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "clip", "--"] + me +
          ["--shapes", PROFILED, "--modes", "clip", "--steps", "20", "--reps", "1"], 600, os.path.join(args.out, "prof.log"))
    from transformergrooveinfilling_amd import _lib
    d, B, prec = _dims(PROFILED)
    cfg = _lib.make_config(B, d["embedding_size_src"], d["d_model"], d["n_heads"], d["dim_feedforward"], d["num_encoder_layers"])
    n = _lib.get_lib().param_layout(cfg)[0] - 1    # floats each pass covers (the guard element aside)
    kern = {}
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            for k, nbytes in (("grad_norm_kernel", 4 * n), ("grad_scale_kernel", 8 * n)):
                if k in r["Name"]:
                    us = float(r["AverageNs"]) / 1e3
                    kern[k] = {"calls": int(r["Calls"]), "avg_us": round(us, 2), "GB_per_s": round(nbytes / us / 1e3, 1),
                               "share_of_hbm_peak": round(nbytes / (us * 1e-6) / HBM_PEAK, 3)}
    print(json.dumps({"clip_bench": rows, "kernels_" + PROFILED: kern, "floats": n}))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--inner", action="store_true", help="one timing run in this process (what the driver starts)")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--steps", type=int, default=0, help="timed steps per mode (default: 1000 at batch <= 64, else 60)")
    ap.add_argument("--reps", type=int, default=2, help="alternations of the modes; the best time of each is kept")
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "clip_bench"))
    args = ap.parse_args()
    inner(args) if args.inner else driver(args)


if __name__ == "__main__":
    main()
