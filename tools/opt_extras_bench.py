"""Cost of the optimizer's extras (momentum / Nesterov / weight decay / AdamW: one launch in front of the update, StepEngine(momentum=...))
in the train step: ms/step of the plain fused step ("off": bitwise the step without the feature), of the split step with everything off but
max_grad_norm = inf ("split": what leaving the fused step costs, the clip's two launches included), and with momentum 0.9 ("momentum") or
all of momentum + Nesterov + weight decay ("all"), measured in the same process and alternated; then the pass alone, enqueued back to back
between two events (its buffers then sit in the caches: a lower bound of its time inside a step).  One JSON line per shape.

usage: python tools/opt_extras_bench.py [--shapes A,B] [--modes ...] [--reps N] [--steps N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (model dims, batch)
SHAPES = {
    "C2_d128_bs64": (dict(d_model=128, n_heads=4, dim_feedforward=512, num_encoder_layers=3, dropout=0.24), 64),
    "C4_d512_bs64": (dict(d_model=512, n_heads=8, dim_feedforward=512, num_encoder_layers=6, dropout=0.3), 64),
}
# name: (max_grad_norm, momentum, nesterov, weight_decay)
MODES = {"off": (None, 0.0, False, 0.0), "split": (float("inf"), 0.0, False, 0.0), "momentum": (None, 0.9, False, 0.0),
         "all": (None, 0.9, True, 5e-4)}
BYTES = {"momentum": 16, "all": 20}     # per element: gradient read + written, momentum buffer read + written [, parameter read]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--steps", type=int, default=0, help="timed steps per mode (default: 1000 at d_model 128, else 300)")
    ap.add_argument("--reps", type=int, default=3, help="alternations of the modes; the best time of each is kept")
    args = ap.parse_args()
    import torch
    from transformergrooveinfilling_amd import layout
    from transformergrooveinfilling_amd.engine import StepEngine
    modes = args.modes.split(",")
    for name in args.shapes.split(","):
        dims, B = SHAPES[name]
        d = dict(dims, num_decoder_layers=0, embedding_size_src=16)
        eng = StepEngine(batch_size=B, optimizer="sgd", learning_rate=0.07, hit_loss_penalty=0.38, seed=1, device="cuda", **d)
        eng.load_named(layout.init_params(d, seed=0))
        x, y = layout.synthetic_batch(B, 16, seed=1)
        eng.x.copy_(torch.from_numpy(x))
        eng.y.copy_(torch.from_numpy(y))
        steps = args.steps or (1000 if d["d_model"] <= 128 else 300)
        best = {}
        for _ in range(args.reps):
            for mode in modes:                     # alternated: every mode sees the same clocks and neighbours
                eng.max_grad_norm, eng.momentum, eng.nesterov, eng.weight_decay = MODES[mode]
                for _ in range(max(10, steps // 10)):
                    eng.train_step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    eng.train_step()
                torch.cuda.synchronize()
                best[mode] = min(best.get(mode, float("inf")), (time.perf_counter() - t0) / steps * 1e3)
        rec = {"shape": name, "batch": B, "floats": eng.total, "steps": steps, "reps": args.reps,
               "ms_per_step": {k: round(v, 5) for k, v in best.items()}}
        if "off" in best:
            rec.update({"ratio_" + k: round(v / best["off"], 4) for k, v in best.items() if k != "off"})
        s = eng.slot(B)
        for mode in (m for m in modes if m in BYTES):          # the pass alone, back to back
            eng.max_grad_norm, eng.momentum, eng.nesterov, eng.weight_decay = MODES[mode]
            hp = eng._opt_extras()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(20):
                eng._enqueue_prepare(s.cfg, s.ws, hp)
            a.record()
            for _ in range(200):
                eng._enqueue_prepare(s.cfg, s.ws, hp)
            b.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(b) / 200 * 1e3
            rec["pass_us_" + mode] = round(us, 2)
            rec["pass_GB_per_s_" + mode] = round(BYTES[mode] * (eng.total - 1) / us / 1e3, 1)
        print(json.dumps(rec), flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
