"""Cost of the loss options (gt_loss_opts: pos_weight, voice / term weights, focal modulation, separate penalties, per-voice statistics --
StepEngine.loss_opts) in the train step: ms/step of today's fused step ("off": bitwise the step without the feature) against the step
with options, whose loss is a launch of its own (gt_train_step_loss) -- "neutral": every option at its neutral value, what the extra
launch and, on the sequence-resident path, the lost forward-into-backward fusion cost; "all": pos_weight, voice and term weights, separate
penalties and focal gamma 2 (powf per element).  Measured in the same process and alternated; then the loss kernel alone, enqueued back to
back between two events.  One JSON line per shape.

usage: python tools/loss_opts_bench.py [--shapes A,B] [--modes ...] [--reps N] [--steps N]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (model dims, batch)
SHAPES = {
    "C2_d128_bs64": (dict(d_model=128, n_heads=4, dim_feedforward=512, num_encoder_layers=3, dropout=0.24), 64),      # BASELINE configs[1]
    "ClosedHH_d32_h16_bs16": (dict(d_model=32, n_heads=16, dim_feedforward=512, num_encoder_layers=6, dropout=0.24), 16),   # InfillingClosedHH YAML
}
PW = [0.5, 1.0, 2.0, 3.5, 6.0, 12.0, 1.5, 0.75, 9.0]
VW = [2.0, 1.5, 1.0, 0.0, 0.5, 0.25, 1.0, 3.0, 0.1]
# name: keywords of StepEngine.make_loss_opts (None: the options off)
MODES = {"off": None, "neutral": {}, "all": dict(vo_penalty=0.05, pos_weight=PW, voice_weight=VW, focal_gamma=2.0, term_weights=(0.7, 2.0, 0.4))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--steps", type=int, default=1000, help="timed steps per mode")
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
        opts = {m: None if MODES[m] is None else eng.make_loss_opts(**MODES[m]) for m in modes}
        best = {}
        for _ in range(args.reps):
            for mode in modes:                     # alternated: every mode sees the same clocks and neighbours
                eng.loss_opts = opts[mode]
                for _ in range(max(10, args.steps // 10)):
                    eng.train_step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    eng.train_step()
                torch.cuda.synchronize()
                best[mode] = min(best.get(mode, float("inf")), (time.perf_counter() - t0) / args.steps * 1e3)
        s = eng.slot(B)
        rec = {"shape": name, "batch": B, "steps": args.steps, "reps": args.reps, "graph": bool(eng.graph_for(s)),
               "launches_off": int(eng.lib.cdll.gt_step_launches(ctypes.byref(s.cfg))),
               "ms_per_step": {k: round(v, 5) for k, v in best.items()}}
        if "off" in best:
            rec.update({"ratio_" + k: round(v / best["off"], 4) for k, v in best.items() if k != "off"})
        for mode in (m for m in modes if opts[m] is not None):          # the loss kernel alone, back to back (on the last step's outputs)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(20):
                eng.loss(s, s.y, 0.0, want_grad=False, opts=opts[mode])
            a.record()
            for _ in range(200):
                eng.loss(s, s.y, 0.0, want_grad=False, opts=opts[mode])
            b.record()
            torch.cuda.synchronize()
            rec["loss_kernel_us_" + mode] = round(a.elapsed_time(b) / 200 * 1e3, 2)
        print(json.dumps(rec), flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
