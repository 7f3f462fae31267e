"""Cost of drawing the infilling pair in the gather: ms/step of the indexed train step with gt_gather_infill at its head
(StepEngine.train_step_indexed_infill: ONE resident tensor of full grooves) beside the indexed step with gt_gather_batch
(StepEngine.train_step_indexed: two resident tensors paired beforehand), same process, alternated, on the InfillingClosedHH_Symbolic YAML
shape and on the BASELINE configs[4] shape.  Then the two gather kernels' own times from the library's launch timing (gt_profile_report):
each is enqueued alone with timing on, so the report holds that kernel's launches and nothing else, whatever row they are filed under.

usage: python tools/infill_bench.py [--shapes A,B] [--reps N] [--steps N] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (model dims, batch, precision); embedding_size_src is 27 for both (the input is the groove itself)
SHAPES = {
    "ClosedHH_Symbolic_d32_H16_F512_L6_bs16": (dict(d_model=32, n_heads=16, dim_feedforward=512, num_encoder_layers=6, dropout=0.24), 16, "fp32"),
    "C5_d512_H8_F512_L6_bs512_bf16": (dict(d_model=512, n_heads=8, dim_feedforward=512, num_encoder_layers=6, dropout=0.3), 512, "bf16"),
}
N_SET = 8192            # resident grooves (2 x 28 MB paired, 28 MB full)
INFILL = dict(voices=[2], min_remove=1, max_remove=1)       # the ClosedHH case


def grooves(n, seed):
    """full grooves: hits ~ Bernoulli(0.15), vel = U * h, off = (U - 0.5) * h (train.py's synthetic generator); the closed hi-hat and the kick
    are made active everywhere, so every groove can be paired"""
    import torch
    g = torch.Generator().manual_seed(seed)
    h = (torch.rand(n, 32, 9, generator=g) < 0.15).float()
    h[:, 0, 0] = 1.0
    h[:, 0, 2] = 1.0
    v = torch.rand(n, 32, 9, generator=g) * h
    o = (torch.rand(n, 32, 9, generator=g) - 0.5) * h
    return torch.cat([h, v, o], -1).contiguous()


def run(args):
    import torch
    from transformergrooveinfilling_amd import _lib, infill, layout
    from transformergrooveinfilling_amd.engine import StepEngine
    if not torch.cuda.is_available():
        sys.exit("infill_bench measures on the GPU; none is visible")
    rows = []
    for name in args.shapes.split(","):
        dims, B, prec = SHAPES[name]
        d = dict(dims, num_decoder_layers=0, embedding_size_src=27)
        eng = StepEngine(batch_size=B, optimizer="sgd", learning_rate=0.07, hit_loss_penalty=0.38, seed=1, device="cuda", precision=prec, **d)
        eng.load_named(layout.init_params(d, seed=0))
        eng.infill_opts = eng.make_infill_opts(**INFILL)
        hvo = grooves(N_SET, 7).cuda()
        assert infill.infill_eligible(hvo, INFILL).numel() == N_SET
        xs, ys, _ = infill.pair_once(hvo, INFILL, seed=1)           # the parent's resident form: paired beforehand
        g = torch.Generator().manual_seed(3)
        batches = [torch.randint(0, N_SET, (B,), generator=g).cuda() for _ in range(64)]
        modes = {"gather_batch": lambda i: eng.train_step_indexed(xs, ys, batches[i % 64]),
                 "gather_infill": lambda i: eng.train_step_indexed_infill(hvo, batches[i % 64])}
        steps = args.steps or (2000 if B <= 64 else 100)

        def timed():
            times = {m: [] for m in modes}
            for _ in range(args.reps):
                for m, fn in modes.items():             # alternated: both see the same clocks and neighbours
                    for i in range(max(20, steps // 10)):
                        fn(i)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(steps):
                        fn(i)
                    torch.cuda.synchronize()
                    times[m].append((time.perf_counter() - t0) / steps * 1e3)
            return times

        times = timed()                                 # the engine's own choice between direct enqueue and graph replay
        auto_graph = bool(eng.graph_for(eng.slot(B)))
        replayed = None
        if not auto_graph:                              # ... and, where it enqueues directly, both steps as replayed graphs: no host work per step
            eng.use_graph = True
            replayed = timed()
            eng.use_graph = "auto"
        loss = float(eng.slot(B).stats[0])
        # the gather kernels alone, timed by the library's events around each launch
        lib, s = eng.lib, eng.slot(B)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        io = _lib.infill_opts_struct(eng.infill_opts)
        kern = {}
        for label, call in (("gather_batch", lambda: lib.call("gt_gather_batch", p(xs), p(ys), p(s.idx), ctypes.c_int64(N_SET), B, 27, p(s.x), p(s.y), eng.stream)),
                            ("gather_infill", lambda: lib.call("gt_gather_infill", p(hvo), p(s.idx), ctypes.c_int64(N_SET), B, ctypes.byref(io),
                                                               p(eng.state), p(s.x), p(s.y), p(s.removed), eng.stream))):
            for _ in range(20):
                call()
            torch.cuda.synchronize()
            lib.cdll.gt_profile_enable(1)
            try:
                for _ in range(args.kernel_launches):
                    call()
                buf = ctypes.create_string_buffer(1 << 16)
                lib.cdll.gt_profile_report(buf, len(buf), 256)
            finally:
                lib.cdll.gt_profile_enable(0)
            rep = [ln.split() for ln in buf.value.decode().splitlines()]
            n, ms = sum(int(r[1]) for r in rep), sum(float(r[2]) for r in rep)
            assert n == args.kernel_launches, rep                   # (only this kernel ran while timing was on)
            kern[label] = round(ms / n * 1e3, 3)                    # us per launch
        rec = {"shape": name, "batch": B, "precision": prec, "resident_grooves": N_SET, "steps": steps, "reps": args.reps,
               "graph": auto_graph, "replayed_best_ms": None if replayed is None else {m: round(min(v), 5) for m, v in replayed.items()},
               "ms_per_step": {m: [round(t, 5) for t in v] for m, v in times.items()},
               "best_ms": {m: round(min(v), 5) for m, v in times.items()},
               "spread_pct": {m: round(100 * (max(v) - min(v)) / min(v), 2) for m, v in times.items()},
               "infill_over_batch": round(min(times["gather_infill"]) / min(times["gather_batch"]), 4),
               "gather_kernel_us": kern, "last_loss": loss}
        print(json.dumps(rec), flush=True)
        rows.append(rec)
        del eng, hvo, xs, ys
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--steps", type=int, default=0, help="timed steps per mode and repetition (default: 2000 at batch <= 64, else 100)")
    ap.add_argument("--reps", type=int, default=5, help="alternations of the two modes; every time is reported, the best is compared")
    ap.add_argument("--kernel-launches", type=int, default=200, help="launches of each gather kernel under the library's launch timing")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
