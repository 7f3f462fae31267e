"""Cost of drawing the event-level infilling pair in the gather: ms/step of three forms of the indexed train step, same process, alternated:
  gather_batch   StepEngine.train_step_indexed               two resident tensors paired beforehand (gt_gather_batch)
  gather_infill  StepEngine.train_step_indexed_infill        ONE resident tensor, whole voices removed in the gather (gt_gather_infill)
  gather_events  StepEngine.train_step_indexed_infill_events ONE resident tensor, a share of the hits removed in the gather (gt_gather_infill_events)
on the InfillingClosedHH_Symbolic YAML shape and on the BASELINE configs[4] shape (the two of tools/infill_bench.py).  Medians over the
repetitions and each mode's run-to-run spread are reported.  Then the gather kernels' own times from the library's launch timing
(gt_profile_report), each enqueued alone; the event gather twice: with every hit a candidate, and with a voice mask that names a voice
without hits -- no thread then enters the rank loop while the loads, barriers and stores are the same, so the difference is the rank loop.

usage: python tools/infill_events_bench.py [--shapes A,B] [--reps N] [--steps N] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from infill_bench import INFILL, N_SET, SHAPES  # noqa: E402

EVENTS = dict(voices=list(range(9)), ratio=(0.4, 0.6))      # the reference's remove_random_events(thres_range=(0.4, 0.6))
EMPTY_VOICE = 8                                             # no groove of the bench set has a hit there: events_no_candidates


def grooves(n, seed):
    """tools/infill_bench.py's grooves with voice EMPTY_VOICE left without hits"""
    from infill_bench import grooves as base
    g = base(n, seed)
    g[:, :, [EMPTY_VOICE, 9 + EMPTY_VOICE, 18 + EMPTY_VOICE]] = 0.0
    return g.contiguous()


def run(args):
    import torch
    from transformergrooveinfilling_amd import _lib, infill, layout
    from transformergrooveinfilling_amd.engine import StepEngine
    if not torch.cuda.is_available():
        sys.exit("infill_events_bench measures on the GPU; none is visible")
    rows = []
    for name in args.shapes.split(","):
        dims, B, prec = SHAPES[name]
        d = dict(dims, num_decoder_layers=0, embedding_size_src=27)
        eng = StepEngine(batch_size=B, optimizer="sgd", learning_rate=0.07, hit_loss_penalty=0.38, seed=1, device="cuda", precision=prec, **d)
        eng.load_named(layout.init_params(d, seed=0))
        eng.infill_opts = eng.make_infill_opts(**INFILL)
        eng.infill_event_opts = eng.make_infill_event_opts(**EVENTS)
        hvo = grooves(N_SET, 7).cuda()
        assert infill.infill_eligible(hvo, INFILL).numel() == N_SET and infill.events_eligible(hvo, dict(EVENTS, mode="events")).numel() == N_SET
        xs, ys, _ = infill.pair_once(hvo, INFILL, seed=1)           # the resident form of the plain step: paired beforehand
        g = torch.Generator().manual_seed(3)
        batches = [torch.randint(0, N_SET, (B,), generator=g).cuda() for _ in range(64)]
        modes = {"gather_batch": lambda i: eng.train_step_indexed(xs, ys, batches[i % 64]),
                 "gather_infill": lambda i: eng.train_step_indexed_infill(hvo, batches[i % 64]),
                 "gather_events": lambda i: eng.train_step_indexed_infill_events(hvo, batches[i % 64])}
        steps = args.steps or (2000 if B <= 64 else 100)

        def timed():
            times = {m: [] for m in modes}
            for _ in range(args.reps):
                for m, fn in modes.items():             # alternated: all three see the same clocks and neighbours
                    for i in range(max(20, steps // 10)):
                        fn(i)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(steps):
                        fn(i)
                    torch.cuda.synchronize()
                    times[m].append((time.perf_counter() - t0) / steps * 1e3)
            return times

        def summary(times):
            med = {m: statistics.median(v) for m, v in times.items()}
            return {"ms_per_step": {m: [round(t, 5) for t in v] for m, v in times.items()},
                    "median_ms": {m: round(med[m], 5) for m in times},
                    "spread_pct": {m: round(100 * (max(v) - min(v)) / min(v), 2) for m, v in times.items()},
                    "events_over_infill": round(med["gather_events"] / med["gather_infill"], 4),
                    "events_minus_infill_us": round((med["gather_events"] - med["gather_infill"]) * 1e3, 3),
                    "events_over_batch": round(med["gather_events"] / med["gather_batch"], 4),
                    "infill_over_batch": round(med["gather_infill"] / med["gather_batch"], 4)}

        direct = summary(timed())                       # the engine's own choice between direct enqueue and graph replay
        auto_graph = bool(eng.graph_for(eng.slot(B)))
        replayed = None
        if not auto_graph:                              # ... and, where it enqueues directly, all three as replayed graphs: no host work per step
            eng.use_graph = True
            replayed = summary(timed())
            eng.use_graph = "auto"
        loss = float(eng.slot(B).stats[0])
        # the gather kernels alone, timed by the library's events around each launch
        lib, s = eng.lib, eng.slot(B)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        io = _lib.infill_opts_struct(eng.infill_opts)
        eo = _lib.infill_event_opts_struct(eng.infill_event_opts)
        eo_none = _lib.make_infill_event_opts(voices=[EMPTY_VOICE])
        ev = lambda o: lambda: lib.call("gt_gather_infill_events", p(hvo), p(s.idx), ctypes.c_int64(N_SET), B, ctypes.byref(o), p(eng.state),
                                        p(s.x), p(s.y), p(s.cells), eng.stream)
        kern = {}
        for label, call in (("gather_batch", lambda: lib.call("gt_gather_batch", p(xs), p(ys), p(s.idx), ctypes.c_int64(N_SET), B, 27, p(s.x), p(s.y), eng.stream)),
                            ("gather_infill", lambda: lib.call("gt_gather_infill", p(hvo), p(s.idx), ctypes.c_int64(N_SET), B, ctypes.byref(io),
                                                               p(eng.state), p(s.x), p(s.y), p(s.removed), eng.stream)),
                            ("gather_events", ev(eo)), ("events_no_candidates", ev(eo_none))):
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
               "graph": auto_graph, "direct": direct, "replayed": replayed, "gather_kernel_us": kern, "last_loss": loss}
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
    ap.add_argument("--reps", type=int, default=7, help="alternations of the three modes; every time is reported, medians are compared")
    ap.add_argument("--kernel-launches", type=int, default=200, help="launches of each gather kernel under the library's launch timing")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    run(ap.parse_args())


if __name__ == "__main__":
    main()
