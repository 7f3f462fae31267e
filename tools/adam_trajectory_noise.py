#!/usr/bin/env python3
"""adam_trajectory_noise.py -- what tests/seq_variants.py's ADAM_ORACLE is written from (python tools/adam_trajectory_noise.py; CPU only, 1 min).

For every Adam case of tests/seq_variants.py (table and generated): the fp32 oracle's own free-running three-step Adam trajectory at lr 0.05
against the fp64 one, as a fraction of check_train_step's free-running bars (loss 2e-5, live elements 1e-3, well-conditioned 1e-4) and whether a
ReLU decision of the fp32 run differs from the fp64 run's away from the kink (1e-5).  One JSON line per case: its worst fraction of each bar, "kink" in units of 1e-5."""
import sys, os, json
from multiprocessing import Pool
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def measure(item):
    name, cfg, B, p, lr = item
    from oracle import numpy_groove as ng
    cfg = dict(cfg, dropout=p)
    P = ng.init_params(cfg, seed=9, perturb=0.05)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=4)
    st = {}
    for dt in (np.float64, np.float32):
        st[dt] = dict(cur={k: v.astype(dt) for k, v in P.items()})
    worst = dict(loss=0.0, live=0.0, strong=0.0, kink=0.0)
    for step in range(3):
        rng = (77, 5, step) if p > 0 else None
        out = {}
        for dt in (np.float64, np.float32):
            s = st[dt]
            (h, v, o), C = ng.forward(s["cur"], cfg, x.astype(dt), rng=rng, dtype=dt)
            stats, dpred = ng.calculate_loss((h, v, o), y.astype(dt), dt(0.38))
            G = ng.backward(s["cur"], cfg, C, dpred, dtype=dt)
            if step == 0:
                s["m"], s["v"] = {k: np.zeros_like(a) for k, a in s["cur"].items()}, {k: np.zeros_like(a) for k, a in s["cur"].items()}
            s["cur"], s["m"], s["v"] = ng.adam_step(s["cur"], G, s["m"], s["v"], step + 1, lr)
            out[dt] = (float(stats[0]), C, G)
        l64, C64, G64 = out[np.float64]; l32, C32, _ = out[np.float32]
        worst["loss"] = max(worst["loss"], abs(l32 - l64) / (2e-5 * max(1, abs(l64))))
        for c64, c32 in zip(C64["enc"], C32["enc"]):
            pre, flips = c64["hpre"], (c64["hpre"] > 0) != (c32["hpre"] > 0)
            if c64.get("mf") is not None:
                flips &= np.asarray(c64["mf"]) != 0
            if flips.any():
                worst["kink"] = max(worst["kink"], float(np.abs(pre[flips]).max()) / 1e-5)
        a64, a32 = C64["in_enc"]["a"], C32["in_enc"]["a"]
        flips = (a64 > 0) != (a32 > 0)
        if flips.any():
            worst["kink"] = max(worst["kink"], float(np.abs(a64[flips]).max()) / 1e-5)
        c64, c32 = st[np.float64]["cur"], st[np.float32]["cur"]
        for k in c64:
            g = np.abs(G64[k]); sc = max(1.0, np.abs(c64[k]).max()); d = np.abs(c32[k].astype(np.float64) - c64[k])
            worst["live"] = max(worst["live"], d[g > 1e-6].max(initial=0) / (1e-3 * sc))
            worst["strong"] = max(worst["strong"], d[g > 0.1 * g.max()].max(initial=0) / (1e-4 * sc))
    return name, worst


if __name__ == "__main__":
    import seq_variants as sv
    items = [(k, c[1], c[2], c[3], 0.05) for k, c in sv.CASES.items() if c[0] == "adam"]
    items += [(k, spec[1], spec[2], spec[3], 0.05) for k, (spec, sigs) in sv.before_cases().items() if spec[0] == "adam"]
    items.sort(key=lambda it: -it[2] * it[1]["d_model"])
    with Pool(14) as pool:
        for name, w in pool.imap_unordered(measure, items):
            print(json.dumps(dict(name=name, **{k: round(v, 3) for k, v in w.items()})), flush=True)
