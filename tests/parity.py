"""Parity checks shared by the emulator tests (CPU, small) and the GPU tests (real HIP library).
Tolerances (fp32 path, stated per BASELINE.json north_star): outputs max-abs <= 1e-4 vs the fp64
oracle (we assert 2e-5), gradients <= 1e-3 relative to the tensor's max (we assert 2e-4), hit masks
bit-exact wherever |sigmoid(logit) - thres| exceeds 1e-4; ReLU decisions identical wherever the oracle's
|pre-activation| exceeds 1e-5 (adopt_device_kinks)."""
import glob
import os

import ctypes

import numpy as np

import harness
import regimes
from harness import Runner
from oracle import numpy_groove as ng

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUT_TOL, GRAD_TOL = 2e-5, 2e-4
# the last check's largest error / bar ratios ("out": outputs against OUT_TOL, "grad": the worst gradient tensor against GRAD_TOL, "update":
# check_update's ratio, "bf16_op": the worst per-operation ratio of check_ops_bf16, "bf16_e2e": the end-to-end sanity bound,
# "probe": the worst tensor of the worst probe of check_grad_probes against GRAD_TOL, "accumulate": check_accumulate's worst element) -- figures for
# reports (profiles/dispatch_edges.txt, profiles/grad_probes.txt); nothing asserts on them.  A regime run (check_step(regime=...)) records
# "noise": the worst quantity's device error / max(fp32 oracle's error, floor) -- the ratio regimes.NOISE_FACTOR bounds --, "noise_at": that
# quantity's name, "noise_rows": every quantity's (name, err, noise, scale, ratio), "regime": regimes.figures of the oracle's cache
FIGURES = {}
# what goes with FIGURES["bf16_op"] and is no number: "op_at" (the comparison with the worst ratio), "ops" (bar class -> (worst ratio, its comparison)),
# "widened" ((comparison, class bar, the np.float32 restatement's error, the device's error), all relative to the tensor's largest entry, for every
# bar _close's np.float32 rule widened), "ledger" (the last walk's Ledger).  Cleared with FIGURES["bf16_op"]
BF16_FIGURES = {}


def shift_right(y):
    return np.concatenate([np.zeros_like(y[:, :1]), y[:, :-1]], 1)


def rel_err(a, ref):
    return float(np.abs(a - ref).max() / (np.abs(ref).max() + 1e-12))


KINK = 1e-5


def adopt_device_kinks(r, C, cfg):
    """ReLU has no derivative at 0.  Where the fp64 oracle's pre-activation lies within KINK of the kink, the fp32 device
    may round to the other side (about one element per 1e6 pre-activations: BASELINE configs[1] at full size has 1e6 per
    layer) and both subgradients are legitimate -- the same reasoning as the hit-threshold margin above.  Take the
    device's decision for exactly those elements so that both backward passes differentiate the same function; a
    differing decision anywhere else is an error.  Returns the number of adopted elements."""
    n_enc, adopted = len(C["enc"]), 0
    todo = [(c, "hpre", c["mf"], r.ws_get("hact", l)) for l, c in enumerate(C["enc"])]
    todo += [(c, "hpre", c["mf"], r.ws_get("hact", n_enc + l)) for l, c in enumerate(C["dec"])]
    todo.append((C["in_enc"], "a", None, r.ws_get("a0")))
    for c, key, keep, dev in todo:
        pre = c[key]
        on = dev.reshape(pre.shape) > 0
        flips = on != (pre > 0)
        if keep is not None:
            flips &= keep != 0                      # dropped elements are zero on both sides whatever the sign
        if flips.any():
            assert (np.abs(pre[flips]) < KINK).all(), "ReLU decision differs away from the kink: max |pre| %g" % np.abs(pre[flips]).max()
            pre[flips] = np.where(on[flips], 1e-30, -1e-30)
            adopted += int(flips.sum())
    return adopted


def _check_forward_and_loss(r, hvo, hvo_ref, C, y, penalty, check_ws):
    """The forward half of check_step: outputs, saved activations, loss statistics and d loss / d hvo of Runner r (after r.forward) against
    the fp64 oracle's (h, v, o) and cache C.  Clears FIGURES and records "out"; returns the oracle's (dh, dv, do)."""
    h, v, o = hvo_ref
    ref = np.concatenate([h, v, o], -1)
    FIGURES.clear()
    FIGURES["out"] = float(np.abs(hvo - ref).max() / OUT_TOL)
    assert np.abs(hvo - ref).max() < OUT_TOL, "forward max-abs %g" % np.abs(hvo - ref).max()
    if check_ws:
        c0 = C["enc"][0]
        assert rel_err(r.ws_get("x0").reshape(-1), c0["x_in"].reshape(-1)) < 1e-5
        assert rel_err(r.ws_get("P", 0).reshape(-1), c0["attn"]["P"].reshape(-1)) < 1e-5
        assert rel_err(r.ws_get("hact", 0).reshape(-1), c0["hact"].reshape(-1)) < 1e-5
        assert rel_err(r.ws_get("memory").reshape(-1), C["memory"].reshape(-1)) < 1e-5
    stats, d_hvo = r.loss(y, penalty)
    rstats, dpred = ng.calculate_loss((h, v, o), y.astype(np.float64), penalty)
    for i in (0, 3, 4, 5):
        assert abs(stats[i] - rstats[i]) < 1e-5 * max(1.0, abs(rstats[i])), (i, stats[i], rstats[i])
    # hit accuracy counts (h > 0) == y_h: a logit within 1e-4 of 0 may fall on the other side in fp32, one count each
    near = int((np.abs(h) < 1e-4).sum())
    assert abs(stats[1] - rstats[1]) <= (near + 0.01) / h.size + 1e-6, (stats[1], rstats[1], near)
    assert rel_err(d_hvo, np.concatenate(dpred, -1)) < 1e-5
    return dpred


def check_step(backend, cfg, B, p=0.0, penalty=0.47, seed=3, check_ws=True, seq=True, flags=0, regime=None):
    """forward + loss + backward (+ saved activations) against the fp64 numpy oracle.  regime: a name of tests/regimes.py -- the same step
    away from initialisation, under check_step_regime's bars."""
    if regime is not None:
        return check_step_regime(backend, cfg, B, regime, p, penalty, seed, seq, flags)
    cfg = dict(cfg, dropout=p)
    P = ng.init_params(cfg, seed=seed, perturb=0.05)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=seed + 2)
    Ld = cfg.get("num_decoder_layers", 0)
    tgt = shift_right(y) if Ld else None
    rng = (1234, 99, 7)
    r = Runner(cfg, B, backend, rng=rng, seq=seq, flags=flags)
    r.set_params(P)
    hvo = r.forward(x, tgt, train=p > 0)
    (h, v, o), C = ng.forward(P, cfg, x, tgt=tgt, rng=rng if p > 0 else None, dtype=np.float64)
    dpred = _check_forward_and_loss(r, hvo, (h, v, o), C, y, penalty, check_ws)
    G = r.backward(train=p > 0)
    adopted = adopt_device_kinks(r, C, cfg)
    assert adopted <= kink_bound(r, cfg), adopted
    Gr = ng.backward(P, cfg, C, dpred, dtype=np.float64)
    assert set(G) == set(Gr)
    for k in Gr:
        # relative to the tensor's largest entry, with an absolute floor: a tensor that is numerically zero (|g| < 1e-5
        # everywhere -- e.g. LayerNorm gammas at d_model 2, where the normalised outputs are +-1 and the sum cancels; the
        # oracle's own fp32 run is 10 % off its fp64 run there) is compared absolutely
        err = float(np.abs(G[k] - Gr[k]).max() / max(np.abs(Gr[k]).max(), 1e-5))
        FIGURES["grad"] = max(FIGURES.get("grad", 0.0), err / GRAD_TOL)
        assert err < GRAD_TOL, (k, err)
    return r, P, G, Gr


# ---- the same step away from initialisation (tests/regimes.py) ------------------------------------------------------------------------------
def check_step_regime(backend, cfg, B, regime, p=0.0, penalty=0.47, seed=3, seq=True, flags=0):
    """check_step with the parameters moved by regimes.REGIMES[regime].  The fp32 oracle runs beside the fp64 one, and every compared
    quantity -- outputs, every encoder layer's saved P and hact, x0, memory, d loss / d hvo, each gradient tensor -- meets two bars:
    (1) check_step's fixed bar, with one correction: the hit-logit columns of the output are compared relative to max(1, max |h_ref|) (on
        logits of +-48 ... +-91 stock fp32 numpy is 2.9e-5 ... 4.1e-5 off fp64 absolutely, 3e-7 ... 6e-7 relative to the largest); the v and
        o columns stay absolute.  The saved P's fixed 1e-5 gives way to (2) (shift: the fp32 oracle's own P is 3.5e-6 ... 8.9e-6 off);
    (2) error <= regimes.NOISE_FACTOR x max(the fp32 oracle's error on that quantity, 4 ulp of its scale), asserted for all quantities
        together at the end (regimes.Noise.check), after the fixed bars.
    The regime's own condition is asserted on the fp64 cache first.  Records FIGURES (see above); returns (r, P, G, Gr)."""
    cfg = dict(cfg, dropout=p)
    P = regimes.apply(ng.init_params(cfg, seed=seed, perturb=0.05), cfg, regime, seed)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=seed + 2)
    Ld = cfg.get("num_decoder_layers", 0)
    tgt = shift_right(y) if Ld else None
    rng = (1234, 99, 7)
    orng = rng if p > 0 else None
    (h, v, o), C = ng.forward(P, cfg, x, tgt=tgt, rng=orng, dtype=np.float64)
    FIGURES.clear()
    FIGURES["regime"] = regimes.assert_condition(regime, C, h)
    (h32, v32, o32), C32 = ng.forward(P, cfg, x, tgt=tgt, rng=orng, dtype=np.float32)
    noise = regimes.Noise()
    FIGURES["noise_rows"] = noise.rows

    def done():
        name, _, _, _, ratio = noise.worst()
        FIGURES["noise"], FIGURES["noise_at"] = ratio, name

    try:
        r = Runner(cfg, B, backend, rng=rng, seq=seq, flags=flags)
        r.set_params(P)
        hvo = r.forward(x, tgt, train=p > 0)
        hs = max(1.0, float(np.abs(h).max()))
        e = noise.add("out.h", hvo[..., :9], h32, h, scale=hs)
        FIGURES["out"] = e / OUT_TOL
        assert e < OUT_TOL, "forward hit logits: max-abs %g of max |h| %g" % (e * hs, hs)
        vo, vo32 = np.concatenate([v, o], -1), np.concatenate([v32, o32], -1)
        e = noise.add("out.vo", hvo[..., 9:], vo32, vo, scale=hs) * hs
        FIGURES["out"] = max(FIGURES["out"], e / OUT_TOL)
        assert e < OUT_TOL, "forward v / o max-abs %g" % e
        saved = [("x0", 0, C["enc"][0]["x_in"], C32["enc"][0]["x_in"])]
        for l, (c, c32) in enumerate(zip(C["enc"], C32["enc"])):
            saved += [("P", l, c["attn"]["P"], c32["attn"]["P"]), ("hact", l, c["hact"], c32["hact"])]
        saved.append(("memory", 0, C["memory"], C32["memory"]))
        for name, l, ref, ref32 in saved:
            e = noise.add("%s[%d]" % (name, l), r.ws_get(name, l), ref32.reshape(-1), ref.reshape(-1))
            assert name == "P" or e < 1e-5, (name, l, e)
        stats, d_hvo = r.loss(y, penalty)
        rstats, dpred = ng.calculate_loss((h, v, o), y.astype(np.float64), penalty)
        for i in (0, 3, 4, 5):
            assert abs(stats[i] - rstats[i]) < 1e-5 * max(1.0, abs(rstats[i])), (i, stats[i], rstats[i])
        near = int((np.abs(h) < 1e-4).sum())
        assert abs(stats[1] - rstats[1]) <= (near + 0.01) / h.size + 1e-6, (stats[1], rstats[1], near)
        _, dpred32 = ng.calculate_loss((h32, v32, o32), y.astype(np.float32), np.float32(penalty))
        e = noise.add("d_hvo", d_hvo, np.concatenate(dpred32, -1), np.concatenate(dpred, -1))
        assert e < 1e-5, ("d_hvo", e)
        G = r.backward(train=p > 0)
        adopted = adopt_device_kinks(r, C, cfg)
        assert adopted <= kink_bound(r, cfg), adopted
        regimes.same_kinks(C32, C)
        Gr = ng.backward(P, cfg, C, dpred, dtype=np.float64)
        G32 = ng.backward(P, cfg, C32, dpred32, dtype=np.float32)
        assert set(G) == set(Gr)
        for k in Gr:
            err = noise.add(k, G[k], G32[k], Gr[k], scale=max(float(np.abs(Gr[k]).max()), 1e-5))
            FIGURES["grad"] = max(FIGURES.get("grad", 0.0), err / GRAD_TOL)
            assert err < GRAD_TOL, (k, err)
    finally:
        done()
    noise.check()
    return r, P, G, Gr


# ---- each sequence's share of the parameter gradients (check_grad_probes), accumulation (check_accumulate) ---------------------------------
# check_step's gradient bar is relative to the WHOLE batch's tensor, a sum over all 32 B tokens: one sequence's share of it is 1.4e-2 ...
# 2e-2 of the tensor's largest entry at 64 sequences and 3e-3 ... 6e-3 at 256, one token row's 2e-4 ... 3e-3 -- a sequence counted at 98 %,
# or a row lost at a partition's boundary, passes it.  gt_backward is linear in d_hvo and sequences meet only in the parameter gradients,
# so ONE forward and one backward per PROBE -- a d_hvo that is zero outside one sequence, or one token row -- puts the same bar,
# GRAD_TOL, on that sequence's (row's) contribution alone.  The oracle's own fp32 run differs from its fp64 run by <= 8.3e-7 on such
# probes (d128 B 17, d32 encoder-decoder B 5, d256 B 64, d32 / H16 B 16): the bar keeps 240 x over the reference.
PROBE_FLOOR = 1e-3               # every oracle tensor of every probe must reach this (the smallest seen: 1.5e-2): the 1e-5 floor never engages
MAX_PROBES = 12


def gradient_gaps(r):
    """the flat gradient buffer's elements outside every tensor of the layout: alignment gaps and the guard element (the last one)"""
    inside = np.zeros(r.total, bool)
    for off, size, _, _ in r.entries:
        inside[off:off + size] = True
    assert not inside[-1], "the guard element lies inside a tensor"
    return ~inside


def assert_gaps_zero(r, gaps, tag):
    """gt_clip_grad_norm sums the whole buffer: whatever a backward leaves outside the tensors counts as gradient"""
    g = r.grads.numpy()
    bad = np.flatnonzero(g[gaps] != 0)
    assert bad.size == 0, "%s: %d non-zero elements outside the gradient tensors, first at flat index %d" % (tag, bad.size, np.flatnonzero(gaps)[bad[0]])


def probe_d_hvo(B, place, seed):
    """d loss / d hvo of one probe.  place = ("seq", s): sequence s; ("row", t): token row t of the 32 B (sequence t // 32, step t % 32).
    U(-1, 1) in float32 inside, exactly zero outside."""
    d = np.zeros((B * 32, 27), np.float32)
    rnd = np.random.default_rng(seed)
    kind, at = place
    if kind == "seq":
        assert 0 <= at < B, place
        d[32 * at:32 * at + 32] = rnd.uniform(-1, 1, (32, 27)).astype(np.float32)
    else:
        assert kind == "row" and 0 <= at < 32 * B, place
        d[at] = rnd.uniform(-1, 1, 27).astype(np.float32)
    return d.reshape(B, 32, 27)


def probe_places(B, token_rows=(), split_rows=True, limit=None):
    """Where the token dimension of the weight gradients is cut.  Always sequences 0 and B - 1 and the last row of the batch; split_rows:
    rows 15 and 16 of sequence B // 2 (the two 16-row halves of the two-workgroups-per-sequence kernels); token_rows: the caller's
    boundaries (chunk ends from the dispatch trace, ride_last_k, the tail's chunk), in the caller's order, rows outside the batch dropped.
    No place twice, at most limit (MAX_PROBES) of them."""
    M = 32 * B
    places = [("seq", 0), ("seq", B - 1)]
    if split_rows:
        places += [("row", 32 * (B // 2) + 15), ("row", 32 * (B // 2) + 16)]
    places.append(("row", M - 1))
    places += [("row", int(t)) for t in token_rows if 0 <= t < M]
    out = []
    for pl in places:
        if pl not in out:
            out.append(pl)
    return out[:min(limit or MAX_PROBES, MAX_PROBES)]


def chunk_rows(trace, M):
    """token rows either side of the first chunk boundary, and the first row of the last chunk, for every distinct k_chunk among the
    trace's queued weight-gradient problems over M tokens (family "wgrad_queue"); the chunk length of the largest gradient first"""
    size = {}
    for d in harness.dispatched(trace, "wgrad_queue"):
        if d["K"] == M and d["k_chunk"] < M:
            size[d["k_chunk"]] = max(size.get(d["k_chunk"], 0), d["M"] * d["N"])
    rows = []
    for kc in sorted(size, key=lambda k: (-size[k], k)):
        rows += [kc - 1, kc, (M - 1) // kc * kc]
    return rows


def rider_rows(M):
    """the rider path's cuts (csrc/groove_hip.hip backward_impl, csrc/gt_seq_wg.h seq_wg_phase_unit, restated): the last phase's riders take
    the tokens [0, ride_last_k) and the tail launch the rest; the tail's own problems are cut into ks = 2 chunks of `per` tokens"""
    ride_last_k = (M * 50 // 100) // 64 * 64
    ks = 2
    per = ((M // 8 + ks - 1) // ks) * 8
    return [ride_last_k - 1, ride_last_k, per - 1, per]


def probe_compare(G, Gr, place):
    """One probe's gradients G (name -> array) against the oracle's Gr: max |G - Gr| / max(max |Gr|, 1e-5) < GRAD_TOL per tensor -- check_step's
    bar, relative to THIS probe's tensor.  AssertionError naming the probe, the tensor and the element; ValueError when an oracle tensor
    stays under PROBE_FLOOR (the probe says nothing about that tensor: take another probe seed).  Returns the worst err / GRAD_TOL."""
    assert set(G) == set(Gr), sorted(set(G) ^ set(Gr))
    worst = 0.0
    for k in Gr:
        ref = np.asarray(Gr[k], np.float64)
        top = float(np.abs(ref).max())
        if top < PROBE_FLOOR:
            raise ValueError("probe %s: max |G_ref| of %s is %.3g < %g -- pick another probe seed" % (place, k, top, PROBE_FLOOR))
        diff = np.abs(np.asarray(G[k], np.float64).reshape(ref.shape) - ref)
        err = float(diff.max() / max(top, 1e-5))
        worst = max(worst, err / GRAD_TOL)
        if not err < GRAD_TOL:
            i = tuple(int(j) for j in np.unravel_index(int(np.argmax(diff)), ref.shape))
            raise AssertionError("probe %s: %s element %s: device %.9g oracle %.9g, error %.3g of the probe's max |G_ref| %.3g (bar %g)"
                                 % (place, k, i, np.asarray(G[k]).reshape(ref.shape)[i], ref[i], err, top, GRAD_TOL))
    return worst


def _deterministic(lib, on):
    import contextlib

    @contextlib.contextmanager
    def cm():
        if on:
            lib.cdll.gt_set_deterministic(1)
        try:
            yield
        finally:
            if on:                                   # (unset: back to what the environment asks for, else the library's default)
                lib.cdll.gt_set_deterministic(-1)
    return cm()


def check_grad_probes(backend, cfg, B, p, probes, seq=True, flags=0, precision=0, deterministic=False, penalty=0.47, seed=3, probe_seed=100):
    """One forward, then one backward per probe (probe_d_hvo), each against the oracle's backward of the same probe from the SAME fp64
    forward cache (device's ReLU decisions adopted once, as in check_step); check_step's forward assertions unchanged.  After every
    backward the buffer's gaps and guard element are exactly zero.
    probes: a list of places (probe_places), or a callable (trace, M) -> such a list, given the dispatch trace of one full step (forward,
    loss backward) that runs first in either case.  precision 1: the per-operation check of the bf16 path (check_ops_bf16, bars
    unchanged) per probe instead of the end-to-end comparison -- with a sparse dlogits its weight-gradient lines are sharp by themselves.
    deterministic: under gt_set_deterministic(1), put back afterwards.
    Records FIGURES["probe"] (worst error / bar); returns (r, trace of the full step, places)."""
    cfg = dict(cfg, dropout=p)
    if precision:
        cfg["precision"] = precision
    lib = harness.emu_lib() if backend == "emu" else harness._lib.get_lib()
    with _deterministic(lib, deterministic):
        return _check_grad_probes(backend, cfg, B, p, probes, seq, flags, penalty, seed, probe_seed)


def _check_grad_probes(backend, cfg, B, p, probes, seq, flags, penalty, seed, probe_seed):
    precision = cfg.get("precision", 0)
    P = ng.init_params(cfg, seed=seed, perturb=0.05)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=seed + 2)
    Ld = cfg.get("num_decoder_layers", 0)
    tgt = shift_right(y) if Ld else None
    rng = (1234, 99, 7)
    train = p > 0
    r = Runner(cfg, B, backend, rng=rng, seq=seq, flags=flags)
    r.set_params(P)
    gaps = gradient_gaps(r)
    hvo, trace = harness.trace_dispatch(lambda: r.forward(x, tgt, train=train))
    (h, v, o), C = ng.forward(P, cfg, x, tgt=tgt, rng=rng if train else None, dtype=np.float64)
    if precision == 0:
        _check_forward_and_loss(r, hvo, (h, v, o), C, y, penalty, True)
    else:                                            # check_step_bf16's end-to-end sanity bound on the forward
        (h0, v0, o0), _ = ng.forward(P, dict(cfg, precision=0), x, tgt=tgt, rng=rng if train else None, dtype=np.float64)
        ref, ref0 = np.concatenate([h, v, o], -1), np.concatenate([h0, v0, o0], -1)
        eq = _rms(ref0 - ref)
        assert eq > 1e-5, "the bf16 rounding has no visible effect on this case: pick another"
        assert np.abs(hvo - ref).max() < BF16_OUT_MAX, "forward max-abs %g" % np.abs(hvo - ref).max()
        frac = BF16_E2E_FRAC if r.precision_in_force() < 2 else 2.5
        FIGURES.clear()
        FIGURES["bf16_e2e"] = _rms(hvo - ref) / (frac * eq + 1e-5)
        assert _rms(hvo - ref) <= frac * eq + 1e-5, "forward rms %g vs bf16 effect %g" % (_rms(hvo - ref), eq)
        stats, _ = r.loss(y, penalty)
        rstats, _ = ng.calculate_loss((h, v, o), y.astype(np.float64), penalty)
        assert abs(stats[0] - rstats[0]) < 1e-2 * max(1.0, abs(rstats[0]))
    _, bwd_trace = harness.trace_dispatch(lambda: r.backward(train=train))          # the whole batch's backward: the path every probe takes
    trace = trace + bwd_trace
    assert_gaps_zero(r, gaps, "whole batch")
    if precision == 0:
        adopted = adopt_device_kinks(r, C, cfg)
        assert adopted <= kink_bound(r, cfg), adopted
    places = list(probes(trace, r.M)) if callable(probes) else list(probes)
    assert 1 <= len(places) <= MAX_PROBES and len(set(places)) == len(places), places
    ran = 0
    for i, place in enumerate(places):
        d = probe_d_hvo(B, place, probe_seed + i)
        G = r.backward(d, train=train)
        assert_gaps_zero(r, gaps, "probe %s" % (place,))
        if precision == 0:
            Gr = ng.backward(P, cfg, C, (d[..., :9], d[..., 9:18], d[..., 18:]), dtype=np.float64)
            ratio = probe_compare(G, Gr, place)
        else:
            FIGURES.pop("bf16_op", None)
            BF16_FIGURES.clear()
            try:
                check_ops_bf16(r, P, cfg, x, tgt, rng, p, G, forward_checks=(i == 0))
            except AssertionError as e:
                raise AssertionError("probe %s: %s" % (place, e)) from None
            ratio = FIGURES["bf16_op"]
        FIGURES["probe"] = max(FIGURES.get("probe", 0.0), ratio)
        ran += 1
    assert ran == len(places), (ran, len(places))
    return r, trace, places


ACC_TOL = 2e-6                   # check_bucketed_backward's bar for two summation orders of the same gradient


def check_accumulate(backend, cfg, B, p, seq=True, flags=0, penalty=0.47, seed=3):
    """gt_backward(accumulate = 1) -- what the nn.Module path always passes, and what selects the adding store modes of the sequence-resident
    weight-gradient units -- onto a NON-ZERO gradient buffer.  G0: multiples of 2^-10 in [-1, 1] inside the tensors, zero in the gaps and the
    guard element.  d: the loss's d_hvo.
    (a) buffer = G0; backward(d, accumulate=1)             must equal  G0 + backward(d, accumulate=0)
    (b) buffer = G0; backward(d1, accumulate=0) (overwrites); backward(d2, accumulate=1)   must equal  backward(d1 + d2, accumulate=0),
        d1 = d on the first half of the sequences, d2 = d on the second half.
    Bar per element: ACC_TOL x max |expected buffer| + np.spacing(|expected|) -- check_bucketed_backward's bar, whose max is taken over the
    whole flat buffer too.  In (a) that buffer is G0 + g, so the bar is about 2e-6: up to 32 partial tiles adding onto an element of size 1
    round by 2^-24 each (worst case 1.9e-6); a store in place of an add, or a chunk added twice, is off by |G0| or |g| themselves.
    Gaps and guard element stay zero.  Records FIGURES["accumulate"] (worst error / bar); returns the Runner."""
    cfg = dict(cfg, dropout=p)
    P = ng.init_params(cfg, seed=seed, perturb=0.05)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=seed + 2)
    tgt = shift_right(y) if cfg.get("num_decoder_layers", 0) else None
    train = p > 0
    r = Runner(cfg, B, backend, rng=(1234, 99, 7), seq=seq, flags=flags)
    r.set_params(P)
    gaps = gradient_gaps(r)
    r.forward(x, tgt, train=train)
    _, d = r.loss(y, penalty)
    rnd = np.random.default_rng(seed + 40)
    G0 = np.zeros(r.total, np.float32)
    for off, size, _, _ in r.entries:
        G0[off:off + size] = (rnd.integers(-1024, 1025, size) / 1024.0).astype(np.float32)
    d1, d2 = d.copy(), d.copy()
    d1[B // 2:] = 0
    d2[:B // 2] = 0
    assert np.abs(d1).max() > 0 and np.abs(d2).max() > 0

    def run(dh, accumulate, start=None):
        if start is not None:
            r.grads = r.Buf(start.copy())
        r.backward(dh, train=train, accumulate=accumulate)
        return r.grads.numpy().astype(np.float64)

    def close(got, want, what):
        bar = ACC_TOL * np.abs(want).max() + np.spacing(np.abs(want))
        err = np.abs(got - want)
        FIGURES["accumulate"] = max(FIGURES.get("accumulate", 0.0), float((err / bar).max()))
        if (err > bar).any():
            i = int(np.argmax(err - bar))
            name = [n for (n, _), (off, size, _, _) in zip(r.names, r.entries) if off <= i < off + size]
            raise AssertionError("%s: %s flat element %d: got %.9g want %.9g, |err| %.3g > bar %.3g (%d elements over)"
                                 % (what, name[0] if name else "gap", i, got[i], want[i], err[i], bar[i], int((err > bar).sum())))

    FIGURES.pop("accumulate", None)
    g = run(d, 0, np.zeros(r.total, np.float32))
    assert np.abs(g).max() > 0
    assert_gaps_zero(r, gaps, "accumulate = 0")
    ga = run(d, 1, G0)                               # (a)
    close(ga, G0.astype(np.float64) + g, "(a) backward(d, accumulate=1) onto G0")
    assert_gaps_zero(r, gaps, "(a)")
    run(d1, 0, G0)                                   # (b): the first call overwrites G0
    gb = run(d2, 1)
    close(gb, g, "(b) backward(d1) then backward(d2, accumulate=1)")
    assert_gaps_zero(r, gaps, "(b)")
    return r


# ---- bf16 operand path (gt_config.precision = 1, BASELINE configs[4]) -------------------------------------------------------
# Two bars.
# (1) PER OPERATION, teacher-forced (check_ops_bf16): every Linear of the forward and of the backward is recomputed in fp64
#     from the DEVICE's own saved inputs (workspace activations / gradient temporaries), its two operands rounded to bf16 at
#     exactly the points the device rounds them (oracle.numpy_groove.round_bf16), and compared with the device's output of
#     that one operation.  Nothing propagates, so the bar is the fp32 one: 5e-5 of the tensor's largest entry (fp32
#     accumulation over up to 16384 terms), LayerNorm / activation epilogues included.  This is the parity proof.
#     The other operations -- attention cores, LayerNorm passes, dropout masks on gradients, d loss / d logits -- are restated the same way
#     under the bar of their class (_bar_class), and the walk asserts its own CLOSURE (Ledger): no gradient tensor left uncompared, no device
#     tensor read as an input that an earlier operation of the walk did not compare.
# (2) END TO END against the bf16-operand oracle (oracle "bf16 operand mode").  Here differences DO propagate: an operand the
#     device computed 6e-8 (relative) away from the oracle's value rounds to the neighbouring bf16 now and then, that moves
#     its row by ~1e-3, and from there on the rest of the sequence rounds differently too -- two legitimate realisations of
#     the same rounding noise decorrelate.  So this bar is a sanity bound, relative to the bf16 effect itself
#     E_q = RMS(fp32-operand oracle - bf16-operand oracle):  RMS(device - bf16 oracle) <= 1.5 E_q + 1e-5, max-abs <= 5e-2,
#     loss within 1 %.
BF16_OP_TOL, BF16_E2E_FRAC, BF16_OUT_MAX = 5e-5, 1.5, 5e-2


def _rms(a):
    return float(np.sqrt((np.asarray(a, np.float64) ** 2).mean()))


def _bar_class(tol, rms_tol):
    """the name BF16_FIGURES["ops"] files a comparison under: the walk's bar classes"""
    if rms_tol is not None:
        return "behind a hidden bf16 rounding (max %.3g, rms %.3g)" % (tol, rms_tol)
    return {BF16_OP_TOL: "matmul-like, fp32 accumulation (5e-5)", 2e-5: "probabilities / LayerNorm forward (2e-5)",
            1e-4: "dgrad + LayerNorm backward, LayerNorm parameter gradients (1e-4)", 1e-6: "dropout mask on a gradient (1e-6)"}.get(tol, "%g" % tol)


def _close(dev, ref, what, tol=BF16_OP_TOL, where=None, stored16=False, rms_tol=None, ref32=None):
    """stored16: the device keeps this tensor in bf16 alone (operand-only tensors, gt_set_operand_shadows level 2) -- what is read back
    is the RNE rounding of the value the bar applies to, so each element may additionally be off by half a bf16 ulp of itself (2^-9;
    2^-8 allowed: the fp32 value may sit a hair on the other side of a rounding boundary).
    ref32: () -> the same restatement evaluated in np.float32 from the same inputs.  Consulted only when the comparison misses its class
    bar: if that fp32 restatement is itself more than 1 / 8 of the bar away from the fp64 one, the bar of this one comparison becomes
    regimes.NOISE_FACTOR x the restatement's own error (recorded in BF16_FIGURES["widened"]); otherwise the miss stands.
    Records FIGURES["bf16_op"] (the worst error / bar ratio) and, in BF16_FIGURES, "op_at" (that comparison's name) and "ops" (bar class ->
    (worst ratio, its comparison's name))."""
    dev, ref = np.asarray(dev, np.float64).reshape(ref.shape), np.asarray(ref, np.float64)
    err = np.abs(dev - ref)
    if stored16:
        err = np.maximum(err - np.abs(ref) * 2.0 ** -8, 0.0)
    if where is not None:
        err = err * where
    scale = max(float(np.abs(ref).max()), 1e-6)
    bar = tol * scale
    if not err.max() <= bar and ref32 is not None:
        noise = float(np.abs(np.asarray(ref32(), np.float64).reshape(ref.shape) - ref).max())
        if noise > bar / 8:
            BF16_FIGURES.setdefault("widened", []).append((what, bar / scale, noise / scale, float(err.max()) / scale))
            bar = regimes.NOISE_FACTOR * noise
            import warnings
            warnings.warn("%s: class bar %.3g widened to %.3g (the np.float32 restatement is %.3g off; device %.3g)"
                          % (what, tol, bar / scale, noise / scale, float(err.max()) / scale))
    ratio = float(err.max() / bar)
    if ratio >= FIGURES.get("bf16_op", 0.0):
        FIGURES["bf16_op"], BF16_FIGURES["op_at"] = ratio, what
    rows = BF16_FIGURES.setdefault("ops", {})
    cls = _bar_class(tol, rms_tol)
    if ratio >= rows.get(cls, (0.0, None))[0]:
        rows[cls] = (ratio, what)
    assert err.max() <= bar, "%s: max |err| %.3g of max |ref| %.3g (ratio %.3g, bar %.3g)" % (what, err.max(), scale, err.max() / scale, bar / scale)
    if rms_tol is not None:      # behind a HIDDEN bf16 rounding single elements may sit one ulp off (max bar 2^-8-ish); on average nothing may
        assert _rms(err) <= rms_tol * scale, "%s: rms err %.3g of max |ref| %.3g (ratio %.3g)" % (what, _rms(err), scale, _rms(err) / scale)


class Ledger:
    """What one walk of check_ops_bf16 has proved, kept so that the walk can assert its own closure.  A tensor is named "<region>[<layer>]"
    (workspace regions, as gt_ws_find names them), "hvo" or "d_hvo".
    compared: tensor -> the first comparison that covered it.  consumed: tensor -> why the walk may read it as a teacher-forcing input
    ("compared: ..." by an EARLIER operation of the same walk, or the probe's d_hvo the test itself supplied), None if nothing admits it.
    cover: gradient key -> which of its rows some comparison covered (the packed in-proj tensors are compared slice by slice).
    The true inputs of the step -- x, tgt, the parameters, y -- come from the caller, not from the device, and are not recorded.
    forward_checks=False (check_grad_probes' probes after the first: another backward from the SAME forward): the forward's comparisons are
    not repeated; the ledger enters them as "by the first walk of this forward" and the closure assertion runs all the same."""

    def __init__(self, G, forward_checks, d_hvo_supplied):
        self.compared, self.consumed = {}, {}
        self.forward_by_first_walk = not forward_checks
        self.d_hvo_supplied = d_hvo_supplied
        self.cover = None if G is None else {k: np.zeros(np.shape(v)[0], bool) for k, v in G.items()}

    @staticmethod
    def key(name, layer=None):
        return name if layer is None else "%s[%d]" % (name, layer)

    def did_compare(self, key, what):
        if isinstance(key, tuple):                   # ("grad", the gradient's key, which of its rows)
            self.cover[key[1]][key[2]] = True
        else:
            self.compared.setdefault(key, what)

    def consume(self, key):
        if key in self.consumed:
            return
        if key in self.compared:
            self.consumed[key] = "compared: " + self.compared[key]
        elif key == "d_hvo" and self.d_hvo_supplied:
            self.consumed[key] = "supplied by the test (probe)"
        else:
            self.consumed[key] = None

    def verdict(self):
        """(gradient keys -- or row ranges of them -- no comparison covered, consumed tensors nothing admits), both in the walk's order"""
        grads = []
        for k, c in (self.cover or {}).items():
            if not c.any():
                grads.append(k)
            elif not c.all():
                miss = np.flatnonzero(~c)
                grads.append("%s rows %d..%d" % (k, miss[0], miss[-1]))
        return grads, [k for k, how in self.consumed.items() if how is None]

    def assert_closed(self):
        grads, tensors = self.verdict()
        assert not grads and not tensors, ("the per-operation walk is not closed -- gradient tensors no operation compared: %s; device tensors consumed "
                                           "as inputs that no earlier operation compared: %s" % (grads or "none", tensors or "none"))


def _ledger_compare(led, key, dev, ref, what, **kw):
    """One comparison of the walk: dev() reads the device's tensor, ref is the fp64 restatement -- an array, or dt -> array for the operations
    that can also be restated in np.float32 (_close's ref32).  Only a comparison that held enters the ledger."""
    if callable(ref):
        _close(dev(), ref(np.float64), what, ref32=lambda: ref(np.float32), **kw)
    else:
        _close(dev(), ref, what, **kw)
    led.did_compare(key, what)


def check_ops_bf16(r, P, cfg, x, tgt, rng, p, G=None, forward_checks=True):
    """Teacher-forced per-operation parity of the bf16 path (bar (1) above).  r: Runner after forward (and, with G = the device's
    gradients, after loss + backward).  forward_checks=False: only the backward half is compared (a second backward from the same forward:
    check_grad_probes) -- the forward half is still walked for its operands.
    The walk keeps a Ledger and asserts its own closure at the end: every device tensor it read as an input was the compared output of an
    earlier operation (or the probe's d_hvo), and, with G, every gradient tensor was compared, the packed ones slice by slice.  The Ledger
    stays in BF16_FIGURES["ledger"].  Returns the number of comparisons."""
    rb = ng.round_bf16
    f64 = lambda a: np.asarray(a, np.float64)
    P = {k: f64(v) for k, v in P.items()}
    d, F, H = cfg["d_model"], cfg["dim_feedforward"], cfg["n_heads"]
    L, Ld = cfg["num_encoder_layers"], cfg.get("num_decoder_layers", 0)
    M = r.M
    pe = np.tile(f64(ng.positional_encoding(d)), (M // 32, 1))
    scale = 1.0 / (1.0 - float(np.float32(p))) if p > 0 else 1.0
    led = Ledger(G, forward_checks, getattr(r, "d_hvo_from", None) == "caller")
    BF16_FIGURES["ledger"] = led
    if G is not None:
        G = {k: f64(v) for k, v in G.items()}
    n = 0

    def mask(site, n, shape=None):
        m = ng.keep_mask(rng, site, n, p) if p > 0 else None
        return 1.0 if m is None else (m if shape is None else m.reshape(shape))

    def ws(name, layer=0, cols=None):
        """a device tensor CONSUMED as a teacher-forcing input (the ledger wants it compared before)"""
        led.consume(Ledger.key(name, layer))
        a = f64(r.ws_get(name, layer))
        return a.reshape(M, -1) if cols is None else a.reshape(-1, cols)

    def tname(name):                                      # (without dropout the masked copies are the tensors themselves)
        return name[:-1] if (p == 0 and name in ("dzAm", "dzBm", "dzCm")) else name

    def tmp(name, gl, cols):
        return ws(tname(name), gl, cols)

    def cmp(name, layer, ref, what, fwd=False, **kw):
        """compare region `name` of `layer` (None: r.hvo) with its restatement; fwd: a comparison of the forward half"""
        nonlocal n
        n += 1
        key = Ledger.key(tname(name), layer)
        if fwd and not forward_checks:
            led.did_compare(key, what + " (by the first walk of this forward)")
            return
        _ledger_compare(led, key, (lambda: r.hvo.numpy()) if name == "hvo" else (lambda: r.ws_get(tname(name), layer)), ref, what, **kw)

    def gcmp(key, ref, what, rows=slice(None), **kw):
        """compare (rows of) gradient tensor G[key]"""
        nonlocal n
        n += 1
        _ledger_compare(led, ("grad", key, rows), lambda: G[key][rows], ref, what, **kw)

    def memo(fn):
        got = {}
        return lambda dt: got[dt] if dt in got else got.setdefault(dt, fn(dt))

    def lin(a, w, b=None):
        y = rb(a) @ rb(w).T
        return y if b is None else y + b

    def ln(z, g, b):
        mu = z.mean(-1, keepdims=True)
        var = ((z - mu) ** 2).mean(-1, keepdims=True)
        rstd = 1.0 / np.sqrt(var + 1e-5)
        xh = (z - mu) * rstd
        return xh * g + b, xh, rstd

    def ln_bwd(dy, xh, rstd, g):
        gdy = dy * g
        return rstd * (gdy - gdy.mean(-1, keepdims=True) - xh * (gdy * xh).mean(-1, keepdims=True)), (dy * xh).sum(0), dy.sum(0)

    # precision 2 (encoder layers): Linear outputs are STORED in bf16 -- qkv and dqkv observably (stored16), the out-proj / linear2 outputs
    # ahead of their LayerNorm and the dgrad outputs ahead of a LayerNorm backward only transiently: the oracle rounds the same value (hrb)
    # and an element whose fp32 and fp64 values straddle a rounding boundary lands one bf16 ulp apart -- max bar 2^-7 of the tensor's
    # largest entry, RMS bar 2e-4 (the flips are rare)
    P2 = r.precision_in_force() == 2
    hrb = (lambda a: rb(a)) if P2 else (lambda a: a)
    HID = dict(tol=2.0 ** -7, rms_tol=2e-4) if P2 else {}
    HIDB = dict(tol=2.0 ** -7, rms_tol=4e-4)             # ... and behind a hidden rounding in the backward
    heads, hd = cfg["n_heads"], cfg["d_model"] // cfg["n_heads"]

    def split_heads(a):                                   # (M, d) -> (B, H, 32, hd)
        return a.reshape(M // 32, 32, heads, hd).transpose(0, 2, 1, 3)

    def merge_heads(a):
        return a.transpose(0, 2, 1, 3).reshape(M, heads * hd)

    def probs(name, gl, dt):                              # the device's saved probabilities (B, H, 32, 32)
        return ws(name, gl, 32).reshape(M // 32, heads, 32, 32).astype(dt)

    # ---- the attention core, one helper per direction for the three kinds (encoder self, decoder masked self, decoder cross).  Its arithmetic
    # is fp32 at every precision (precision 2 only STORES q / k / v / dctx in bf16: ws() widens them), so the bars are the fp32 class bars
    # unless an operand was rounded out of sight (precision 2's dctx).  qkv_of() -> the device's saved (q, k, v), each (M, d)
    def attn_core(pre, gl, kind, qkv_of, Pname, ctxname, site, causal):
        enc2 = P2 and gl < L

        def p_ref(dt):
            q_, k_ = (split_heads(a.astype(dt)) for a in qkv_of()[:2])
            sc = (q_ @ k_.transpose(0, 1, 3, 2)) * dt(1.0 / np.sqrt(hd))
            if causal:
                sc = sc + np.triu(np.full((32, 32), -np.inf, dt), 1)
            e = np.exp(sc - sc.max(-1, keepdims=True))
            return e / e.sum(-1, keepdims=True)

        def ctx_ref(dt):
            pr = probs(Pname, gl, dt)
            return merge_heads((pr * np.asarray(mask(site, pr.size, pr.shape), dt)) @ split_heads(qkv_of()[2].astype(dt)))

        cmp(Pname, gl, p_ref, pre + ("attention probabilities over bf16-stored q / k" if enc2 else kind + " attention probabilities"), fwd=True, tol=2e-5)
        if causal and forward_checks:
            above = r.ws_get(Pname, gl).reshape(-1, 32, 32)[:, np.triu(np.ones((32, 32), bool), 1)]
            assert not above.any(), "%s%s attention: %d probabilities above the diagonal are not exactly 0" % (pre, kind, int((above != 0).sum()))
        cmp(ctxname, gl, ctx_ref, pre + ("attention output over bf16-stored v" if enc2 else kind + " attention output"), fwd=True,
            stored16=r.bf16_only(ctxname, gl))

    def attn_core_bwd(pre, gl, kind, qkv_of, Pname, site, dzm_of, wo, outname, flat):
        """dq, dk, dv from the saved q, k, v, P, the dropout mask and dctx = the out-proj dgrad of the (compared) masked dz; flat: the cross
        attention's layout [dq (M, d) | dk, dv (M, 2d)], else one (M, 3d) tensor"""
        enc2 = P2 and gl < L                             # attn_bwd_lds_kernel, IN16: dctx itself is stored in bf16

        def ref(dt):
            dctx = rb(dzm_of()).astype(dt) @ rb(wo).astype(dt)
            if enc2:
                dctx = rb(dctx)
            q_, k_, v_ = (split_heads(a.astype(dt)) for a in qkv_of())
            pr = probs(Pname, gl, dt)
            mk = np.asarray(mask(site, pr.size, pr.shape), dt)
            do = split_heads(dctx)
            dp = (do @ v_.transpose(0, 1, 3, 2)) * mk
            ds = pr * (dp - (dp * pr).sum(-1, keepdims=True)) * dt(1.0 / np.sqrt(hd))
            dq, dk, dv = merge_heads(ds @ k_), merge_heads(ds.transpose(0, 1, 3, 2) @ q_), merge_heads((pr * mk).transpose(0, 1, 3, 2) @ do)
            return np.concatenate([dq.reshape(-1), np.concatenate([dk, dv], 1).reshape(-1)]) if flat else np.concatenate([dq, dk, dv], 1)

        if enc2:
            cmp(outname, gl, ref, pre + "attention backward over bf16-stored operands", tol=2.0 ** -6, rms_tol=2e-3)
        else:
            cmp(outname, gl, ref, pre + kind + " attention backward", stored16=r.bf16_only(outname, gl))

    def self_qkv(gl):
        def of():
            qkv = ws("qkv", gl)
            return tuple(qkv[:, i * d:(i + 1) * d] for i in range(3))
        return of

    def cross_qkv(gl):
        def of():
            kv = ws("kvx", gl)
            return ws("qx", gl), kv[:, :d], kv[:, d:]
        return of

    # ---------------------------------------------------------------------------------------------- forward
    def input_layer(xin, pre, a0name, outname, site):
        a = lin(f64(xin).reshape(M, -1), P[pre + "weight"], P[pre + "bias"])
        safe = np.abs(a) > 1e-4
        cmp(a0name, 0, a, pre + "pre-activation", fwd=True)
        cmp(outname, 0, (np.maximum(a, 0) + pe) * mask(site, a.size, a.shape), pre + "output", fwd=True, where=safe)

    def attn_block(name, gl, xin, inw, qkvname, ctxname, outname, xhname, rstdname, normname, site, q_rows=None):
        enc = P2 and gl < L
        out = lin(ws(ctxname, gl), P[name + "out_proj.weight"], P[name + "out_proj.bias"])
        out = (hrb(out) if enc else out) * mask(site, M * d, (M, d))
        y, xh, rstd = ln(xin + out, P[normname + ".weight"], P[normname + ".bias"])
        cmp(outname, gl, y, "%s out-proj + norm (layer %d)" % (name, gl), fwd=True, **(HID if enc else dict(tol=2e-5)))
        cmp(xhname, gl, xh, "%s xhat (layer %d)" % (name, gl), fwd=True, **(HID if enc else dict(tol=2e-5)))
        cmp(rstdname, gl, rstd, "%s rstd (layer %d)" % (name, gl), fwd=True, **(HID if enc else dict(tol=2e-5)))
        return ws(outname, gl)

    def ffn_block(pre, gl, xin, normname, outname="xout"):
        hp = lin(xin, P[pre + "linear1.weight"], P[pre + "linear1.bias"])
        cmp("hact", gl, np.maximum(hp, 0) * mask(ng.layer_site(gl, ng.S_FFN), hp.size, hp.shape),
            pre + "linear1", fwd=True, where=np.abs(hp) > 1e-4, stored16=r.bf16_only("hact", gl))
        enc = P2 and gl < L - 1          # (the top encoder layer's linear2 feeds the two-norm pass from fp32)
        f = lin(ws("hact", gl), P[pre + "linear2.weight"], P[pre + "linear2.bias"])
        f = (hrb(f) if enc else f) * mask(ng.layer_site(gl, ng.S_DROPF), M * d, (M, d))
        y, xh, rstd = ln(xin + f, P[pre + normname + ".weight"], P[pre + normname + ".bias"])
        cmp(outname, gl, y, pre + "linear2 + norm", fwd=True, **(HID if enc else dict(tol=2e-5)))
        cmp("xhat2", gl, xh, pre + normname + " xhat", fwd=True, **(HID if enc else dict(tol=2e-5)))
        cmp("rstd2", gl, rstd, pre + normname + " rstd", fwd=True, **(HID if enc else dict(tol=2e-5)))
        return ws(outname, gl)

    input_layer(x, "InputLayerEncoder.Linear.", "a0", "x0", ng.SITE_PE_ENC)
    cur = ws("x0")
    enc_in = []
    for l in range(L):
        pre = "Encoder.Encoder.layers.%d." % l
        enc_in.append(cur)
        cmp("qkv", l, lin(cur, P[pre + "self_attn.in_proj_weight"], P[pre + "self_attn.in_proj_bias"]), pre + "in_proj", fwd=True,
            stored16=r.bf16_only("qkv", l))
        attn_core(pre, l, "self", self_qkv(l), "P", "ctx", ng.layer_site(l, ng.S_ATTN), False)
        x1 = attn_block(pre + "self_attn.", l, cur, None, "qkv", "ctx", "x1", "xhat1", "rstd1", pre + "norm1", ng.layer_site(l, ng.S_DROP1))
        cur = ffn_block(pre, l, x1, "norm2")
    mem, xh, rstd = ln(cur, P["Encoder.Encoder.norm.weight"], P["Encoder.Encoder.norm.bias"])
    cmp("memory", 0, mem, "final encoder norm", fwd=True, tol=2e-5)
    cmp("enc_xhat", 0, xh, "final encoder norm xhat", fwd=True, tol=2e-5)
    cmp("enc_rstd", 0, rstd, "final encoder norm rstd", fwd=True, tol=2e-5)
    final = ws("memory")
    dec_in = []
    if Ld:
        input_layer(tgt, "InputLayerDecoder.Linear.", "b0", "y0", ng.SITE_PE_DEC)
        ycur = ws("y0")
        for l in range(Ld):
            pre, gl = "Decoder.Decoder.layers.%d." % l, L + l
            dec_in.append(ycur)
            cmp("qkv", gl, lin(ycur, P[pre + "self_attn.in_proj_weight"], P[pre + "self_attn.in_proj_bias"]), pre + "self in_proj", fwd=True)
            attn_core(pre, gl, "masked self", self_qkv(gl), "P", "ctx", ng.layer_site(gl, ng.S_ATTN), True)
            y1 = attn_block(pre + "self_attn.", gl, ycur, None, "qkv", "ctx", "x1", "xhat1", "rstd1", pre + "norm1", ng.layer_site(gl, ng.S_DROP1))
            wx, bx = P[pre + "multihead_attn.in_proj_weight"], P[pre + "multihead_attn.in_proj_bias"]
            cmp("qx", gl, lin(y1, wx[:d], bx[:d]), pre + "cross q in_proj", fwd=True)
            cmp("kvx", gl, lin(final, wx[d:], bx[d:]), pre + "cross kv in_proj", fwd=True)
            attn_core(pre, gl, "cross", cross_qkv(gl), "Px", "ctxx", ng.layer_site(gl, ng.S_XATTN), False)
            y2 = attn_block(pre + "multihead_attn.", gl, y1, None, "qx", "ctxx", "x2", "xhatx", "rstdx", pre + "norm2", ng.layer_site(gl, ng.S_DROP2))
            ycur = ffn_block(pre, gl, y2, "norm3")
        # (dec_xhat / dec_rstd have no public name: the backward below takes the fp64 ones of the saved, compared norm input)
        fin, dec_xh, dec_rstd = ln(ycur, P["Decoder.Decoder.norm.weight"], P["Decoder.Decoder.norm.bias"])
        cmp("dec_final", 0, fin, "final decoder norm", fwd=True, tol=2e-5)
        final = ws("dec_final")
    logits = lin(final, P["OutputLayer.Linear.weight"], P["OutputLayer.Linear.bias"])
    want = np.concatenate([logits[:, :9], 1 / (1 + np.exp(-logits[:, 9:18])), 0.5 * np.tanh(logits[:, 18:])], 1)
    cmp("hvo", None, want, "output layer + heads", fwd=True)
    if G is None:
        led.assert_closed()
        return n
    # ---------------------------------------------------------------------------------------------- backward
    def wgrad(dy, xin, wname, bname):
        gcmp(wname, rb(dy).T @ rb(xin), "grad " + wname)
        gcmp(bname, rb(dy).sum(0), "grad " + bname)

    def masked(name, gl, site, what):
        """the dropout-masked copy of a gradient (the operand of the Linear's dgrad and weight gradient) against the mask on the gradient"""
        if p > 0:
            cmp(name + "m", gl, lambda dt: tmp(name, gl, d).astype(dt) * np.asarray(mask(site, M * d, (M, d)), dt), what, tol=1e-6,
                stored16=r.bf16_only(name + "m", gl))

    def dlog_ref(dt):
        """d loss / d logits = d loss / d hvo x the heads' derivatives at the device's hvo (heads_bwd_kernel); d loss / d hvo: the probe's,
        or the loss's derivative at the device's hvo, y and the penalty (gt_loss)"""
        led.consume("hvo")
        a = f64(r.hvo.numpy()).reshape(M, 27).astype(dt)
        if led.d_hvo_supplied:
            led.consume("d_hvo")
            g = f64(r.d_hvo.numpy()).reshape(M, 27).astype(dt)
        else:
            assert getattr(r, "d_hvo_from", None) == "loss", "d_hvo is neither the loss's nor the caller's"
            y = f64(r.y.numpy()).reshape(M // 32, 32, 27).astype(dt)
            hvo3 = a.reshape(M // 32, 32, 27)
            _, dpred = ng.calculate_loss((hvo3[..., :9], hvo3[..., 9:18], hvo3[..., 18:]), y, float(np.float32(r.loss_penalty)))
            g = np.concatenate(dpred, -1).reshape(M, 27).astype(dt)
        return np.concatenate([g[:, :9], g[:, 9:18] * a[:, 9:18] * (1 - a[:, 9:18]), g[:, 18:] * (dt(0.5) - 2 * a[:, 18:] * a[:, 18:])], 1)

    cmp("dlogits", 0, dlog_ref, "d loss / d logits (loss derivative x head derivatives)")
    dlog = ws("dlogits")
    wgrad(dlog, final, "OutputLayer.Linear.weight", "OutputLayer.Linear.bias")

    # the output layer's dgrad (bf16 operands: mk_gemm) through the final norm and the top layer's closing norm: one fused row pass (ln_bwd2)
    top = L + Ld - 1
    fin_norm = "Decoder.Decoder.norm" if Ld else "Encoder.Encoder.norm"
    top_norm = ("Decoder.Decoder.layers.%d.norm3" % (Ld - 1)) if Ld else ("Encoder.Encoder.layers.%d.norm2" % (L - 1))

    def top_chain(dt):
        dfin = rb(ws("dlogits")).astype(dt) @ rb(P["OutputLayer.Linear.weight"]).astype(dt)
        xh, rs = (dec_xh, dec_rstd) if Ld else (ws("enc_xhat"), ws("enc_rstd", 0, 1))
        mid, dgo, dbo = ln_bwd(dfin, xh.astype(dt), rs.astype(dt), P[fin_norm + ".weight"].astype(dt))
        return (mid, dgo, dbo) + ln_bwd(mid, ws("xhat2", top).astype(dt), ws("rstd2", top, 1).astype(dt), P[top_norm + ".weight"].astype(dt))

    top_chain = memo(top_chain)
    cmp("dzA", top, lambda dt: top_chain(dt)[3], "output layer dgrad + final norm + top layer's closing norm backward", tol=1e-4)
    gcmp(fin_norm + ".weight", lambda dt: top_chain(dt)[1], "grad " + fin_norm + ".weight (behind the output layer's dgrad)", tol=1e-4)
    gcmp(fin_norm + ".bias", lambda dt: top_chain(dt)[2], "grad " + fin_norm + ".bias (behind the output layer's dgrad)", tol=1e-4)
    gcmp(top_norm + ".weight", lambda dt: top_chain(dt)[4], "grad " + top_norm + ".weight (two-norm row pass)", tol=1e-4)
    gcmp(top_norm + ".bias", lambda dt: top_chain(dt)[5], "grad " + top_norm + ".bias (two-norm row pass)", tol=1e-4)

    def ffn_bwd(pre, gl, xin, dz_name, prev_xh, prev_rstd, prev_norm, dzprev_name):
        masked(dz_name, gl, ng.layer_site(gl, ng.S_DROPF), pre + "dropout mask on the gradient of linear2's output")
        dz, dzm = tmp(dz_name, gl, d), tmp(dz_name + "m", gl, d)
        wgrad(dzm, ws("hact", gl), pre + "linear2.weight", pre + "linear2.bias")
        dh = (rb(dzm) @ rb(P[pre + "linear2.weight"])) * np.where(ws("hact", gl) != 0, scale, 0.0)
        cmp("dhid", gl, dh, pre + "linear2 dgrad (relu / dropout mask)", stored16=r.bf16_only("dhid", gl))
        dhid = tmp("dhid", gl, F)
        wgrad(dhid, xin, pre + "linear1.weight", pre + "linear1.bias")
        enc = P2 and gl < L
        pre_ln = rb(dhid) @ rb(P[pre + "linear1.weight"])
        pre_ln = (hrb(pre_ln) if enc else pre_ln) + dz
        want, dg, db = ln_bwd(pre_ln, ws(prev_xh, gl), ws(prev_rstd, gl, 1), P[pre + prev_norm + ".weight"])
        HB = HIDB if enc else dict(tol=1e-4)
        cmp(dzprev_name, gl, want, pre + "linear1 dgrad + " + prev_norm + " backward", **HB)
        gcmp(pre + prev_norm + ".weight", dg, "grad " + pre + prev_norm + ".weight", **HB)
        gcmp(pre + prev_norm + ".bias", db, "grad " + pre + prev_norm + ".bias", **HB)

    for l in reversed(range(Ld)):
        pre, gl = "Decoder.Decoder.layers.%d." % l, L + l
        ffn_bwd(pre, gl, ws("x2", gl), "dzA", "xhatx", "rstdx", "norm2", "dzB")
        masked("dzB", gl, ng.layer_site(gl, ng.S_DROP2), pre + "dropout2 mask on the gradient")
        wo = P[pre + "multihead_attn.out_proj.weight"]
        wgrad(tmp("dzBm", gl, d), ws("ctxx", gl), pre + "multihead_attn.out_proj.weight", pre + "multihead_attn.out_proj.bias")
        attn_core_bwd(pre, gl, "cross", cross_qkv(gl), "Px", ng.layer_site(gl, ng.S_XATTN), lambda gl=gl: tmp("dzBm", gl, d), wo, "dqkvx", True)
        dqkvx = ws("dqkvx", gl).reshape(-1)
        dqx, dkvx = dqkvx[:M * d].reshape(M, d), dqkvx[M * d:].reshape(M, 2 * d)
        wx = P[pre + "multihead_attn.in_proj_weight"]
        gcmp(pre + "multihead_attn.in_proj_weight", rb(dqx).T @ rb(ws("x1", gl)), "grad " + pre + "cross q in_proj weight", rows=slice(0, d))
        gcmp(pre + "multihead_attn.in_proj_weight", rb(dkvx).T @ rb(ws("memory")), "grad " + pre + "cross kv in_proj weight", rows=slice(d, 3 * d))
        gcmp(pre + "multihead_attn.in_proj_bias", np.concatenate([rb(dqx).sum(0), rb(dkvx).sum(0)]), "grad " + pre + "cross in_proj bias")

        def c_chain(dt, gl=gl, dqx=dqx, wx=wx, pre=pre):     # dz1 = LNbwd_norm1(dqx Wq + dz2)
            pre_ln = rb(dqx).astype(dt) @ rb(wx[:d]).astype(dt) + tmp("dzB", gl, d).astype(dt)
            return ln_bwd(pre_ln, ws("xhat1", gl).astype(dt), ws("rstd1", gl, 1).astype(dt), P[pre + "norm1.weight"].astype(dt))

        c_chain = memo(c_chain)
        cmp("dzC", gl, lambda dt: c_chain(dt)[0], pre + "cross q dgrad + norm1 backward", tol=1e-4)
        gcmp(pre + "norm1.weight", lambda dt: c_chain(dt)[1], "grad " + pre + "norm1.weight", tol=1e-4)
        gcmp(pre + "norm1.bias", lambda dt: c_chain(dt)[2], "grad " + pre + "norm1.bias", tol=1e-4)
        masked("dzC", gl, ng.layer_site(gl, ng.S_DROP1), pre + "dropout1 mask on the gradient")
        wgrad(tmp("dzCm", gl, d), ws("ctx", gl), pre + "self_attn.out_proj.weight", pre + "self_attn.out_proj.bias")
        attn_core_bwd(pre, gl, "masked self", self_qkv(gl), "P", ng.layer_site(gl, ng.S_ATTN), lambda gl=gl: tmp("dzCm", gl, d),
                      P[pre + "self_attn.out_proj.weight"], "dqkv", False)
        wgrad(tmp("dqkv", gl, 3 * d), dec_in[l], pre + "self_attn.in_proj_weight", pre + "self_attn.in_proj_bias")

        def in_chain(dt, gl=gl, pre=pre):                    # the self in-proj dgrad + the residual branch's gradient
            return rb(tmp("dqkv", gl, 3 * d)).astype(dt) @ rb(P[pre + "self_attn.in_proj_weight"]).astype(dt) + tmp("dzC", gl, d).astype(dt)

        if l > 0:
            pp = "Decoder.Decoder.layers.%d." % (l - 1)

            def below(dt, gl=gl, pp=pp, in_chain=in_chain):
                return ln_bwd(in_chain(dt), ws("xhat2", gl - 1).astype(dt), ws("rstd2", gl - 1, 1).astype(dt), P[pp + "norm3.weight"].astype(dt))

            below = memo(below)
            cmp("dzA", gl - 1, lambda dt: below(dt)[0], pre + "self in_proj dgrad + previous layer's norm3 backward", tol=1e-4)
            gcmp(pp + "norm3.weight", lambda dt: below(dt)[1], "grad " + pp + "norm3.weight", tol=1e-4)
            gcmp(pp + "norm3.bias", lambda dt: below(dt)[2], "grad " + pp + "norm3.bias", tol=1e-4)
        else:
            # The decoder input layer's backward.  Its output (da0_dec) has no public name: it is checked through the weight and bias gradients
            # it feeds, the dropout / ReLU mask restated from b0 and da rounded to bf16 where the weight gradient rounds it -- weight and bias
            # gradients: the matmul-like class bar
            def din(dt, in_chain=in_chain):
                da = rb(in_chain(dt) * np.asarray(mask(ng.SITE_PE_DEC, M * d, (M, d)), dt) * (ws("b0") > 0))
                return da.T @ rb(f64(tgt).reshape(M, -1)).astype(dt), da.sum(0)

            din = memo(din)
            gcmp("InputLayerDecoder.Linear.weight", lambda dt: din(dt)[0], "grad InputLayerDecoder.Linear.weight (in_proj dgrad, dropout, relu mask)")
            gcmp("InputLayerDecoder.Linear.bias", lambda dt: din(dt)[1], "grad InputLayerDecoder.Linear.bias (in_proj dgrad, dropout, relu mask)")
    if Ld:
        # encoder half of the encoder-decoder backward: the memory gradient = the sum of the decoder layers' cross-attention k / v
        # dgrads; through the final encoder norm and the top layer's closing norm it becomes that layer's dz (one fused row pass on the device)
        dmem = np.zeros((M, d))
        for l in range(Ld):
            dkvx = ws("dqkvx", L + l).reshape(-1)[M * d:].reshape(M, 2 * d)
            dmem += rb(dkvx) @ rb(P["Decoder.Decoder.layers.%d.multihead_attn.in_proj_weight" % l][d:])
        cmp("dmem", 0, dmem, "memory gradient (sum of the cross-attention k / v dgrads)", tol=1e-4)
        g_top, dg, db = ln_bwd(ws("dmem"), ws("enc_xhat"), ws("enc_rstd", 0, 1), P["Encoder.Encoder.norm.weight"])
        gcmp("Encoder.Encoder.norm.weight", dg, "grad Encoder.Encoder.norm.weight", tol=1e-4)
        gcmp("Encoder.Encoder.norm.bias", db, "grad Encoder.Encoder.norm.bias", tol=1e-4)
        pp = "Encoder.Encoder.layers.%d." % (L - 1)
        want, dg, db = ln_bwd(g_top, ws("xhat2", L - 1), ws("rstd2", L - 1, 1), P[pp + "norm2.weight"])
        cmp("dzA", L - 1, want, "final encoder norm + top layer's norm2 backward", tol=1e-4)
        gcmp(pp + "norm2.weight", dg, "grad " + pp + "norm2.weight (two-norm row pass)", tol=1e-4)
        gcmp(pp + "norm2.bias", db, "grad " + pp + "norm2.bias (two-norm row pass)", tol=1e-4)
    for l in reversed(range(L)):
        pre = "Encoder.Encoder.layers.%d." % l
        ffn_bwd(pre, l, ws("x1", l), "dzA", "xhat1", "rstd1", "norm1", "dzB")
        dz1 = tmp("dzB", l, d)
        if p > 0:
            cmp("dzBm", l, dz1 * mask(ng.layer_site(l, ng.S_DROP1), M * d, (M, d)), pre + "dropout1 mask on the gradient", tol=1e-6,
                stored16=r.bf16_only("dzBm", l))
        dz1m = tmp("dzBm", l, d)
        wgrad(dz1m, ws("ctx", l), pre + "self_attn.out_proj.weight", pre + "self_attn.out_proj.bias")
        attn_core_bwd(pre, l, "self", self_qkv(l), "P", ng.layer_site(l, ng.S_ATTN), lambda l=l: tmp("dzBm", l, d),
                      P[pre + "self_attn.out_proj.weight"], "dqkv", False)
        dqkv = tmp("dqkv", l, 3 * d)
        wgrad(dqkv, enc_in[l], pre + "self_attn.in_proj_weight", pre + "self_attn.in_proj_bias")
        dx = rb(dqkv) @ rb(P[pre + "self_attn.in_proj_weight"])
        dx = (hrb(dx) if (P2 and l > 0) else dx) + dz1
        if l > 0:
            pp = "Encoder.Encoder.layers.%d." % (l - 1)
            want, dg, db = ln_bwd(dx, ws("xhat2", l - 1), ws("rstd2", l - 1, 1), P[pp + "norm2.weight"])
            HB = HIDB if P2 else dict(tol=1e-4)
            cmp("dzA", l - 1, want, pre + "in_proj dgrad + previous layer's norm2 backward", **HB)
            gcmp(pp + "norm2.weight", dg, "grad " + pp + "norm2.weight", **HB)
            gcmp(pp + "norm2.bias", db, "grad " + pp + "norm2.bias", **HB)
        else:
            da = dx * mask(ng.SITE_PE_ENC, M * d, (M, d)) * (ws("a0") > 0)
            cmp("dctx", 0, da, "InputLayer backward (in_proj dgrad, dropout, relu mask)", tol=1e-4)
            wgrad(ws("dctx"), f64(x).reshape(M, -1), "InputLayerEncoder.Linear.weight", "InputLayerEncoder.Linear.bias")
    led.assert_closed()
    return n


def check_bf16_shadows(backend, cfg, B, p):
    """precision = 1 where the Linears run on the big-tile kernel (csrc/groove_hip.hip bf16_shadows): the producers of every GEMM operand
    also write a bf16 copy and the GEMMs stage those (gemm32h_kernel) -- each shadow must be, bit for bit, the RNE rounding of the fp32
    tensor beside it (the value the fp32-source kernel rounds at fragment assembly), for activations, gradients and both weight copies.
    With that the shadow path's results are those of the fp32-source path; check_step_bf16 on the same shape compares them with the oracle."""
    cfg = dict(cfg, dropout=p, precision=1)
    P = ng.init_params(cfg, seed=3, perturb=0.05)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=5)
    lib = harness.emu_lib() if backend == "emu" else harness._lib.get_lib()
    lib.cdll.gt_set_operand_shadows(1)               # (off by default; process-wide switch: restored below)
    try:
        return _check_bf16_shadows(backend, cfg, B, p, P, x, y)
    finally:
        lib.cdll.gt_set_operand_shadows(-1)


def _check_bf16_shadows(backend, cfg, B, p, P, x, y):
    r = Runner(cfg, B, backend, rng=(1234, 99, 7))
    r.set_params(P)
    r.forward(x, train=p > 0)
    _, dpred = r.loss(y, 0.47)
    r.backward(dpred, train=p > 0)
    L, d, F = cfg["num_encoder_layers"], cfg["d_model"], cfg["dim_feedforward"]

    def bf(a):
        return (ng.round_bf16(np.asarray(a, np.float32)).view(np.uint32) >> 16).astype(np.uint16)

    def shadow(name, l):
        o, c = r.lib.ws_find(r.c, name + "16", l)
        return r.ws.numpy()[o:o + c].view(np.uint16)

    n = 0
    want = bf(r.ws_get("x0", 0))                          # the input layer's output (operand of layer 0's in-proj and of its weight gradient)
    got = shadow("x0", 0)[:want.size]
    assert np.array_equal(got, want), ("x0", int((got != want).sum()), want.size)
    n += 1
    for l in range(L):
        for name in ["ctx", "x1", "hact"] + (["xout"] if l + 1 < L else []) + ["dhid", "dqkv", "dzAm" if p > 0 else "dzA", "dzBm" if p > 0 else "dzB"]:
            want = bf(r.ws_get(name, l))
            got = shadow(name, l)[:want.size]
            assert np.array_equal(got, want), (name, l, int((got != want).sum()), want.size)
            n += 1
        pre = "Encoder.Encoder.layers.%d." % l
        o, c = r.lib.ws_find(r.c, "w16", l)
        w16 = r.ws.numpy()[o:o + c].view(np.uint16)
        o, c = r.lib.ws_find(r.c, "w16t", l)
        w16t = r.ws.numpy()[o:o + c].view(np.uint16)
        at = 0
        for wn in ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "linear1.weight", "linear2.weight"):
            W = np.asarray(P[pre + wn], np.float32)
            assert np.array_equal(w16[at:at + W.size], bf(W).reshape(-1)), (wn, l)
            assert np.array_equal(w16t[at:at + W.size], bf(W.T.copy()).reshape(-1)), (wn, l, "transposed")
            at += W.size
            n += 2
    return n


def check_step_bf16(backend, cfg, B, p=0.0, penalty=0.47, seed=3, precision=1, flags=0, regime=None):
    """precision = 2: the same two bars; the end-to-end sanity bound is taken against the bf16-OPERAND oracle with a wider factor (the
    storage roundings of precision 2 are additional noise of the same size: 2.5 x the bf16 effect).
    regime: a name of tests/regimes.py -- the parameters moved away from initialisation, the regime's condition asserted on the fp64
    (bf16-operand) oracle's cache.  The per-operation walk keeps its fixed class bars (_close's np.float32 rule included) and is the
    assertion.  Three end-to-end assertions are not made, in two regimes (reasons below): the max-abs bound in saturated, and both the
    max-abs and the rms bound in shift with precision 2 in force."""
    cfg = dict(cfg, dropout=p, precision=precision)
    cfg0 = dict(cfg, precision=0)
    P = regimes.apply(ng.init_params(cfg, seed=seed, perturb=0.05), cfg, regime, seed)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=seed + 2)
    Ld = cfg.get("num_decoder_layers", 0)
    tgt = shift_right(y) if Ld else None
    rng = (1234, 99, 7)
    (h, v, o), C = ng.forward(P, cfg, x, tgt=tgt, rng=rng if p > 0 else None, dtype=np.float64)
    FIGURES.clear()
    BF16_FIGURES.clear()
    if regime is not None:
        FIGURES["regime"] = regimes.assert_condition(regime, C, h)
    r = Runner(cfg, B, backend, rng=rng, flags=flags)
    r.set_params(P)
    hvo = r.forward(x, tgt, train=p > 0)
    # (2) end to end, sanity bound
    (h0, v0, o0), _ = ng.forward(P, cfg0, x, tgt=tgt, rng=rng if p > 0 else None, dtype=np.float64)
    ref, ref0 = np.concatenate([h, v, o], -1), np.concatenate([h0, v0, o0], -1)
    eq = _rms(ref0 - ref)
    assert eq > 1e-5, "the bf16 rounding has no visible effect on this case: pick another"
    frac = BF16_E2E_FRAC if r.precision_in_force() < 2 else 2.5
    FIGURES["bf16_out_max"] = float(np.abs(hvo - ref).max() / BF16_OUT_MAX)
    FIGURES["bf16_e2e"] = _rms(hvo - ref) / (frac * eq + 1e-5)
    # Two regimes take a forward bound away, because E_q -- the distance between the two ORACLES -- no longer measures what separates the device
    # from them; the bound relative to the loss and the walk, which is the assertion, stay.
    # saturated: the absolute 5e-2 was sized for hit logits within +-1.7.  With the output layer's weights x 30 they reach +-23 ... +-91, and ONE
    # operand element that rounds to the neighbouring bf16 on the device -- the decorrelation described above -- moves such a logit by 3e-2
    # (emulator, d_model 32: 0.63 of the bound from a single flip).  The bound relative to E_q, which scales with the logits, stays.
    # shift with precision 2 in force: k carries a bias of N(0, 40), and STORING it in bf16 moves each element by up to 2^-9 of that -- score noise
    # the operand-rounding oracle E_q is measured on does not have (its k is rounded inside the in-proj only, before the bias is added): the
    # device sits 3.7 x E_q (emulator, d_model 256) and 0.078 max-abs (MI355X, d_model 512) from that oracle.  The walk restates the softmax
    # over the STORED q / k.
    stored_k = regime == "shift" and r.precision_in_force() == 2
    if regime != "saturated" and not stored_k:
        assert np.abs(hvo - ref).max() < BF16_OUT_MAX, "forward max-abs %g" % np.abs(hvo - ref).max()
    if not stored_k:
        assert _rms(hvo - ref) <= frac * eq + 1e-5, "forward rms %g vs bf16 effect %g" % (_rms(hvo - ref), eq)
    stats, d_hvo = r.loss(y, penalty)
    rstats, _ = ng.calculate_loss((h, v, o), y.astype(np.float64), penalty)
    assert abs(stats[0] - rstats[0]) < 1e-2 * max(1.0, abs(rstats[0]))
    G = r.backward(train=p > 0)
    # (1) per operation, teacher-forced: the parity proof
    nops = check_ops_bf16(r, P, cfg, x, tgt, rng, p, G)
    assert nops >= 10 * (cfg["num_encoder_layers"] + Ld)
    return r, P, G


def check_autocast_anchor(backend, cfg, B, seed=3):
    """precision = 2 against the third-party definition it is anchored on: the eval forward of the stock torch modules under
    torch.autocast(bfloat16) (oracle.torch_groove.forward_autocast).  Two realisations of "bf16 where the bytes are" cannot agree element
    for element (autocast also runs the attention products in bf16 and rounds more tensors); the device must sit within the bf16 effect
    itself: RMS(device - autocast) and RMS(device - fp32) <= 1.5 x RMS(fp32 - autocast)."""
    from oracle import torch_groove as tg
    cfg = dict(cfg, dropout=0.0, precision=2)
    P = ng.init_params(cfg, seed=seed, perturb=0.05)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=seed + 2)
    r = Runner(cfg, B, backend)
    assert r.precision_in_force() == 2, "precision 2 is not in force for this shape"
    r.set_params(P)
    hvo = r.forward(x, None, train=False)
    ac, ref = tg.forward_autocast(P, cfg, x)
    eq = _rms(ref - ac)
    assert eq > 1e-5
    assert _rms(hvo - ac) <= 1.5 * eq + 1e-5 and _rms(hvo - ref) <= 1.5 * eq + 1e-5, (_rms(hvo - ac), _rms(hvo - ref), eq)
    assert np.abs(hvo - ac).max() < BF16_OUT_MAX
    return _rms(hvo - ac), _rms(hvo - ref), eq


def check_train_step_bf16(backend, cfg, B, p, precision=1, flags=0):
    """gt_train_step with precision = 1 (fp32 master weights): after each of two SGD steps the per-operation checks hold on the
    step's own saved state, the update is exactly  w -= lr * g  of the device's gradients ... observed through the parameters:
    they move along the bf16-operand oracle's gradient within the end-to-end bound."""
    cfg = dict(cfg, dropout=p, precision=precision)
    P = ng.init_params(cfg, seed=9, perturb=0.05)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=4)
    tgt = shift_right(y) if cfg.get("num_decoder_layers", 0) else None
    r = Runner(cfg, B, backend, rng=(77, 5, 0), lr=0.05, flags=flags)
    r.set_params(P)
    cur = {k: v.astype(np.float64) for k, v in P.items()}
    for step in range(2):
        before = r.unflatten(r.params.numpy())
        stats = r.train_step(x, y, 0.38, algo=0)
        (h, v, o), C = ng.forward(before, cfg, x, tgt=tgt, rng=(77, 5, step) if p > 0 else None, dtype=np.float64)
        rstats, dpred = ng.calculate_loss((h, v, o), y.astype(np.float64), 0.38)
        assert abs(stats[0] - rstats[0]) < 1e-2 * max(1, abs(rstats[0])), (step, stats[0], rstats[0])
        check_ops_bf16(r, before, cfg, x, tgt, (77, 5, step), p)                    # forward state of THIS step
        G = ng.backward(before, cfg, C, dpred, dtype=np.float64)
        got = r.unflatten(r.params.numpy())
        for k in G:
            upd = (before[k].astype(np.float64) - got[k]) / 0.05                  # the gradient the device applied
            assert np.abs(upd - G[k]).max() <= 5e-2 * max(np.abs(G[k]).max(), 1e-4) + 1e-5, (step, k)
    assert r.step_state().step == 2


def check_optimizers(backend, cfg, B):
    cfg = dict(cfg, dropout=0.0)
    r, P, G, Gr = check_step(backend, cfg, B, check_ws=False)
    Gf = {k: G[k].astype(np.float32) for k in G}
    new = r.optimizer_step(0)
    want = ng.sgd_step(P, Gf, 0.094)
    for k in P:
        assert np.abs(new[k] - want[k]).max() < 1e-6, k
    assert r.step_state().step == 8
    # adam from the SGD-updated point with the same grads, two steps (bias correction uses step+1 relative to start)
    r2 = Runner(cfg, B, backend, rng=(1, 2, 0), lr=1e-3)
    r2.set_params(P)
    r2.grads = r2.Buf(r2.flatten(Gf))
    m = {k: np.zeros_like(P[k]) for k in P}
    v = {k: np.zeros_like(P[k]) for k in P}
    cur = P
    for t in (1, 2):
        got = r2.optimizer_step(1)
        cur, m, v = ng.adam_step(cur, Gf, m, v, t, 1e-3)
        for k in P:
            assert np.abs(got[k] - cur[k]).max() < 2e-6, (t, k)


def expected_packs(Pd, cfg):
    """Fragment-ordered weight copies of the sequence-resident kernels (csrc/gt_seq.h, seq_pack_kernel) from a name -> array dict:
    per layer [in_w | out_w | w1 | w2]; pack[((t * nkt + u) * 64 + lane) * 4 + j] = B(16 u + 4 lg + j, 16 t + l16), lane = l16 + 16 lg;
    forward copy: B(k, n) = W[n][k], dgrad copy: B(k, n) = W[k][n]."""
    pf, pb = [], []
    for l in range(cfg["num_encoder_layers"]):
        pre = "Encoder.Encoder.layers.%d." % l
        for name in ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "linear1.weight", "linear2.weight"):
            W = np.asarray(Pd[pre + name], np.float32)
            R, C = W.shape
            pf.append(W.reshape(R // 16, 16, C // 16, 4, 4).transpose(0, 2, 3, 1, 4).reshape(-1))      # (t, l16, u, lg, j) -> (t, u, lg, l16, j)
            pb.append(W.reshape(R // 16, 4, 4, C // 16, 16).transpose(3, 0, 1, 4, 2).reshape(-1))      # (u, lg, j, t, l16) -> (t, u, lg, l16, j)
    return np.concatenate(pf), np.concatenate(pb)


def check_update(before, after, G, lr, adam=None, tag=None):
    """One optimizer step of the device against the fp64 update of the oracle's gradients G, teacher-forced: the reference starts from the
    device's own parameters `before` (and, for Adam, its own moments), so nothing of earlier steps propagates and the bar can be per element.
    before / after / G: name -> array.  adam: None (SGD) or dict(m0, v0, m1, v1, t) -- the device's moments before / after the step and the
    step number t the bias correction uses (beta1 0.9, beta2 0.999, eps 1e-8: the Runner's step state).
    SGD: |dp_dev - dp_ref| <= GRAD_TOL * max(max |dp_ref|, lr 1e-5) + ulp_fp32(p_after), dp_ref = -lr G: the gradient bar of check_step
    carried through the update, plus the fp32 rounding of p - lr g (it matters for LayerNorm gains near 1).
    Adam: the moments within GRAD_TOL (m) / 2 GRAD_TOL (v) of the tensor's largest, the parameters within the live / strong bars of
    check_train_step.  Raises AssertionError naming the step, the tensor and the element; returns the largest error / bar ratio."""
    lr = float(np.float32(lr))
    f64 = lambda a: np.asarray(a, np.float64)
    ratio = 0.0
    for k in G:
        p0, p1, g = f64(before[k]), f64(after[k]), f64(G[k])

        def worst(err, bar, what):
            nonlocal ratio
            ratio = max(ratio, float((err / bar).max(initial=0.0)))
            excess = err - bar
            if excess.max(initial=-1.0) > 0:
                i = np.unravel_index(int(np.argmax(excess)), err.shape)
                raise AssertionError("step %s %s%s element %s: |err| %.3g > bar %.3g (%d elements over)"
                                     % (tag, k, what, tuple(int(j) for j in i), err[i], bar[i] if np.ndim(bar) else bar, int((excess > 0).sum())))

        if adam is None:
            d_ref = -lr * g
            ulp = np.spacing(np.abs(np.asarray(after[k], np.float32))).astype(np.float64)
            worst(np.abs((p1 - p0) - d_ref), GRAD_TOL * max(float(np.abs(d_ref).max()), lr * 1e-5) + ulp, "")
            continue
        b1, b2, eps, t = 0.9, 0.999, 1e-8, adam["t"]
        m_ref = b1 * f64(adam["m0"][k]) + (1 - b1) * g
        v_ref = b2 * f64(adam["v0"][k]) + (1 - b2) * g * g
        # (floors: the moments of a gradient of 1e-5, check_step's floor for a numerically zero gradient tensor)
        worst(np.abs(f64(adam["m1"][k]) - m_ref), GRAD_TOL * max(float(np.abs(m_ref).max()), (1 - b1) * 1e-5), " (first moment)")
        worst(np.abs(f64(adam["v1"][k]) - v_ref), 2 * GRAD_TOL * max(float(np.abs(v_ref).max()), (1 - b2) * 1e-10), " (second moment)")
        p_ref = p0 - (lr / (1 - b1 ** t)) * m_ref / (np.sqrt(v_ref) / np.sqrt(1 - b2 ** t) + eps)
        scale = max(1.0, float(np.abs(p_ref).max()))
        err = np.abs(p1 - p_ref)
        live = np.abs(g) > 1e-6
        worst(np.where(live, err, 0.0), 1e-3 * scale, " (live elements)")
        strong = np.abs(g) > 0.1 * np.abs(g).max()
        worst(np.where(strong, err, 0.0), 1e-4 * scale, " (well-conditioned elements)")
    return ratio


def kink_bound(r, cfg):
    """How many ReLU decisions adopt_device_kinks may take from the device: about one per 1e6 pre-activations, at least 4."""
    return 4 + r.M * cfg["dim_feedforward"] * (cfg["num_encoder_layers"] + cfg.get("num_decoder_layers", 0)) // 100000


def check_decisions_current(r, C):
    """The workspace tensors adopt_device_kinks reads (every layer's hact, the input layer's pre-activation a0) hold the values of the
    forward that cache C describes -- after gt_train_step too, on whatever path ran it: a stale or never-written tensor would feed the
    adoption decisions of another step."""
    n_enc = len(C["enc"])
    todo = [("hact", l, c["hact"]) for l, c in enumerate(C["enc"])] + [("hact", n_enc + l, c["hact"]) for l, c in enumerate(C["dec"])]
    todo.append(("a0", 0, C["in_enc"]["a"]))
    for name, l, ref in todo:
        tol = 2.0 ** -8 if r.bf16_only(name, l) else 1e-4
        err = rel_err(r.ws_get(name, l).reshape(-1), np.asarray(ref).reshape(-1))
        assert err < tol, "%s of layer %d is not this step's: rel err %g" % (name, l, err)
    return len(todo)


def check_train_step(backend, cfg, B, p, algo=0, seq=True, flags=0, regime=None, lr=0.05, steps=3):
    """gt_train_step == forward+loss+backward+update with the oracle's masks, three steps; later steps use step+1.  Each step is checked
    twice: teacher-forced (the fp64 oracle's step from the device's own parameters and moments before it, per element: check_update) and
    along the free-running fp64 trajectory from the initial parameters.  Both oracle caches adopt the device's ReLU decisions at the kink.
    regime: the initial parameters moved by tests/regimes.py, the regime's condition asserted on the first step's oracle cache."""
    cfg = dict(cfg, dropout=p)
    P = regimes.apply(ng.init_params(cfg, seed=9, perturb=0.05), cfg, regime, 9)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=4)
    Ld = cfg.get("num_decoder_layers", 0)
    tgt = shift_right(y) if Ld else None
    r = Runner(cfg, B, backend, rng=(77, 5, 0), lr=lr, seq=seq, flags=flags)
    r.set_params(P)
    cur = {k: v.astype(np.float64) for k, v in P.items()}
    folded = r.lib.cdll.gt_step_launches(ctypes.byref(r.c)) > 0     # sequence-resident path: the update writes the next step's weight packs
    bound = kink_bound(r, cfg)
    f64 = lambda D: {k: np.asarray(v, np.float64) for k, v in D.items()}
    FIGURES.clear()
    for step in range(steps):
        before = r.unflatten(r.params.numpy())
        if algo == 1:
            m0, v0 = ((r.unflatten(r.m.numpy()), r.unflatten(r.v.numpy())) if hasattr(r, "m")
                      else ({k: np.zeros_like(a) for k, a in before.items()},) * 2)
        # from the second step on: GT_STEP_PACKS_CURRENT (4) -- the previous step's update left this step's fragment-ordered weights
        stats = r.train_step(x, y, 0.38, algo=algo, skip_update=4 if (folded and step > 0) else 0)
        rng = (77, 5, step) if p > 0 else None
        got = r.unflatten(r.params.numpy())
        # teacher-forced: the oracle's step from where the device started it
        (h, v, o), Ct = ng.forward(f64(before), cfg, x, tgt=tgt, rng=rng, dtype=np.float64)
        tstats, dpt = ng.calculate_loss((h, v, o), y.astype(np.float64), 0.38)
        if regime is not None and step == 0:
            FIGURES["regime"] = regimes.assert_condition(regime, Ct, h)
        assert abs(stats[0] - tstats[0]) < 2e-5 * max(1, abs(tstats[0])), (step, "teacher-forced loss", stats[0], tstats[0])
        assert check_decisions_current(r, Ct) >= len(Ct["enc"]) + 1
        adopted = adopt_device_kinks(r, Ct, cfg)
        assert adopted <= bound, (step, adopted)
        Gt = ng.backward(f64(before), cfg, Ct, dpt, dtype=np.float64)
        adam = None
        if algo == 1:
            adam = dict(m0=m0, v0=v0, m1=r.unflatten(r.m.numpy()), v1=r.unflatten(r.v.numpy()), t=step + 1)
        FIGURES["update"] = max(FIGURES.get("update", 0.0), check_update(before, got, Gt, lr, adam=adam, tag=step))
        # free-running fp64 trajectory
        (h, v, o), C = ng.forward(cur, cfg, x, tgt=tgt, rng=rng, dtype=np.float64)
        rstats, dpred = ng.calculate_loss((h, v, o), y.astype(np.float64), 0.38)
        assert abs(stats[0] - rstats[0]) < 2e-5 * max(1, abs(rstats[0])), (step, stats[0], rstats[0])
        adopted = adopt_device_kinks(r, C, cfg)
        assert adopted <= bound, (step, adopted)
        G = ng.backward(cur, cfg, C, dpred, dtype=np.float64)
        if algo == 0:
            cur = {k: cur[k] - lr * G[k] for k in cur}
        else:
            if step == 0:
                am, av = {k: np.zeros_like(v) for k, v in cur.items()}, {k: np.zeros_like(v) for k, v in cur.items()}
            cur, am, av = ng.adam_step(cur, G, am, av, step + 1, lr)
        for k in cur:
            # (adam: an element whose gradient is numerically zero moves by lr * g / (|g| + eps) -- its sign is noise; skip those)
            live = np.abs(G[k]) > 1e-6 if algo == 1 else np.ones(G[k].shape, bool)
            assert np.abs(got[k] - cur[k])[live].max(initial=0) < (1e-3 if algo == 1 else 2e-5) * max(1.0, np.abs(cur[k]).max()), (step, k)
            if algo == 1:
                # Adam divides by sqrt(v): an element's error is the gradient's error (bar 2e-4 of the tensor's largest entry) over |g|.
                # Where the gradient is well conditioned -- within a factor 10 of the largest -- the update keeps a tight bar
                strong = np.abs(G[k]) > 0.1 * np.abs(G[k]).max()
                assert np.abs(got[k] - cur[k])[strong].max(initial=0) < 1e-4 * max(1.0, np.abs(cur[k]).max()), (step, k, "well-conditioned elements")
        if folded and cfg["d_model"] % 16 == 0:
            # the folded update + pack kernel wrote the NEXT step's fragment-ordered weights: bitwise what packing the updated parameters gives
            ef, eb = expected_packs(got, cfg)
            for name, want in (("pack_f", ef), ("pack_b", eb)):
                o, c = r.lib.ws_find(r.c, name)
                assert c == want.size, (name, c, want.size)
                assert np.array_equal(r.ws.numpy()[o:o + c].view(np.uint32), want.view(np.uint32)), (step, name)
    assert r.step_state().step == steps
    try:                                             # QUAD forward: no pair exchange timed out (error word of the region's header)
        o, _ = r.lib.ws_find(r.c, "seq_xchg")
        assert r.ws.numpy()[o:o + 1].view(np.uint32)[0] == 0
    except Exception as e:
        assert "seq_xchg" in str(e) or "absent" in str(e) or "unknown" in str(e), e


def check_predict(backend, cfg, B, use_thres=True, thres=0.5, out_tol=OUT_TOL, margin_tol=1e-4, pd_seed=None, regime=None, seed=21):
    """out_tol / margin_tol: the fp32 bars by default; the bf16 operand path passes its own (hits compared where the decision
    margin exceeds what a bf16 rounding flip can move a probability by).
    regime: the parameters (of seed `seed`) moved by tests/regimes.py; the regime's condition is asserted on the oracle's cache of the
    decoded sequence, and the encoder-decoder comparison must reach 90 % of all decode steps."""
    cfg = dict(cfg, dropout=0.3)      # predict is eval mode: dropout must be ignored
    P = regimes.apply(ng.init_params(cfg, seed=seed, perturb=0.05), cfg, regime, seed)
    x, _ = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=8)
    r = Runner(cfg, B, backend)
    r.set_params(P)
    hvo = r.predict(x, thres=thres, use_thres=use_thres, pd_seed=pd_seed)         # pd_seed: the reference's use_pd (sampled hits)
    (h, v, o), margin = ng.predict(P, cfg, x, use_thres=use_thres, thres=thres, dtype=np.float64, pd_seed=pd_seed)
    if regime is not None:            # (greedy decoding is causal: the teacher-forced forward over the decoded sequence is its last step's)
        tgt = shift_right(np.concatenate([h, v, o], -1)) if cfg.get("num_decoder_layers", 0) else None
        (hl, _, _), C = ng.forward(P, dict(cfg, dropout=0.0), x, tgt=tgt, dtype=np.float64)
        FIGURES.clear()
        FIGURES["regime"] = regimes.assert_condition(regime, C, hl)
    if pd_seed is not None:
        frac = float(hvo[..., :9].mean())
        assert 0.02 < frac < 0.98, frac                                            # really sampled: neither all hits nor none
    if use_thres or pd_seed is not None:
        sure = margin > margin_tol
        if cfg.get("num_decoder_layers", 0):
            # greedy decoding: a flipped low-margin hit changes every LATER step of that sequence, so each sequence is
            # compared up to (not including) its first step with a decision inside the margin -- bit-exact hits, v / o
            # within tolerance; sequences that are sure everywhere are compared whole
            vo = np.concatenate([v, o], -1)
            compared = 0
            for b in range(B):
                unsure = np.flatnonzero(~sure[b].reshape(32, -1).all(1))
                t_end = int(unsure[0]) if len(unsure) else 32
                compared += t_end
                assert np.array_equal(hvo[b, :t_end, :9], h[b, :t_end]), (b, t_end)
                if t_end:
                    assert np.abs(hvo[b, :t_end, 9:] - vo[b, :t_end]).max() < out_tol, (b, t_end)
            assert compared > 0, "no comparable decode step: every sequence has a low-margin decision at step 0"
            if regime is not None:
                FIGURES["decode_steps"] = compared / (32.0 * B)
                assert compared >= 0.9 * 32 * B, "only %d of %d decode steps lie before a low-margin decision" % (compared, 32 * B)
            return
        assert np.array_equal(hvo[..., :9][sure], h[sure])                      # bit-exact hit mask
        assert set(np.unique(hvo[..., :9])) <= {0.0, 1.0}
    else:
        assert np.abs(hvo[..., :9] - h).max() < out_tol
    assert np.abs(hvo[..., 9:] - np.concatenate([v, o], -1)).max() < out_tol


def predict_inputs(cfg, B, seed=21):
    """check_predict's fixed inputs for one shape: (cfg with dropout 0.3 -- predict is eval mode: it must be ignored --, parameters, x)"""
    cfg = dict(cfg, dropout=0.3)
    return cfg, ng.init_params(cfg, seed=seed, perturb=0.05), ng.synthetic_batch(B, cfg["embedding_size_src"], seed=8)[0]


# the largest share of hit decisions a check_predict_forced case may leave uncompared (inside the margin), per precision: a condition on the
# case's inputs, not a tolerance.  fp32: the fp64 oracle's own share below 1e-4 is 9.1e-4 at d_model 32 and 0 at 64 (73 728 decisions each);
# bf16 operands: its share below 1e-3 is 9.5e-3, about 5 % below the 5e-3 margin
MAX_LEFT_OUT = {0: 0.01, 1: 0.10}


def check_predict_forced(P, cfg, x, hvo, use_thres=True, thres=None, pd_seed=None, first_seq=0, temperature=1.0, prob=None,
                         out_tol=OUT_TOL, margin_tol=1e-4, max_left_out=None):
    """A finished predict -- hvo (N, 32, 27) from Runner.predict, gt_predict_voices (uncapped, unmasked) or StepEngine.predict over the set x
    -- against ONE eval forward of the fp64 oracle, teacher-forced as check_update is: greedy decoding is causal (step t sees target rows
    0..t only), so the oracle's forward with tgt = shift_right(hvo) restates every decode step from the device's OWN earlier decisions.
    Nothing propagates; all 32 N rows are compared, where check_predict stops a sequence at its first decision inside the margin.
      v, o:  |hvo[..., 9:] - ref| < out_tol on every row.
      use_thres False (and no pd_seed):  |hvo[..., :9] - sigmoid(h_ref)| < out_tol on every row.
      thresholded / sampled:  hits in {0, 1}, equal to sigmoid(h_ref / temperature) > cut wherever that probability is more than margin_tol
        from cut; cut = thres (a number or one per voice; None: 0.5), or with pd_seed ng.pd_uniforms at the element's index in the whole set
        (first_seq: the index of x[0] in it); pd_seed and a thres (gt_predict_voices' sampled mode): a hit needs p above both, the margin is
        the smaller one.  The hit fraction lies in (0.02, 0.98), and at most max_left_out (MAX_LEFT_OUT of cfg's precision) of the decisions
        lie inside the margin.
      prob: the call's prob_out (N, 32, 9), held to sigmoid(h_ref / temperature) within out_tol on every row.
    Encoder-only models: the same comparisons against the plain forward.  Records FIGURES "out" (worst error / out_tol) and "left_out" (the
    share of decisions inside the margin); returns the oracle's (h, v, o)."""
    cfg = dict(cfg)
    N = x.shape[0]
    hvo = np.asarray(hvo, np.float64).reshape(N, 32, 27)
    if max_left_out is None:
        max_left_out = MAX_LEFT_OUT[1 if cfg.get("precision", 0) else 0]
    tgt = shift_right(hvo) if cfg.get("num_decoder_layers", 0) else None
    (h, v, o), _ = ng.forward(P, cfg, x, tgt=tgt, dtype=np.float64)                  # (rng None: eval mode whatever cfg's dropout)
    FIGURES.clear()
    vo_err = np.abs(hvo[..., 9:] - np.concatenate([v, o], -1))
    FIGURES["out"] = float(vo_err.max() / out_tol)
    p_ref = 1.0 / (1.0 + np.exp(-h / float(temperature)))
    if prob is not None:
        perr = np.abs(np.asarray(prob, np.float64).reshape(N, 32, 9) - p_ref)
        FIGURES["out"] = max(FIGURES["out"], float(perr.max() / out_tol))
    decided = use_thres or pd_seed is not None
    if not decided:
        herr = np.abs(hvo[..., :9] - p_ref)
        FIGURES["out"] = max(FIGURES["out"], float(herr.max() / out_tol))
        FIGURES["left_out"] = 0.0
    else:
        cuts = []
        if pd_seed is not None:
            cuts.append(ng.pd_uniforms(pd_seed, first_seq + N)[first_seq:])
        if thres is not None or pd_seed is None:
            cuts.append(np.broadcast_to(np.asarray(0.5 if thres is None else thres, np.float64), (N, 32, 9)))
        want = np.ones((N, 32, 9), bool)
        margin = np.full((N, 32, 9), np.inf)
        for cut in cuts:
            want &= p_ref > cut
            margin = np.minimum(margin, np.abs(p_ref - cut))
        sure = margin > margin_tol
        FIGURES["left_out"] = float((~sure).mean())
    # ---- the assertions, after every figure is on record
    if not vo_err.max() < out_tol:
        i = tuple(int(j) for j in np.unravel_index(int(np.argmax(vo_err)), vo_err.shape))
        raise AssertionError("v / o: sequence %d step %d column %d: max-abs %.3g (bar %g), %d elements over" % (i[0], i[1], 9 + i[2], vo_err.max(), out_tol, int((vo_err >= out_tol).sum())))
    if prob is not None:
        assert perr.max() < out_tol, "prob_out max-abs %g (bar %g)" % (perr.max(), out_tol)
    if not decided:
        assert herr.max() < out_tol, "hit probabilities max-abs %g (bar %g)" % (herr.max(), out_tol)
        return h, v, o
    hits = hvo[..., :9]
    assert set(np.unique(hits)) <= {0.0, 1.0}, np.unique(hits)[:8]
    wrong = sure & ((hits != 0) != want)
    if wrong.any():
        i = tuple(int(j) for j in np.argwhere(wrong)[0])
        raise AssertionError("%d hits differ outside the margin, first at sequence %d step %d voice %d: device %g, oracle p %.9g, margin %.3g"
                             % (int(wrong.sum()), i[0], i[1], i[2], hits[i], p_ref[i], margin[i]))
    frac = float(hits.mean())
    assert 0.02 < frac < 0.98, "hit fraction %g: the case decides nothing" % frac
    assert FIGURES["left_out"] <= max_left_out, "%.3g of the decisions lie inside the margin %g (cap %g): pick other inputs" % (FIGURES["left_out"], margin_tol, max_left_out)
    return h, v, o


def check_golden(backend, path):
    """HIP/emulated path against the committed torch-generated vectors."""
    z = np.load(path)
    cfg = {k: (float(v) if k == "dropout" else int(v)) for k, v in zip(z["cfg_keys"], z["cfg_vals"])}
    P = ng.init_params(cfg, seed=int(z["seed"]), perturb=0.05)
    x, y = z["x"], z["y"]
    B = x.shape[0]
    tgt = shift_right(y) if cfg["num_decoder_layers"] else None
    r = Runner(cfg, B, backend, lr=0.094)
    r.set_params(P)
    hvo = r.forward(x, tgt)
    assert np.abs(hvo - np.concatenate([z["h"], z["v"], z["o"]], -1)).max() < OUT_TOL
    for pen in (1.0, 0.0, 0.47):
        stats, _ = r.loss(y, pen)
        ref = z["stats_pen%g" % pen]
        for i in (0, 1, 3, 4, 5):
            assert abs(stats[i] - ref[i]) < 2e-5 * max(1.0, abs(ref[i])), (pen, i)
        assert abs(np.exp(stats[3]) - ref[2]) < 1e-4 * ref[2]                   # perplexity = exp(bce)
    G = r.backward()
    for k in G:
        if "grad/" + k in z.files:
            assert rel_err(G[k], z["grad/" + k]) < GRAD_TOL, k
        else:
            idx, val = z["gidx/" + k], z["gval/" + k]
            assert np.abs(G[k].reshape(-1)[idx] - val).max() <= GRAD_TOL * np.abs(val).max() + 1e-7, k
            assert abs(np.sqrt((G[k].astype(np.float64) ** 2).sum()) - float(z["gnorm/" + k])) < 1e-4 * float(z["gnorm/" + k])
    if "sgd/OutputLayer.Linear.bias" in z.files:
        new = r.optimizer_step(0)
        for k in new:
            assert np.abs(new[k] - z["sgd/" + k]).max() < 1e-5, k


def check_golden_bf16(backend, path):
    """The committed stock-torch vectors (full-depth C4 / C5 models) on the bf16-operand path (precision = 1): the per-operation
    teacher-forced check -- the parity proof of this mode -- on the golden's own parameters and inputs, and the torch fp32 outputs /
    loss as the end-to-end sanity bound (what separates the two is the bf16 rounding of the operands, nothing else)."""
    z = np.load(path)
    cfg = {k: (float(v) if k == "dropout" else int(v)) for k, v in zip(z["cfg_keys"], z["cfg_vals"])}
    cfg = dict(cfg, precision=1)
    P = ng.init_params(cfg, seed=int(z["seed"]), perturb=0.05)
    x, y = z["x"], z["y"]
    tgt = shift_right(y) if cfg["num_decoder_layers"] else None
    r = Runner(cfg, x.shape[0], backend, lr=0.094)
    r.set_params(P)
    hvo = r.forward(x, tgt)
    assert np.abs(hvo - np.concatenate([z["h"], z["v"], z["o"]], -1)).max() < BF16_OUT_MAX
    stats, _ = r.loss(y, 0.47)
    assert abs(stats[0] - z["stats_pen0.47"][0]) < 1e-2 * max(1.0, abs(z["stats_pen0.47"][0]))
    G = r.backward()
    nops = check_ops_bf16(r, P, cfg, x, tgt, (1234, 99, 0), 0.0, G)
    assert nops >= 10 * (cfg["num_encoder_layers"] + cfg["num_decoder_layers"])


def check_demo_ckpt(backend):
    z = np.load(os.path.join(GOLD, "demo_ckpt.npz"))
    P = {k[3:]: z[k] for k in z.files if k.startswith("sd/") and not k.endswith(".pe")}
    for H in (4, 16):
        cfg = dict(d_model=32, n_heads=H, dim_feedforward=16, num_encoder_layers=6, num_decoder_layers=0, embedding_size_src=16)
        r = Runner(cfg, 4, backend)
        r.set_params(P)
        hvo = r.forward(z["x"])
        ref = np.concatenate([z["h_H%d" % H], z["v_H%d" % H], z["o_H%d" % H]], -1)
        assert np.abs(hvo - ref).max() < OUT_TOL


def golden_files():
    return sorted(glob.glob(os.path.join(GOLD, "g2_*.npz")))


def check_bucketed_backward(backend, cfg, B, p, n_buckets, exact, seq=True):
    """gt_train_step(skip_update=2) must leave bucket 0 of gt_grad_buckets FINAL (that is what the data-parallel path
    all-reduces while skip_update=3 runs), and 2 followed by 3 must equal the one-call backward (skip_update=1)."""
    cfg = dict(cfg, dropout=p)
    P = ng.init_params(cfg, seed=11, perturb=0.05)
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=12)
    whole = Runner(cfg, B, backend, rng=(5, 6, 0), seq=seq)
    whole.set_params(P)
    whole.train_step(x, y, 0.47, skip_update=1)
    gw = whole.grads.numpy().copy()
    r = Runner(cfg, B, backend, rng=(5, 6, 0), seq=seq)
    r.set_params(P)
    buckets = r.lib.grad_buckets(r.c)
    assert len(buckets) == n_buckets
    assert sum(c for _, c in buckets) == r.total and min(o for o, _ in buckets) == 0
    r.train_step(x, y, 0.47, skip_update=2)
    g2 = r.grads.numpy().copy()
    r.train_step(x, y, 0.47, skip_update=3)
    g3 = r.grads.numpy().copy()
    tol = 0.0 if exact else 2e-6 * np.abs(gw).max()
    o0, c0 = buckets[0]
    assert np.abs(g2[o0:o0 + c0] - gw[o0:o0 + c0]).max() <= tol, "bucket 0 not final after the first half"
    assert np.abs(g3 - gw).max() <= tol, "two halves differ from the whole backward"
    if n_buckets == 2:
        o1, c1 = buckets[1]
        assert np.abs(gw[o1:o1 + c1]).max() > 0 and np.abs(g2[o1:o1 + c1] - gw[o1:o1 + c1]).max() > 0   # the first half really stops early


# ---- what a fused step hands from its forward to its backward stays inside that call (check_step_handoffs) -------------------------------
# The launches of each form on d128 / H4 / F64 / L2 at batch 2 as (family, phase or kind), written down from the GT_TRACE_DISPATCH lines of
# the commit BEFORE the hand-offs became arguments (profiles/step_handoffs_trace.txt): the QUAD schedule with riders and head_dim 32,
# where gt_train_step's last forward launch runs backward phase 0 and takes the loss along.
HANDOFF_CFG, HANDOFF_B = dict(d_model=128, n_heads=4, dim_feedforward=64, num_encoder_layers=2, num_decoder_layers=0, embedding_size_src=16), 2
_FWD = [("seq_pack", None), ("seq_fwd", 0), ("seq_fwd", 1)]
HANDOFF_WHOLE = _FWD + [("seq_bwd", 1), ("seq_bwd", 2), ("seq_tail", "tail"), ("update", "folded_pack")]          # gt_step_launches = 7
HANDOFF_BACKWARD = [("kernel", None), ("seq_bwd", 0), ("seq_bwd", 1), ("seq_bwd", 2), ("seq_tail", "tail")]       # heads_bwd first
HANDOFF_SKIP2, HANDOFF_SKIP3 = _FWD + [("seq_bwd", 1), ("seq_tail", "out_early")], [("seq_bwd", 2), ("seq_tail", "tail")]
HANDOFF_STEP_LOSS = _FWD + [("kernel", None), ("seq_bwd", 0), ("seq_bwd", 1), ("seq_bwd", 2), ("seq_tail", "tail"), ("update", "folded_pack")]


def check_step_handoffs(backend, read_trace):
    """One Runner, back to back: a whole gt_train_step, gt_forward + gt_loss + gt_backward, gt_train_step(skip_update 2, then 3), a whole
    gt_train_step_loss, a gt_train_step that fails (stats = NULL), another whole gt_train_step.  read_trace() returns the [dispatch] lines
    since its last call (the caller has GT_TRACE_DISPATCH on).  Each part keeps its bar: whole steps check_train_step's (loss 2e-5,
    check_update), forward / loss / backward check_step's, the two-call backward check_step's gradient bar."""
    cfg, B, lr, pen = dict(HANDOFF_CFG, dropout=0.1), HANDOFF_B, 0.05, 0.38
    r = Runner(cfg, B, backend, rng=(77, 5, 0), lr=lr)
    r.set_params(ng.init_params(cfg, seed=9, perturb=0.05))
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=4)
    y64 = y.astype(np.float64)
    n = r.lib.cdll.gt_step_launches(ctypes.byref(r.c))
    assert n == len(HANDOFF_WHOLE), n
    seq = lambda tr: [(f, d.get("phase", d.get("kind"))) for f, d in tr]
    fused = lambda tr: [d["fuse_b0"] for f, d in tr if f in ("seq_fwd", "seq_bwd")]

    def oracle(before):
        """the fp64 step from the device's parameters `before` with this step's masks -> (stats, cache, d loss / d hvo, gradients)"""
        P64 = {k: np.asarray(v, np.float64) for k, v in before.items()}
        hvo, C = ng.forward(P64, cfg, x, rng=(77, 5, r.step_state().step), dtype=np.float64)
        stats, dpred = ng.calculate_loss(hvo, y64, pen)
        return P64, hvo, stats, C, dpred

    def grads_of(P64, C, dpred):
        assert check_decisions_current(r, C) >= len(C["enc"]) + 1
        assert adopt_device_kinks(r, C, cfg) <= kink_bound(r, cfg)
        return ng.backward(P64, cfg, C, dpred, dtype=np.float64)

    def whole_step(call, tag):
        before = r.unflatten(r.params.numpy())
        P64, _, want, C, dpred = oracle(before)
        read_trace()
        stats = call()
        tr = read_trace()
        assert abs(stats[0] - want[0]) < 2e-5 * max(1, abs(want[0])), (tag, stats[0], want[0])
        check_update(before, r.unflatten(r.params.numpy()), grads_of(P64, C, dpred), lr, tag=tag)
        return tr

    def grads_within_bar(G, Gr, tag):
        for k in Gr:
            err = float(np.abs(G[k] - Gr[k]).max() / max(np.abs(Gr[k]).max(), 1e-5))
            assert err < GRAD_TOL, (tag, k, err)

    first = whole_step(lambda: r.train_step(x, y, pen), "first whole step")
    assert seq(first) == HANDOFF_WHOLE and fused(first) == [0, 1, 1, 1], first
    # a plain forward takes no loss along and runs no backward phase; the gt_backward after it runs phase 0 itself
    P64, hvo_ref, _, C, _ = oracle(r.unflatten(r.params.numpy()))
    read_trace()
    hvo = r.forward(x, None, train=True)
    fwd = read_trace()
    assert seq(fwd) == _FWD and fused(fwd) == [0, 0], fwd
    dpred = _check_forward_and_loss(r, hvo, hvo_ref, C, y, pen, True)
    assert seq(read_trace()) == [("kernel", None)]
    G = r.backward(train=True)
    bwd = read_trace()
    assert seq(bwd) == HANDOFF_BACKWARD and fused(bwd) == [0, 0, 0], bwd
    grads_within_bar(G, grads_of(P64, C, dpred), "gt_backward")
    # the two halves of the bucketed backward: the first call's forward runs phase 0, the second call starts at phase 2
    P64, _, want, C, dpred = oracle(r.unflatten(r.params.numpy()))
    read_trace()
    stats = r.train_step(x, y, pen, skip_update=2)
    half1 = read_trace()
    r.train_step(x, y, pen, skip_update=3)
    half2 = read_trace()
    r._grads_dirty = True
    assert seq(half1) == HANDOFF_SKIP2 and fused(half1) == [0, 1, 1], half1
    assert seq(half2) == HANDOFF_SKIP3 and fused(half2) == [0], half2
    assert abs(stats[0] - want[0]) < 2e-5 * max(1, abs(want[0])), (stats[0], want[0])
    grads_within_bar(r.unflatten(r.grads.numpy()), grads_of(P64, C, dpred), "skip_update 2 + 3")
    # gt_train_step_loss (neutral options: gt_loss's numbers): the loss between forward and backward, phase 0 a backward launch again
    from transformergrooveinfilling_amd import _lib
    lo = _lib.make_loss_opts(penalty_h=pen)
    voice, scratch = r.Buf(np.zeros(36, np.float32)), r.Buf(np.zeros(int(r.lib.cdll.gt_loss_scratch_floats(ctypes.byref(r.c))), np.float32))

    def step_loss():
        r.grads = r.Buf(np.zeros(r.total, np.float32))
        r._grads_dirty = False
        r.lib.call("gt_train_step_loss", ctypes.byref(r.c), 0, r.params.ptr, r.grads.ptr, None, None, r.pe.ptr, r.x.ptr, r.y.ptr, ctypes.byref(lo),
                   voice.ptr, scratch.ptr, r.hvo.ptr, r.stats.ptr, r.tgt.ptr, r.ws.ptr, r.state.ptr, 0, r.stream)
        return r.stats.numpy().copy()
    by_opts = whole_step(step_loss, "gt_train_step_loss")
    assert len(by_opts) == n + 2 and seq(by_opts) == HANDOFF_STEP_LOSS and fused(by_opts) == [0, 0, 0, 0, 0], by_opts
    # a call that fails launches nothing, changes nothing and leaves nothing behind for the step after it
    keep = [b.numpy().copy() for b in (r.params, r.grads, r.state, r.hvo)]
    read_trace()
    rc = r.lib.cdll.gt_train_step(ctypes.byref(r.c), 0, r.params.ptr, r.grads.ptr, None, None, r.pe.ptr, r.x.ptr, r.y.ptr, ctypes.c_float(pen),
                                  r.hvo.ptr, None, r.tgt.ptr, r.ws.ptr, r.state.ptr, 0, r.stream)
    assert rc != 0 and b"stats" in r.lib.cdll.gt_last_error(), rc
    assert read_trace() == [], "gt_train_step(stats = NULL) launched before it failed"
    assert all(np.array_equal(a, b.numpy()) for a, b in zip(keep, (r.params, r.grads, r.state, r.hvo)))
    last = whole_step(lambda: r.train_step(x, y, pen), "last whole step")
    assert last == first, (first, last)
    assert r.step_state().step == 3 and r.step_state().opt_step == 3
