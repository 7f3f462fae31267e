"""Weight regimes away from initialisation, and the bars that go with them.

ng.init_params(..., perturb=0.05) puts every model of the suite in one corner: attention scores within +-1.2 (softmax nearly uniform: the
largest probability of a row averages 0.05), hit logits within +-1.7, every LayerNorm variance near 1.  A regime is a pure function
(P, cfg, seed) -> P that moves the initial parameters out of that corner while the model stays well conditioned; it works in float64,
draws from np.random.default_rng(seed + 1000) and rounds to fp32 at the end.  Each regime has a CONDITION on the fp64 oracle's cache
(assert_condition): a later change of seeds or shapes that silently leaves the regime fails there, not nowhere.

Bars (parity.check_step(regime=...)): every compared quantity keeps the suite's fixed bar AND stays within NOISE_FACTOR x the fp32 oracle's
own distance from the fp64 oracle (Noise).  Away from initialisation the fixed bars alone are either unreachable (stock fp32 numpy is
2.9e-5 off fp64 on hit logits of +-48, absolute) or wide (a LayerNorm eps of 1e-6 sits 10 - 40 x over the fp32 noise and 3 - 30 x under
the output and gradient bars): profiles/regimes.txt."""
import math

import numpy as np

NOISE_FACTOR = 8.0               # device error <= 8 x max(fp32 oracle's error, the floor): summation order, libm and the weight gradients'
#                                  atomics are each a bounded, order-one multiple of the same rounding noise (worst 3.6 on the emulator, 3.9 on the MI355X; typical 0.8 - 1.6)
NOISE_FLOOR = 4 * 2.0 ** -23     # ... floor: 4 ulp of the quantity's scale, so that a tensor numpy happened to round luckily sets no impossible bar


def _f64(P):
    return {k: np.asarray(v, np.float64).copy() for k, v in P.items()}


def _f32(P):
    return {k: v.astype(np.float32) for k, v in P.items()}


def peaked(P, cfg, seed):
    """Q and K rows of every in-proj x 6, every in-proj bias += N(0, 0.5): the largest probability of a row averages 0.5 - 0.9, up to a third
    of the rows are one-hot to fp32 -- the softmax backward's P (dP - sum dP P) cancels, exp() runs over its whole range below 0."""
    rnd, d, P = np.random.default_rng(seed + 1000), cfg["d_model"], _f64(P)
    for k in P:
        if k.endswith("in_proj_weight"):
            P[k][:2 * d] *= 6.0
        if k.endswith("in_proj_bias"):
            P[k] += rnd.normal(0, 0.5, P[k].shape)
    return _f32(P)


def shift(P, cfg, seed):
    """Q and K rows x 3, the K slice of every in-proj bias += N(0, 40).  A K bias adds q_i . b_k to the whole of score row i: the softmax is
    unchanged in exact arithmetic, the raw scores reach +-190 ... +-365 and the row maxima run from far below -88 to far above +88 -- a kernel
    that exponentiates without subtracting the row's maximum returns inf / inf or 0 / 0."""
    rnd, d, P = np.random.default_rng(seed + 1000), cfg["d_model"], _f64(P)
    for k in P:
        if k.endswith("in_proj_bias"):
            P[k][d:2 * d] += rnd.normal(0, 40.0, d)
        if k.endswith("in_proj_weight"):
            P[k][:2 * d] *= 3.0
    return _f32(P)


def saturated(P, cfg, seed):
    """Output layer weight x 30, bias += N(0, 3): |hit logit| reaches 23 - 91 and a quarter to three quarters of them exceed 10 -- the stable
    BCE form, both loss implementations, the sigmoid where exp() overflows and 0.5 tanh at its plateau."""
    rnd, P = np.random.default_rng(seed + 1000), _f64(P)
    P["OutputLayer.Linear.weight"] *= 30.0
    P["OutputLayer.Linear.bias"] += rnd.normal(0, 3.0, P["OutputLayer.Linear.bias"].shape)
    return _f32(P)


def flat(P, cfg, seed):
    """Every LayerNorm gain x 0.02, every LayerNorm bias = N(0, 0.01), every out-proj, linear1 and linear2 bias x 0.02: every LayerNorm after
    the first sees a variance of 4e-4 ... 6e-4, where eps = 1e-5 decides several per cent of rstd.  (With LayerNorm biases of N(0, 0.02) and
    linear1's bias left alone the feed-forward branch alone brings 1e-3 ... 3e-3 to norm2's input and the condition below does not hold.)"""
    rnd, P = np.random.default_rng(seed + 1000), _f64(P)
    for k in P:
        if "norm" in k:
            P[k] = P[k] * 0.02 if k.endswith("weight") else rnd.normal(0, 0.01, P[k].shape)
        if k.endswith(("out_proj.bias", "linear1.bias", "linear2.bias")):
            P[k] *= 0.02
    return _f32(P)


REGIMES = dict(peaked=peaked, shift=shift, saturated=saturated, flat=flat)


def apply(P, cfg, regime, seed):
    """regime None: P itself, untouched"""
    return P if regime is None else REGIMES[regime](P, cfg, seed)


def figures(C, h):
    """what the conditions look at, from the fp64 oracle's cache C and hit logits h"""
    a = C["enc"][0]["attn"]
    S = (a["qh"] @ a["kh"].transpose(0, 1, 3, 2)) / math.sqrt(a["qh"].shape[-1])
    c0 = C["enc"][0]
    layers = C["enc"] + C["dec"]
    return dict(peak=max(float(c["attn"]["P"].max(-1).mean()) for c in layers),
                rowmax_min=float(S.max(-1).min()), rowmax_max=float(S.max(-1).max()),
                big_logits=float((np.abs(h) > 10).mean()), h_max=float(np.abs(h).max()),
                var_norm2=float(np.median(1.0 / np.asarray(c0["rstd2"], np.float64) ** 2 - 1e-5)))


def assert_condition(regime, C, h):
    """the regime's own condition on the fp64 oracle's cache: the weights really are where the regime says.  Returns figures(C, h)."""
    f = figures(C, h)
    if regime == "peaked":
        assert f["peak"] >= 0.4, "peaked: the mean largest probability of a row is %.3f < 0.4 in every layer" % f["peak"]
    elif regime == "shift":
        assert f["rowmax_min"] < -88 and f["rowmax_max"] > 88, "shift: layer 0's row maxima run from %.1f to %.1f only" % (f["rowmax_min"], f["rowmax_max"])
    elif regime == "saturated":
        assert f["big_logits"] >= 0.2, "saturated: only %.1f %% of the hit logits exceed 10" % (100 * f["big_logits"])
    elif regime == "flat":
        assert f["var_norm2"] < 1e-3, "flat: the median variance at layer 0's norm2 is %.3g" % f["var_norm2"]
    else:
        raise KeyError(regime)
    return f


def same_kinks(C32, C):
    """The fp32 oracle differentiates the function the fp64 oracle does: where its ReLU decisions differ from cache C's (after C adopted the
    device's at the kink), take C's -- otherwise one flipped element would count as fp32 noise and widen the bar."""
    todo = [(a, b, "hpre") for a, b in zip(C32["enc"] + C32["dec"], C["enc"] + C["dec"])] + [(C32["in_enc"], C["in_enc"], "a")]
    for c32, c, key in todo:
        want = c[key] > 0
        flips = (c32[key] > 0) != want
        if flips.any():
            c32[key][flips] = np.where(want[flips], 1e-30, -1e-30).astype(c32[key].dtype)


class Noise:
    """Per compared quantity: the device's error and the fp32 oracle's error (both max |. - ref64|) and the quantity's scale.  add() records a
    row (name, err, noise, scale, ratio = err / max(noise, NOISE_FLOOR x scale)) and returns err / scale; check() asserts every ratio."""

    def __init__(self):
        self.rows = []

    def add(self, name, dev, ref32, ref64, scale=None):
        ref64 = np.asarray(ref64, np.float64)
        dev = np.asarray(dev, np.float64).reshape(ref64.shape)
        ref32 = np.asarray(ref32, np.float64).reshape(ref64.shape)
        scale = float(np.abs(ref64).max()) if scale is None else float(scale)
        assert np.isfinite(dev).all(), "%s: the device's values are not finite" % name
        err, noise = float(np.abs(dev - ref64).max()), float(np.abs(ref32 - ref64).max())
        self.rows.append((name, err, noise, scale, err / max(noise, NOISE_FLOOR * scale, 1e-300)))
        return err / max(scale, 1e-300)

    def worst(self):
        return max(self.rows, key=lambda r: r[4]) if self.rows else ("-", 0.0, 0.0, 0.0, 0.0)

    def check(self):
        over = [r for r in self.rows if not r[4] <= NOISE_FACTOR]
        assert not over, "; ".join("%s: device error %.3g is %.1f x max(the fp32 oracle's own error %.3g, 4 ulp of the scale %.3g), bar %g x"
                                   % (n, e, q, z, s, NOISE_FACTOR) for n, e, z, s, q in over)
