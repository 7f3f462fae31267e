"""numpy restatement of gt_groove_features (include/groove_hip.h): the same fp32 arithmetic per cell (np.float32 gives the same bits), the
sums as int64 integers (word 12 in two's complement, as the device sums it) -- every comparison with it is exact integer equality."""
import numpy as np

WORDS, PAIR_WORDS, LAGS = 32, 8, 17
F16 = np.float32(16)


def _fix(e):
    """(uint64)((double)e * 2^32 + 0.5) of non-negative fp32 values, as int64"""
    return np.floor(e.astype(np.float64) * 4294967296.0 + 0.5).astype(np.int64)


def _cells(hvo):
    """hvo (n,32,27) fp32 -> dict of (n,32,9) arrays: hit, okv / oko (a hit with a valid value), v' / o' (the value where valid, else 0)"""
    h = hvo[..., :9] == np.float32(1)
    v, o = hvo[..., 9:18], hvo[..., 18:]
    with np.errstate(invalid="ignore"):
        okv = h & (np.float32(0) <= v) & (v <= F16)                 # (a NaN fails both)
        oko = h & (np.abs(o) <= F16)
    zero = np.float32(0)
    return dict(hit=h, okv=okv, oko=oko, v=np.where(okv, v, zero).astype(np.float32), o=np.where(oko, o, zero).astype(np.float32))


def _profile(c):
    """P (n,32) int64: the sum over the voices of q(v) = (uint32)((double)v * 65536 + 0.5) over the hits with a valid velocity"""
    q = np.floor(c["v"].astype(np.float64) * 65536.0 + 0.5).astype(np.int64)
    return (q * c["okv"]).sum(2)


def record(hvo):
    """-> (n, 32) int64: the words of one buffer's record"""
    hvo = np.asarray(hvo, np.float32).reshape(-1, 32, 27)
    n = hvo.shape[0]
    c = _cells(hvo)
    h, t = c["hit"], np.arange(32)
    out = np.zeros((n, WORDS), np.int64)
    out[:, 0] = h.sum((1, 2))
    out[:, 1] = h.any(1).sum(1)
    out[:, 2] = h.any(2).sum(1)
    out[:, 3] = h[:, t % 4 == 0].sum((1, 2))
    out[:, 4] = h[:, t % 4 == 2].sum((1, 2))
    out[:, 5] = h[:, t % 2 == 1].sum((1, 2))
    out[:, 6] = (h[:, :16] & h[:, 16:]).sum((1, 2))
    out[:, 7] = (h & ~c["okv"]).sum((1, 2))
    out[:, 8] = (h & ~c["oko"]).sum((1, 2))
    v, o = c["v"], c["o"]
    with np.errstate(over="ignore"):
        out[:, 9] = (_fix(v) * c["okv"]).sum((1, 2))
        out[:, 10] = (_fix((v * v).astype(np.float32)) * c["okv"]).sum((1, 2))
        out[:, 11] = (_fix(np.abs(o)) * c["oko"]).sum((1, 2))
        out[:, 12] = (np.where(o >= 0, _fix(np.abs(o)), -_fix(np.abs(o))) * c["oko"]).sum((1, 2))
        out[:, 13] = (_fix((o * o).astype(np.float32)) * c["oko"]).sum((1, 2))
    P = _profile(c)
    for l in range(LAGS):
        out[:, 15 + l] = (P * np.roll(P, -l, axis=1)).sum(1)        # P[t] * P[(t + l) mod 32]
    return out


def pair_words(hvo_a, hvo_b):
    """-> (n, 8) int64: p = buffer a, g = buffer b"""
    a = np.asarray(hvo_a, np.float32).reshape(-1, 32, 27)
    b = np.asarray(hvo_b, np.float32).reshape(-1, 32, 27)
    ca, cb = _cells(a), _cells(b)
    p, g = ca["hit"], cb["hit"]
    out = np.zeros((a.shape[0], PAIR_WORDS), np.int64)
    out[:, 0] = (p != g).sum((1, 2))
    out[:, 1] = (p & g).sum((1, 2))

    def neighbour(x):                                               # a hit of the same voice at t - 1 or t + 1; no wrap-around
        nb = np.zeros_like(x)
        nb[:, 1:] |= x[:, :-1]
        nb[:, :-1] |= x[:, 1:]
        return nb
    out[:, 2] = (p & ~g & neighbour(g)).sum((1, 2)) + (g & ~p & neighbour(p)).sum((1, 2))
    dv = (ca["v"] - cb["v"]).astype(np.float32)
    out[:, 3] = _fix((dv * dv).astype(np.float32)).sum((1, 2))
    both = ca["oko"] & cb["oko"]
    do = (ca["o"] - cb["o"]).astype(np.float32)
    out[:, 4] = (_fix((do * do).astype(np.float32)) * both).sum((1, 2))
    out[:, 5] = both.sum((1, 2))
    out[:, 6] = (_profile(ca) * _profile(cb)).sum(1)
    return out


def groove_features(hvo_a, hvo_b=None):
    """-> (feat_a, feat_b or None, pair or None)"""
    if hvo_b is None:
        return record(hvo_a), None, None
    return record(hvo_a), record(hvo_b), pair_words(hvo_a, hvo_b)
