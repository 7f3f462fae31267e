"""numpy restatement of the infilling draw (gt_gather_infill) and of both merge modes (gt_infill_merge), written from the
specification in include/groove_hip.h: plain Python integers masked to 32 bits, no floating point in the draw.  Shared by
tests/test_infill.py (host emulator) and tests/test_infill_gpu.py (MI355X)."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.numpy_groove import site_key  # noqa: E402

SITE_INFILL = 2
M32 = 0xFFFFFFFF


def fmix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def infill_key(seed_lo, seed_hi, step):
    return int(site_key(seed_lo, seed_hi, step, SITE_INFILL))


def active_mask(groove):
    """bit c set iff voice c has a non-zero hit value anywhere in the (32,27) groove"""
    hits = np.asarray(groove)[:, :9] != 0
    return sum(1 << c for c in range(9) if hits[:, c].any())


def size_weights(active, opts):
    """-> (n_act, hi, {k: W_k}) for a sequence with the given activity bits; opts = (voice_mask, min_remove, max_remove, weights)"""
    mask, lo, hi_opt, w = opts
    n_tot = bin(active).count("1")
    n_act = bin(active & mask).count("1")
    hi = min(hi_opt, n_act, n_tot - 1)
    return n_act, hi, {k: int(w[k - lo]) * math.comb(n_act, k) for k in range(lo, hi + 1)}


def draw(active, src, key, opts):
    """the removal bitmask of source index src (already clamped); 0 = ineligible"""
    mask, lo, _, _ = opts
    n_act, hi, W = size_weights(active, opts)
    T = sum(W.values())
    if T == 0:
        return 0
    r = lambda j: fmix32((((src * 16 + j) & M32) * 0x9E3779B1 & M32) ^ key)
    pick = (r(0) * T) >> 32
    run, k = 0, hi
    for kk in range(lo, hi + 1):
        run += W[kk]
        if run > pick:
            k = kk
            break
    need, left, removed = k, n_act, 0
    for c in range(9):
        if not (active & mask) >> c & 1:
            continue
        if ((r(1 + c) * left) >> 32) < need:
            removed |= 1 << c
            need -= 1
        left -= 1
    assert need == 0
    return removed


def column_mask(removed):
    """(27,) bool: the h / v / o columns of the voices in the bitmask"""
    return np.array([(removed >> (j % 9)) & 1 for j in range(27)], bool)


def gather_infill(hvo_set, idx, opts, seed_lo, seed_hi, step):
    """-> x (B,32,27), y (B,32,27), removed (B,) int32: what gt_gather_infill writes"""
    hvo_set = np.asarray(hvo_set, np.float32)
    n = hvo_set.shape[0]
    key = infill_key(seed_lo, seed_hi, step)
    B = len(idx)
    x, y, removed = np.zeros((B, 32, 27), np.float32), np.zeros((B, 32, 27), np.float32), np.zeros(B, np.int32)
    for b, i in enumerate(idx):
        src = min(max(int(i), 0), n - 1)
        g = hvo_set[src]
        removed[b] = draw(active_mask(g), src, key, opts)
        cm = column_mask(int(removed[b]))
        x[b][:, ~cm] = g[:, ~cm]
        y[b][:, cm] = g[:, cm]
    return x, y, removed


def eligible(hvo_set, opts):
    """indices of the sequences with T > 0"""
    return np.array([i for i, g in enumerate(np.asarray(hvo_set)) if sum(size_weights(active_mask(g), opts)[2].values()) > 0], np.int64)


def merge(pred, inp, removed, mode):
    """gt_infill_merge on (n_seq,32,27) arrays; removed: (n_seq,) bitmasks or None"""
    pred, inp = np.array(pred, np.float32, copy=True), np.asarray(inp, np.float32)
    if removed is not None:
        for s, m in enumerate(removed):
            pred[s][:, ~column_mask(int(m))] = 0.0
    ph, pv, po = pred[..., :9], pred[..., 9:18], pred[..., 18:]
    ih, iv, io = inp[..., :9], inp[..., 9:18], inp[..., 18:]
    hit = ih != 0
    if mode == 0:
        return np.concatenate([np.where(hit, ih, ph + ih), pv + iv, po + io], -1).astype(np.float32)
    return np.concatenate([np.where(hit, ih, ph), np.where(hit, iv, pv), np.where(hit, io, po)], -1).astype(np.float32)
