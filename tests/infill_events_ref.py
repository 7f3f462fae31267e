"""numpy restatement of the event-level infilling draw (gt_gather_infill_events) and of the cell-masked merge (gt_infill_merge_cells),
written from the specification in include/groove_hip.h: plain Python integers masked to 32 bits, no floating point in the draw.  Shared by
tests/test_infill_events.py (host emulator) and tests/test_infill_events_gpu.py (MI355X)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from infill_ref import M32, fmix32  # noqa: E402
from oracle.numpy_groove import site_key  # noqa: E402

SITE_INFILL_EVENTS = 3
CELLS = 288


def events_key(seed_lo, seed_hi, step):
    return int(site_key(seed_lo, seed_hi, step, SITE_INFILL_EVENTS))


def flags(groove, voice_mask):
    """-> (event, candidate): two lists of 288 bools, cell j = t * 9 + c"""
    h = np.asarray(groove)[:, :9]
    ev = [bool(h[j // 9, j % 9] != 0) for j in range(CELLS)]
    return ev, [ev[j] and bool(voice_mask >> (j % 9) & 1) for j in range(CELLS)]


def count(groove, opts):
    """-> (n_ev, n_cand, cap); opts = (voice_mask, ratio_lo, ratio_hi) in 1/65536ths"""
    ev, cand = flags(groove, opts[0])
    n_ev, n_cand = sum(ev), sum(cand)
    return n_ev, n_cand, min(n_cand, n_ev - 1)


def size(groove, src, key, opts):
    """k of the specification for source index src (already clamped); 0 = ineligible"""
    _, lo, hi = opts
    _, n_cand, cap = count(groove, opts)
    if cap < 1:
        return 0
    base = (src * 512) & M32
    r0 = fmix32(((base * 0x9E3779B1) & M32) ^ key)
    q = lo + ((r0 * (hi - lo + 1)) >> 32)
    k0 = ((n_cand * q + 32768) & M32) >> 16
    return min(max(k0, 1), cap)


def draw(groove, src, key, opts):
    """the set of removed cells j of source index src (already clamped): the k candidates with the smallest hash"""
    k = size(groove, src, key, opts)
    if k == 0:
        return set()
    _, cand = flags(groove, opts[0])
    base = (src * 512) & M32
    r = {j: fmix32((((base + 1 + j) & M32) * 0x9E3779B1 & M32) ^ key) for j in range(CELLS) if cand[j]}
    assert len(set(r.values())) == len(r)                      # (pairwise different: no tie rule)
    removed = {j for j in r if sum(1 for i in r if r[i] < r[j]) < k}
    assert len(removed) == k
    return removed


def words(removed):
    """nine uint32: bit t of word c set iff cell t * 9 + c is in the set"""
    w = [0] * 9
    for j in removed:
        w[j % 9] |= 1 << (j // 9)
    return w


def cell_mask(w):
    """(32,27) bool from nine bit words: the h / v / o entries of the cells whose bit is set"""
    m = np.zeros((32, 27), bool)
    for c in range(9):
        for t in range(32):
            if int(w[c]) >> t & 1:
                m[t, [c, 9 + c, 18 + c]] = True
    return m


def gather_infill_events(hvo_set, idx, opts, seed_lo, seed_hi, step):
    """-> x (B,32,27), y (B,32,27), cells (B,9) uint32: what gt_gather_infill_events writes"""
    hvo_set = np.asarray(hvo_set, np.float32)
    n = hvo_set.shape[0]
    key = events_key(seed_lo, seed_hi, step)
    B = len(idx)
    x, y, cells = np.zeros((B, 32, 27), np.float32), np.zeros((B, 32, 27), np.float32), np.zeros((B, 9), np.uint32)
    for b, i in enumerate(idx):
        src = min(max(int(i), 0), n - 1)
        g = hvo_set[src]
        cells[b] = words(draw(g, src, key, opts))
        m = cell_mask(cells[b])
        x[b][~m] = g[~m]
        y[b][m] = g[m]
    return x, y, cells


def eligible(hvo_set, opts):
    """indices of the sequences with cap >= 1"""
    return np.array([i for i, g in enumerate(np.asarray(hvo_set)) if count(g, opts)[2] >= 1], np.int64)


def merge_cells(pred, inp, cells, mode):
    """gt_infill_merge_cells on (n_seq,32,27) arrays; cells: (n_seq,9) bit words or None"""
    pred, inp = np.array(pred, np.float32, copy=True), np.asarray(inp, np.float32)
    if cells is not None:
        for s in range(pred.shape[0]):
            pred[s][~cell_mask(cells[s])] = 0.0
    ph, pv, po = pred[..., :9], pred[..., 9:18], pred[..., 18:]
    ih, iv, io = inp[..., :9], inp[..., 9:18], inp[..., 18:]
    hit = ih != 0
    if mode == 0:
        return np.concatenate([np.where(hit, ih, ph + ih), pv + iv, po + io], -1).astype(np.float32)
    return np.concatenate([np.where(hit, ih, ph), np.where(hit, iv, pv), np.where(hit, io, po)], -1).astype(np.float32)
