"""numpy restatement of gt_hit_curve / gt_hit_thresholds (include/groove_hip.h): the counts by np.bincount, the choice in fp64."""
import numpy as np


def curve(prob, hvo_gt, grid):
    """prob (..., 9) fp32, hvo_gt (..., 27), grid (K,) fp32 ascending -> (9, 2, K + 1) int64"""
    grid = np.asarray(grid, np.float32)
    nb = len(grid) + 1
    p = np.asarray(prob, np.float32).reshape(-1, 9)
    g = (np.asarray(hvo_gt, np.float32).reshape(-1, 27)[:, :9] == np.float32(1)).astype(np.int64)
    b = (p[..., None] > grid).sum(-1)                              # strict, fp32; NaN > x is False: bin 0
    key = (np.arange(9)[None, :] * 2 + g) * nb + b
    return np.bincount(key.reshape(-1), minlength=9 * 2 * nb).reshape(9, 2, nb).astype(np.int64)


def rates(counts):
    """-> TP (9, K), FP (9, K), P (9,) as int64: TP_k = sum of counts[c][1][b] over b > k"""
    c = np.asarray(counts).astype(np.int64)
    above = np.cumsum(c[..., ::-1], -1)[..., ::-1][..., 1:]
    return above[:, 1], above[:, 0], c[:, 1].sum(-1)


def fbeta(TP, FP, P, beta):
    b = np.float64(np.float32(beta))
    b2 = b * b
    a = (1.0 + b2) * TP.astype(np.float64)
    den = (a + b2 * (P[..., None] - TP).astype(np.float64)) + FP.astype(np.float64)
    return np.where(TP > 0, a / np.where(den > 0, den, 1.0), 0.0)


def select(counts, grid, criterion=0, beta=1.0, fallback=0.5):
    """-> thresholds (9,) fp32, index (9,) int, scores (9, 4) fp64 = precision, recall, F-beta, density ratio; and per voice the list of
    candidate indices (the tests look at plateaus)"""
    grid = np.asarray(grid, np.float32)
    TP, FP, P = rates(counts)
    F = fbeta(TP, FP, P, beta)
    thr, idx, sc, cands = np.full(9, np.float32(fallback)), np.full(9, -1), np.zeros((9, 4)), []
    for c in range(9):
        if criterion == 0:
            cand = np.flatnonzero(F[c] == F[c].max()) if F[c].max() > 0 else []
        else:
            dist = np.abs(TP[c] + FP[c] - P[c])
            cand = np.flatnonzero(dist == dist.min())
        cand = list(cand) if P[c] > 0 else []
        cands.append(cand)
        if not cand:
            continue
        k = cand[(len(cand) - 1) // 2]
        idx[c], thr[c] = k, grid[k]
        placed = TP[c, k] + FP[c, k]
        sc[c] = [TP[c, k] / placed if placed else 0.0, TP[c, k] / P[c], F[c, k], placed / P[c]]
    return thr, idx, sc, cands


def fbeta_gaps(counts, beta):
    """per voice decided by F-beta: best minus second-best DISTINCT score (inf when there is one score only)"""
    TP, FP, P = rates(counts)
    F = fbeta(TP, FP, P, beta)
    out = []
    for c in range(9):
        u = np.unique(F[c])
        if P[c] > 0 and u[-1] > 0:
            out.append(float(u[-1] - u[-2]) if len(u) > 1 else float("inf"))
    return out
