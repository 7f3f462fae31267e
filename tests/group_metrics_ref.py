"""numpy restatement of gt_group_metrics (include/groove_hip.h): the same fp32 arithmetic per cell (np.float32 gives the same bits), the
sums as Python / int64 integers -- every comparison with it is exact integer equality."""
import numpy as np

WORDS = 8


def acc_words(n_groups):
    return n_groups * (9 * WORDS + 2) + 1


def cell_bits(cells, n_seq):
    """cells: None | (n_seq, 9) uint32 words -> (n_seq, 32, 9) bool, bit t of cells[s, c] = cell (s, t, c)"""
    if cells is None:
        return np.ones((n_seq, 32, 9), bool)
    w = np.asarray(cells).astype(np.uint32).reshape(n_seq, 1, 9)
    return ((w >> np.arange(32, dtype=np.uint32).reshape(1, 32, 1)) & np.uint32(1)).astype(bool)


def _fix(e):
    """(values as int64 with the rejected ones 0, rejected mask): fix(e) = (uint64)((double)e * 2^32 + 0.5) for e <= 16"""
    with np.errstate(invalid="ignore"):
        ok = e <= np.float32(16)                                    # NaN <= x is False
    safe = np.where(ok, e, np.float32(0)).astype(np.float64)
    return np.floor(safe * 4294967296.0 + 0.5).astype(np.int64), ~ok


def group_metrics(hvo_pred, hvo_gt, group=None, cells=None, n_groups=1):
    """-> (acc (acc_words,) int64: what one call ADDS, seq_out (n_seq, 4) int64)"""
    p = np.asarray(hvo_pred, np.float32).reshape(-1, 32, 27)
    g = np.asarray(hvo_gt, np.float32).reshape(-1, 32, 27)
    n = p.shape[0]
    m = cell_bits(cells, n)
    ph, gh = p[..., :9] == np.float32(1), g[..., :9] == np.float32(1)
    with np.errstate(invalid="ignore", over="ignore"):
        dv = p[..., 9:18] - g[..., 9:18]
        do = p[..., 18:] - g[..., 18:]
        ev, eo = (dv * dv).astype(np.float32), (do * do).astype(np.float32)
    fv, bad_v = _fix(ev)
    fo, bad_o = _fix(eo)
    tp, fp, fn = ph & gh & m, ph & ~gh & m, ~ph & gh & m
    per = np.stack([m, tp, fp, fn], -1).astype(np.int64)            # (n, 32, 9, 4)
    fixed = np.stack([fv * m, fo * m, fv * tp, fo * tp], -1)        # (n, 32, 9, 4)
    cellw = np.concatenate([per, fixed], -1).sum(1)                 # (n, 9, 8): summed over the steps
    rej = ((bad_v & m).sum((1, 2)) + (bad_o & m).sum((1, 2))).astype(np.int64)
    gid = np.zeros(n, np.int64) if group is None else np.asarray(group).astype(np.int64).reshape(n)
    acc = np.zeros(acc_words(n_groups), np.int64)
    tail = n_groups * 9 * WORDS
    for s in range(n):
        k = int(gid[s])
        if k < 0 or k >= n_groups:
            acc[-1] += 1
            continue
        acc[k * 72:(k + 1) * 72] += cellw[s].reshape(-1)
        acc[tail + 2 * k] += 1
        acc[tail + 2 * k + 1] += rej[s]
    return acc, per.sum((1, 2))


def split(acc, n_groups):
    """acc -> (words (n_groups, 9, 8), sequences (n_groups,), rejected (n_groups,), skipped)"""
    a = np.asarray(acc).astype(np.int64).reshape(-1)
    tail = a[n_groups * 72:n_groups * 74].reshape(n_groups, 2)
    return a[:n_groups * 72].reshape(n_groups, 9, WORDS), tail[:, 0], tail[:, 1], int(a[-1])
