"""Per-voice evaluation metrics on the device.

The reference logs, three times per epoch, what its GrooveEvaluator computes from ``model.predict`` (ref:evaluator.py:171-177,
522-525): ``get_hits_accuracies`` / ``get_velocity_errors`` / ``get_micro_timing_errors`` over the 9 voices of
``ROLAND_REDUCED_MAPPING`` -- after three ``.cpu()`` copies of the predictions.  Here the (N,32,27) prediction tensor never
leaves the GPU: one reduction (gt_voice_metrics, bitwise reproducible) yields 30 floats, and those are what goes to the host /
W&B.  The evaluator itself is un-vendored (GrooveEvaluator submodule), so the dictionary keys below are this package's own;
the quantities are: fraction of (sequence, step) cells whose hit equals the ground truth's, and mean squared velocity / offset
difference over all cells, per voice and averaged over voices.
"""
import torch

# voice order of hvo_sequence's ROLAND_REDUCED_MAPPING (9 voices; column j of each of the three 9-wide HVO blocks)
VOICES = ("KICK", "SNARE", "HH_CLOSED", "HH_OPEN", "TOM_3_LO", "TOM_2_MID", "TOM_1_HI", "CRASH", "RIDE")
GROUPS = (("Hits_Accuracy", 0), ("Velocity_MSE", 10), ("Offset_MSE", 20))


def voice_metrics(model, hvo_pred, hvo_gt):
    """-> dict of python floats: ``{Hits_Accuracy|Velocity_MSE|Offset_MSE}_{Overall|<voice>}`` (ONE 30-float D2H copy)."""
    out = model.engine.voice_metrics(hvo_pred, hvo_gt).tolist()
    res = {}
    for name, base in GROUPS:
        res[name + "_Overall"] = out[base]
        for j, v in enumerate(VOICES):
            res["%s_%s" % (name, v)] = out[base + 1 + j]
    return res


def hit_scores(model, inputs, gt_hvo, thres=0.5, voice_thresholds=None, beta=1.0):
    """Precision / recall / F-beta of the hits at the thresholds actually used (thres for every voice, or the nine voice_thresholds;
    "calibrated": the model's stored ones) -> ``Hits_{Precision|Recall|F1}_{Overall|<voice>}`` (F1: the F-beta score at `beta`, 1 by default).
    The set is predicted and counted on the device (engine.hit_curve over the grid of the sorted distinct thresholds, each voice read at
    its own index; ONE D2H copy of the counts); Overall is micro-averaged: TP, FP and FN are summed over the voices first.  A zero
    denominator gives 0.  Hit accuracy (evaluate) is dominated by the empty cells; these are not."""
    eng = model.engine
    th = eng._calibrated(voice_thresholds)
    th = [float(thres)] * len(VOICES) if th is None else [float(t) for t in th]
    if len(th) != len(VOICES):
        raise ValueError("expected %d per-voice thresholds, got %d" % (len(VOICES), len(th)))
    import numpy as np
    th32 = [float(np.float32(t)) for t in th]
    grid = sorted(set(th32))
    model.eval()
    with torch.no_grad():
        counts = eng.hit_curve(inputs, gt_hvo, grid=grid, voice_thresholds=th).cpu().numpy()
    b2 = float(beta) ** 2

    def prf(tp, fp, fn):
        f_den = (1 + b2) * tp + b2 * fn + fp
        return (tp / (tp + fp) if tp + fp else 0.0, tp / (tp + fn) if tp + fn else 0.0, (1 + b2) * tp / f_den if f_den else 0.0)

    res, tot = {}, [0, 0, 0]
    for c, v in enumerate(VOICES):
        k = grid.index(th32[c])
        tp, fp = int(counts[c, 1, k + 1:].sum()), int(counts[c, 0, k + 1:].sum())
        fn = int(counts[c, 1].sum()) - tp
        tot = [tot[0] + tp, tot[1] + fp, tot[2] + fn]
        for name, val in zip(("Precision", "Recall", "F1"), prf(tp, fp, fn)):
            res["Hits_%s_%s" % (name, v)] = val
    for name, val in zip(("Precision", "Recall", "F1"), prf(*tot)):
        res["Hits_%s_Overall" % name] = val
    return res


GM_QUANTITIES = ("Hits_Accuracy", "Hits_Precision", "Hits_Recall", "Hits_F1", "Velocity_MSE", "Offset_MSE", "Velocity_MSE_Hits",
                 "Offset_MSE_Hits")


def _div(a, b):
    return float(a) / float(b) if b else 0.0


def _gm_entry(words, sequences, rejected, b2):
    """one group's dictionary from its (9, 8) integer words (Python ints), fp64 from the integers"""
    def scores(w):
        n, tp, fp, fn = w[0], w[1], w[2], w[3]
        return (_div(n - fp - fn, n), _div(tp, tp + fp), _div(tp, tp + fn), _div((1 + b2) * tp, (1 + b2) * tp + b2 * fn + fp),
                _div(w[4] / 4294967296.0, n), _div(w[5] / 4294967296.0, n), _div(w[6] / 4294967296.0, tp), _div(w[7] / 4294967296.0, tp))
    res = {}
    total = [sum(words[c][k] for c in range(len(VOICES))) for k in range(8)]      # micro-average: the integers summed over the voices first
    for name, val in zip(GM_QUANTITIES, scores(total)):
        res[name + "_Overall"] = val
    for c, v in enumerate(VOICES):
        for name, val in zip(GM_QUANTITIES, scores(words[c])):
            res["%s_%s" % (name, v)] = val
    res["Sequences"], res["Cells"], res["Rejected_Values"] = float(sequences), float(total[0]), float(rejected)
    return res


def group_metrics_from_acc(acc, n_groups, names=None, beta=1.0):
    """The dictionaries of group_metrics from a HOST copy of gt_group_metrics' acc (any integer array-like of GT_GM_ACC_WORDS(n_groups)
    words)."""
    flat = [int(v) for v in (acc.reshape(-1).tolist() if hasattr(acc, "reshape") else acc)]
    n_groups = int(n_groups)
    if len(flat) != n_groups * (len(VOICES) * 8 + 2) + 1:
        raise ValueError("acc must hold %d words for %d groups, got %d" % (n_groups * (len(VOICES) * 8 + 2) + 1, n_groups, len(flat)))
    names = ["group%d" % k for k in range(n_groups)] if names is None else [str(s) for s in names]
    if len(names) < n_groups or len(set(names[:n_groups])) != n_groups or "Overall" in names[:n_groups] or "Skipped_Sequences" in names[:n_groups]:
        raise ValueError("names: %d distinct group names other than \"Overall\" / \"Skipped_Sequences\", got %r" % (n_groups, names))
    b2 = float(beta) ** 2
    per = [[flat[(k * len(VOICES) + c) * 8:(k * len(VOICES) + c) * 8 + 8] for c in range(len(VOICES))] for k in range(n_groups)]
    tail = n_groups * len(VOICES) * 8
    seqs, rej = [flat[tail + 2 * k] for k in range(n_groups)], [flat[tail + 2 * k + 1] for k in range(n_groups)]
    whole = [[sum(per[k][c][j] for k in range(n_groups)) for j in range(8)] for c in range(len(VOICES))]       # the integer sum, first
    res = {"Overall": _gm_entry(whole, sum(seqs), sum(rej), b2)}
    for k in range(n_groups):
        res[names[k]] = _gm_entry(per[k], seqs[k], rej[k], b2)
    res["Skipped_Sequences"] = float(flat[-1])
    return res


def group_metrics(model, hvo_pred, hvo_gt, groups=None, names=None, cells=None, removed=None, beta=1.0, n_groups=None):
    """Per-group evaluation of predictions against ground truth, both (N,32,27) HVO tensors: the reference's per-subset numbers
    (ref:evaluator.py:171-196 splits a set by genre tag), counted on the device in one pass (engine.group_metrics; ONE D2H copy of the
    integer words) -> ``{group name: {key: float}}`` plus an ``"Overall"`` entry -- the integer sum over the groups, computed first -- and
    ``"Skipped_Sequences"`` (tags outside 0..n_groups - 1).  groups: N integer tags (None: one group); names: the group names (default
    ``group<k>``); n_groups: default len(names), else the largest tag + 1.  cells / removed confine the count to a mask of cells (the bit
    words or bool mask of the event-level pairing) or of whole voices (the voice bitmasks of the voice-level pairing).
    Keys per group: ``{Hits_Accuracy, Hits_Precision, Hits_Recall, Hits_F1, Velocity_MSE, Offset_MSE, Velocity_MSE_Hits,
    Offset_MSE_Hits}_{Overall|<voice>}`` and ``Sequences``, ``Cells``, ``Rejected_Values``.  Everything is fp64 from the integers: accuracy
    (cells - FP - FN) / cells, Hits_F1 the F-beta score at `beta`, the MSEs word / 2^32 / cells, the ``_Hits`` MSEs word / 2^32 / TP (the
    error on the hits that came back); a zero denominator gives 0.  ``*_Overall`` over the voices is MICRO-averaged: the integers are summed
    over the voices first.  voice_metrics' Overall is the mean of the per-voice values instead; the two agree when every voice has the
    same number of cells (no mask)."""
    if n_groups is None and names is not None:
        n_groups = len(names)
    acc = model.engine.group_metrics(hvo_pred, hvo_gt, groups=groups, n_groups=n_groups, cells=cells, removed=removed)
    return group_metrics_from_acc(acc.cpu().numpy(), (acc.numel() - 1) // (len(VOICES) * 8 + 2), names, beta)


def evaluate_groups(model, inputs, gt_hvo, groups, names=None, **predict_kwargs):
    """evaluate per group: predict the whole set on the device (chunked), count per group on the device, return group_metrics'
    dictionaries.  predict_kwargs go to model.predict_hvo (use_thres, thres, voice_thresholds, ...)."""
    pred = model.predict_hvo(inputs, **predict_kwargs)
    return group_metrics(model, pred, torch.as_tensor(gt_hvo), groups=groups, names=names)


def rank_sequences(seq_counts, groups=None, k=4):
    """The counterpart of the evaluator's per-subset sample choice: per group the indices of the k sequences with the lowest and the k with
    the highest sequence-level F1 = 2 TP / (2 TP + FP + FN) (0 for a zero denominator), from the (N,4) per-sequence counts of
    engine.group_metrics(seq_counts=True) -- on the host, over that small copy.  Ties go to the lower index.
    -> ``{group id: {"lowest": [...], "highest": [...]}}`` (best first in "highest", worst first in "lowest"); negative tags are left out."""
    import numpy as np
    sc = (seq_counts.cpu().numpy() if torch.is_tensor(seq_counts) else np.asarray(seq_counts)).astype(np.int64).reshape(-1, 4)
    n = sc.shape[0]
    gid = np.zeros(n, np.int64) if groups is None else (groups.cpu().numpy() if torch.is_tensor(groups) else np.asarray(groups)).astype(np.int64).reshape(-1)
    if gid.shape[0] != n:
        raise ValueError("groups needs one tag per sequence (%d), got %d" % (n, gid.shape[0]))
    den = 2 * sc[:, 1] + sc[:, 2] + sc[:, 3]
    f1 = np.where(den > 0, 2.0 * sc[:, 1] / np.where(den > 0, den, 1), 0.0)
    res = {}
    for g in sorted(set(int(v) for v in gid if v >= 0)):
        idx = np.flatnonzero(gid == g)
        lo = idx[np.argsort(f1[idx], kind="stable")]                 # ascending F1; equal scores keep the index order
        hi = idx[np.argsort(-f1[idx], kind="stable")]
        res[g] = {"lowest": [int(i) for i in lo[:k]], "highest": [int(i) for i in hi[:k]]}
    return res


def evaluate(model, inputs, gt_hvo, use_thres=True, thres=0.5):
    """What the reference's ``log_eval`` does for the scalar metrics (ref:evaluator.py:516-525): predict the whole set on the
    device (chunked), reduce per voice on the device, return the dictionary."""
    pred = model.predict_hvo(inputs, use_thres=use_thres, thres=thres)
    return voice_metrics(model, pred, torch.as_tensor(gt_hvo))
