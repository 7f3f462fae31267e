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


# ---- groove descriptors and rhythmic distances (gt_groove_features) -------------------------------------------------------------------------
# The second leg of the reference's log_eval (ref:evaluator.py:516-601): on the "all" epochs it writes get_stats_from_evaluator's table of
# rhythmic descriptors -- mean, std, min, max, median and quartiles, __Ground_Truth beside __Prediction -- and keeps a commented call to
# get_rhythmic_distances.  The GrooveEvaluator that defines those descriptors is un-vendored, so the definitions below are THIS PACKAGE'S
# OWN, named after the reference's columns where a counterpart exists (as the keys above are).  The device yields integers per sequence
# (engine.groove_features); everything here is fp64 from a host copy of them, and a quantity whose denominator is zero is 0.
DESCRIPTORS = ("Statistical::NoI", "Statistical::Total Step Density", "Statistical::Avg Voice Density", "Statistical::Weak to Strong Ratio",
               "Statistical::Symmetry", "Statistical::Poly Velocity Mean", "Statistical::Poly Velocity std", "Statistical::Poly Offset Mean",
               "Statistical::Poly Offset std", "Micro-Timing::Accuracy", "Auto-Correlation::Max", "Auto-Correlation::Centroid",
               "Auto-Correlation::Skewness", "Auto-Correlation::Beat", "Auto-Correlation::Bar")
DISTANCES = ("Hamming", "Fuzzy Hamming", "Jaccard", "Velocity L2", "Offset RMS", "Profile Cosine")
TABLE_STATS = ("mean", "std", "min", "max", "median", "q1", "q3")
_FIX = 4294967296.0


def _words(t, width):
    import numpy as np
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    if a.ndim != 2 or a.shape[1] != width or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("expected an (N,%d) integer array, got %s of %s" % (width, a.shape, a.dtype))
    return a.astype(np.int64).astype(np.float64)                   # (every word is below 2^53: exact)


def _ratio(num, den):
    import numpy as np
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape, np.float64), where=den != 0)


def groove_descriptors(feat):
    """Rhythmic descriptors per sequence from the (N,32) records of engine.groove_features -> ``{name: (N,) float64}`` over DESCRIPTORS.
    This package's own definitions (the reference's GrooveEvaluator is un-vendored), named after the reference's table columns.  With w<k>
    word k of the record, nv = hits - rejected velocities, no = hits - rejected offsets, a[l] = A[l] / A[0] the normalised circular
    autocorrelation of the velocity profile:
    NoI = voices with a hit; Total Step Density = steps with a hit / 32; Avg Voice Density = hits / (32 * voices); Weak to Strong Ratio =
    hits at odd steps / hits at even steps; Symmetry = 2 * (cells hit in both halves of the bar) / hits; Poly Velocity Mean / std and Poly
    Offset Mean / std over the hits with a valid value (std = sqrt(max(0, E[x^2] - mean^2))); Micro-Timing::Accuracy = the mean |offset|;
    Auto-Correlation::Max = the largest a[l], l = 1..16; Centroid = sum l a[l] / sum a[l] and Skewness = the third standardised moment of
    the lag under the weights a[l] / sum a, both over l = 1..16; Beat = a[4]; Bar = a[16].  A zero denominator gives 0."""
    import numpy as np
    w = _words(feat, 32)
    hits, nv, no = w[:, 0], w[:, 0] - w[:, 7], w[:, 0] - w[:, 8]
    vmean, omean = _ratio(w[:, 9] / _FIX, nv), _ratio(w[:, 12] / _FIX, no)
    a = _ratio(w[:, 15:32], w[:, 15:16])                            # (N,17): a[0] = 1 wherever the profile is not empty
    lag = np.arange(1, 17, dtype=np.float64)
    tot = a[:, 1:].sum(1)
    p = _ratio(a[:, 1:], tot[:, None])
    cen = (p * lag).sum(1)
    var = (p * (lag - cen[:, None]) ** 2).sum(1)
    m3 = (p * (lag - cen[:, None]) ** 3).sum(1)
    vals = (w[:, 1], w[:, 2] / 32.0, _ratio(hits, 32.0 * w[:, 1]), _ratio(w[:, 5], w[:, 3] + w[:, 4]), _ratio(2.0 * w[:, 6], hits),
            vmean, np.sqrt(np.maximum(0.0, _ratio(w[:, 10] / _FIX, nv) - vmean ** 2)),
            omean, np.sqrt(np.maximum(0.0, _ratio(w[:, 13] / _FIX, no) - omean ** 2)),
            _ratio(w[:, 11] / _FIX, no), a[:, 1:].max(1), cen, _ratio(m3, var ** 1.5), a[:, 4], a[:, 16])
    return dict(zip(DESCRIPTORS, vals))


def groove_distances(feat_a, feat_b, pair):
    """Rhythmic distances per sequence of grooves a from grooves b, from the records and pair words of engine.groove_features ->
    ``{name: (N,) float64}`` over DISTANCES (this package's own definitions): Hamming = cells whose hits differ; Fuzzy Hamming = Hamming -
    near misses / 2 (a hit one step beside its target counts half); Jaccard = 1 - |both| / |either|; Velocity L2 = the 2-norm of the
    velocity difference over all cells (0 where there is no hit); Offset RMS over the cells hit in both; Profile Cosine = 1 - the cosine of
    the two velocity profiles.  A zero denominator gives 0."""
    import numpy as np
    fa, fb, p = _words(feat_a, 32), _words(feat_b, 32), _words(pair, 8)
    union = p[:, 0] + p[:, 1]
    norm = np.sqrt(fa[:, 15] * fb[:, 15])
    vals = (p[:, 0], p[:, 0] - p[:, 2] / 2.0, np.where(union != 0, 1.0 - _ratio(p[:, 1], union), 0.0), np.sqrt(p[:, 3] / _FIX),
            np.sqrt(_ratio(p[:, 4] / _FIX, p[:, 5])), np.where(norm != 0, 1.0 - _ratio(p[:, 6], norm), 0.0))
    return dict(zip(DISTANCES, vals))


def _table_stats(x):
    import numpy as np
    if x.size == 0:
        return {k: 0.0 for k in TABLE_STATS}
    q1, med, q3 = np.percentile(x, [25, 50, 75])
    return {"mean": float(x.mean()), "std": float(x.std()), "min": float(x.min()), "max": float(x.max()), "median": float(med),
            "q1": float(q1), "q3": float(q3)}


def descriptor_table(desc_gt, desc_pred, dist=None, groups=None, names=None):
    """The reference's descriptor table (get_stats_from_evaluator) from per-sequence descriptors -> ``{"Overall" | group name: {column:
    ...}}``.  Columns: ``<name>__Ground_Truth`` and ``<name>__Prediction`` (and ``Distance::<name>`` for every entry of dist) hold
    ``{mean, std, min, max, median, q1, q3}`` of the sample (std of the population; numpy.percentile in its linear default);
    ``<name>__W1`` is one float, the mean absolute difference of the two sorted samples -- the 1-Wasserstein distance of the two empirical
    distributions, which have the same N.  groups: N integer tags (a tag outside 0..n_groups - 1 is in "Overall" only); names: the group
    names (default ``group<k>``, n_groups = the largest tag + 1).  An empty group holds zeros."""
    import numpy as np
    if set(desc_gt) != set(desc_pred):
        raise ValueError("desc_gt and desc_pred must hold the same descriptors")
    cols = {k: (np.asarray(desc_gt[k], np.float64).reshape(-1), np.asarray(desc_pred[k], np.float64).reshape(-1)) for k in desc_gt}
    dist = {} if dist is None else {k: np.asarray(v, np.float64).reshape(-1) for k, v in dist.items()}
    sizes = {len(v) for pr in cols.values() for v in pr} | {len(v) for v in dist.values()}
    if len(sizes) != 1:
        raise ValueError("every sample must hold one value per sequence, got sizes %s" % sorted(sizes))
    n = sizes.pop()
    sel = [("Overall", np.ones(n, bool))]
    if groups is not None:
        gid = (groups.cpu().numpy() if torch.is_tensor(groups) else np.asarray(groups)).astype(np.int64).reshape(-1)
        if gid.shape[0] != n:
            raise ValueError("groups needs one tag per sequence (%d), got %d" % (n, gid.shape[0]))
        n_groups = len(names) if names is not None else max(1, int(gid.max()) + 1)
        names = ["group%d" % k for k in range(n_groups)] if names is None else [str(s) for s in names]
        if len(set(names)) != n_groups or "Overall" in names:
            raise ValueError("names: distinct group names other than \"Overall\", got %r" % (names,))
        sel += [(names[k], gid == k) for k in range(n_groups)]
    res = {}
    for gname, m in sel:
        tab = {}
        for k, (g, p) in cols.items():
            tab[k + "__Ground_Truth"], tab[k + "__Prediction"] = _table_stats(g[m]), _table_stats(p[m])
            tab[k + "__W1"] = float(np.abs(np.sort(g[m]) - np.sort(p[m])).mean()) if m.any() else 0.0
        for k, v in dist.items():
            tab["Distance::" + k] = _table_stats(v[m])
        res[gname] = tab
    return res


def groove_table(model, hvo_pred, hvo_gt, groups=None, names=None, gt_feat=None):
    """descriptor_table of predictions (N,32,27) beside their ground truth, with the distances of each prediction from its target: ONE
    engine.groove_features call, ONE D2H copy of the integer records.  gt_feat: the ground truth's (N,32) records from an earlier call
    (they stay on the device; the call then computes the predictions' records and the pair words only)."""
    eng = model.engine
    if gt_feat is None:
        fa, fb, pw = eng.groove_features(hvo_pred, hvo_gt)
    else:
        fa, pw = eng.groove_features(hvo_pred, hvo_gt, feat_b=False)
        fb = torch.as_tensor(gt_feat).to(fa.device)
    host = torch.cat([fa, fb, pw], 1).cpu().numpy()
    fa, fb, pw = host[:, :32], host[:, 32:64], host[:, 64:]
    return descriptor_table(groove_descriptors(fb), groove_descriptors(fa), groove_distances(fa, fb, pw), groups=groups, names=names)


def evaluate_descriptors(model, inputs, gt_hvo, groups=None, names=None, gt_feat=None, **predict_kwargs):
    """The descriptor leg of the evaluation: predict the whole set on the device (chunked), one gt_groove_features call, one D2H copy of the
    records, then descriptor_table.  predict_kwargs go to model.predict_hvo (use_thres, thres, voice_thresholds, ...)."""
    pred = model.predict_hvo(inputs, **predict_kwargs)
    return groove_table(model, pred, torch.as_tensor(gt_hvo), groups=groups, names=names, gt_feat=gt_feat)
