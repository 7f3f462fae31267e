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


def evaluate(model, inputs, gt_hvo, use_thres=True, thres=0.5):
    """What the reference's ``log_eval`` does for the scalar metrics (ref:evaluator.py:516-525): predict the whole set on the
    device (chunked), reduce per voice on the device, return the dictionary."""
    pred = model.predict_hvo(inputs, use_thres=use_thres, thres=thres)
    return voice_metrics(model, pred, torch.as_tensor(gt_hvo))
