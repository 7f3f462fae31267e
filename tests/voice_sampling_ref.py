"""numpy restatement of gt_predict_voices' decision and of the cap / mask pass (gt_voice_select; include/groove_hip.h), for the tests."""
import numpy as np

NV = 9


def decide(prob, thres, u=None):
    """hits (float32 0 / 1) of fp32 probabilities (..., 9): p > thres[voice], in the sampled mode also p > u"""
    p = np.asarray(prob, np.float32)
    h = p > np.asarray(thres, np.float32)
    if u is not None:
        h &= p > np.asarray(u, np.float32)
    return h.astype(np.float32)


def select(hvo, prob, max_count, mask_vo=False):
    """hvo (n,32,27), prob (n,32,9) -> hvo after the pass.  Per (sequence, voice): a hit step t stays iff fewer than max_count other hit
    steps t' have p[t'] > p[t], or p[t'] == p[t] with t' < t; with mask_vo velocity and offset are 0 wherever the final hit is 0."""
    hvo = np.array(hvo, np.float32, copy=True)
    p = np.asarray(prob, np.float32)
    n = hvo.shape[0]
    assert hvo.shape == (n, 32, 27) and p.shape == (n, 32, NV)
    cand = hvo[..., :NV] != 0                                                    # (n, t, c)
    step = np.arange(32)
    # axes (n, t, t', c): is t' ahead of t
    first = (p[:, None, :, :] > p[:, :, None, :]) | ((p[:, None, :, :] == p[:, :, None, :]) & (step[None, None, :, None] < step[None, :, None, None]))
    ahead = (first & cand[:, None, :, :]).sum(2)
    keep = cand & (ahead < np.asarray(max_count).reshape(1, 1, NV))
    hvo[..., :NV] = np.where(keep, hvo[..., :NV], np.float32(0))
    if mask_vo:
        on = hvo[..., :NV] != 0
        hvo[..., NV:2 * NV] = np.where(on, hvo[..., NV:2 * NV], np.float32(0))
        hvo[..., 2 * NV:] = np.where(on, hvo[..., 2 * NV:], np.float32(0))
    return hvo


def over_cap_groups(hvo, max_count):
    """(groups with more hits than their cap, all groups) of an uncapped (n,32,27) result"""
    cnt = (np.asarray(hvo)[..., :NV] != 0).sum(1)                                # (n, c)
    return int((cnt > np.asarray(max_count).reshape(1, NV)).sum()), int(cnt.size)
