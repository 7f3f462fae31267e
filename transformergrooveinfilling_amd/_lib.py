"""ctypes binding of libgroove_hip.so (C ABI declared in include/groove_hip.h; the process-wide gt_set_* switches and the
gt_debug_* aids in include/groove_hip_debug.h).

The product path has NO CPU fallback: if the HIP library is missing this module raises, it never
substitutes another implementation.  (tests/ may call ``load(path)`` with the host-emulator build
of the same sources, tests/emu/libgroove_emu.so, to debug kernels without a GPU.)
"""
import ctypes
import math
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.environ.get("GT_LIB_PATH") or os.path.join(_HERE, "lib", "libgroove_hip.so")   # GT_LIB_PATH: experiments only

GT_T = 32
GT_TGT = 27
GT_VOICES = 9


class GtConfig(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int32), ("src_dim", ctypes.c_int32), ("d_model", ctypes.c_int32),
                ("n_heads", ctypes.c_int32), ("dim_ff", ctypes.c_int32), ("n_enc_layers", ctypes.c_int32),
                ("n_dec_layers", ctypes.c_int32), ("dropout", ctypes.c_float), ("precision", ctypes.c_int32),
                ("flags", ctypes.c_int32)]


CFG_NO_QUAD = 1          # gt_config.flags (include/groove_hip.h): per-caller schedule switches
CFG_NO_LN_XCHG = 2


class GtStepState(ctypes.Structure):
    _fields_ = [("seed_lo", ctypes.c_uint32), ("seed_hi", ctypes.c_uint32), ("step", ctypes.c_uint32),
                ("opt_step", ctypes.c_uint32), ("lr", ctypes.c_float), ("grad_scale", ctypes.c_float),
                ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float),
                ("pad2", ctypes.c_float * 3)]


STEP_STATE_BYTES = ctypes.sizeof(GtStepState)   # 48


class GtOptHparams(ctypes.Structure):
    """gt_opt_hparams: host memory, read when gt_optimizer_prepare is enqueued"""
    _fields_ = [("weight_decay", ctypes.c_float), ("momentum", ctypes.c_float), ("nesterov", ctypes.c_int32),
                ("decoupled", ctypes.c_int32)]


class GtVoiceSampling(ctypes.Structure):
    """gt_voice_sampling: host memory, read when gt_predict_voices / gt_voice_select is enqueued"""
    _fields_ = [("thres", ctypes.c_float * GT_VOICES), ("max_count", ctypes.c_int32 * GT_VOICES), ("temperature", ctypes.c_float),
                ("mode", ctypes.c_int32), ("mask_vo", ctypes.c_int32)]


class GtThresholdRule(ctypes.Structure):
    """gt_threshold_rule: how gt_hit_thresholds picks a voice's threshold from its curve"""
    _fields_ = [("criterion", ctypes.c_int32), ("beta", ctypes.c_float), ("fallback", ctypes.c_float)]


CURVE_MAX_THRES = 127            # GT_CURVE_MAX_THRES
CRITERIA = {"f_beta": 0, "density": 1}

GM_MAX_GROUPS = 64               # GT_GM_MAX_GROUPS
GM_WORDS = 8                     # GT_GM_WORDS: 64-bit words per (group, voice) of gt_group_metrics' acc
GF_WORDS = 32                    # GT_GF_WORDS: 64-bit words per sequence and buffer of gt_groove_features' records
GF_PAIR_WORDS = 8                # GT_GF_PAIR_WORDS


def gm_acc_words(n_groups):
    """GT_GM_ACC_WORDS: n_groups x 9 x 8 words, then (sequences, rejected values) per group, then the skipped sequences"""
    return int(n_groups) * (GT_VOICES * GM_WORDS + 2) + 1


class GtLossOpts(ctypes.Structure):
    """gt_loss_opts: host memory, read when gt_loss_ex / gt_train_step_loss is enqueued"""
    _fields_ = [("penalty_h", ctypes.c_float), ("penalty_vo", ctypes.c_float), ("pos_weight", ctypes.c_float * GT_VOICES),
                ("voice_weight", ctypes.c_float * GT_VOICES), ("focal_gamma", ctypes.c_float), ("term_weight", ctypes.c_float * 3)]


class GtInfillOpts(ctypes.Structure):
    """gt_infill_opts: host memory, read when gt_gather_infill is enqueued"""
    _fields_ = [("voice_mask", ctypes.c_int32), ("min_remove", ctypes.c_int32), ("max_remove", ctypes.c_int32),
                ("count_weight", ctypes.c_int32 * GT_VOICES)]


class GtInfillEventOpts(ctypes.Structure):
    """gt_infill_event_opts: host memory, read when gt_gather_infill_events is enqueued"""
    _fields_ = [("voice_mask", ctypes.c_int32), ("ratio_lo", ctypes.c_int32), ("ratio_hi", ctypes.c_int32)]


_vp, _cfgp = ctypes.c_void_p, ctypes.POINTER(GtConfig)
_SIGS = {
    "gt_last_error": (ctypes.c_char_p, []),
    "gt_version": (ctypes.c_int, []),
    "gt_param_count": (ctypes.c_int, [_cfgp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "gt_param_layout": (ctypes.c_int, [_cfgp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                       ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "gt_workspace_bytes": (ctypes.c_size_t, [_cfgp]),
    "gt_ws_find": (ctypes.c_int, [_cfgp, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                                  ctypes.POINTER(ctypes.c_int64)]),
    # cfg, params, pe, x, tgt_in, hvo_out, ws, state, train, stream
    "gt_forward": (ctypes.c_int, [_cfgp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    # cfg, hvo, y, penalty, stats, d_hvo, stream
    "gt_loss": (ctypes.c_int, [_cfgp, _vp, _vp, ctypes.c_float, _vp, _vp, _vp]),
    # cfg, params, grads, x, tgt_in, hvo, d_hvo, ws, state, train, accumulate, stream
    "gt_backward": (ctypes.c_int, [_cfgp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp]),
    # algo, params, grads, m, v, n, state, zero_grads, stream
    "gt_optimizer_step": (ctypes.c_int, [ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp, ctypes.c_int, _vp]),
    # cfg, algo, params, grads, m, v, pe, x, y, penalty, hvo_out, stats, tgt_scratch, ws, state, skip_update, stream
    "gt_train_step": (ctypes.c_int, [_cfgp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_float, _vp, _vp,
                                     _vp, _vp, _vp, ctypes.c_int, _vp]),
    "gt_loss_scratch_floats": (ctypes.c_int64, [_cfgp]),
    # cfg, hvo, y, lo, stats, voice_stats, d_out, wrt_logits, scratch, stream
    "gt_loss_ex": (ctypes.c_int, [_cfgp, _vp, _vp, ctypes.POINTER(GtLossOpts), _vp, _vp, _vp, ctypes.c_int, _vp, _vp]),
    # cfg, algo, params, grads, m, v, pe, x, y, lo, voice_stats, loss_scratch, hvo_out, stats, tgt_scratch, ws, state, skip_update, stream
    "gt_train_step_loss": (ctypes.c_int, [_cfgp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(GtLossOpts), _vp, _vp, _vp,
                                          _vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    # cfg, params, pe, x, hvo_out, thres, use_thres, tgt_scratch, ws, stream
    "gt_predict": (ctypes.c_int, [_cfgp, _vp, _vp, _vp, _vp, ctypes.c_float, ctypes.c_int, _vp, _vp, _vp]),
    # cfg, params, pe, x, hvo_out, seed, tgt_scratch, ws, stream
    "gt_predict_pd": (ctypes.c_int, [_cfgp, _vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp]),
    "gt_predict_pd_at": (ctypes.c_int, [_cfgp, _vp, _vp, _vp, _vp, ctypes.c_uint32, ctypes.c_int64, _vp, _vp, _vp]),
    # cfg, params, pe, x, hvo_out, vs, seed, first_seq, prob_out, tgt_scratch, ws, stream
    "gt_predict_voices": (ctypes.c_int, [_cfgp, _vp, _vp, _vp, _vp, ctypes.POINTER(GtVoiceSampling), ctypes.c_uint32, ctypes.c_int64, _vp,
                                         _vp, _vp, _vp]),
    # hvo, prob, vs, n_seq, stream
    "gt_voice_select": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(GtVoiceSampling), ctypes.c_int64, _vp]),
    "gt_voice_metrics_scratch_floats": (ctypes.c_int64, [ctypes.c_int64]),
    # hvo_pred, hvo_gt, n_rows, out30, scratch, stream
    "gt_voice_metrics": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _vp, _vp, _vp]),
    "gt_hit_curve_scratch_words": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    # prob, prob_stride, hvo_gt, n_rows, thres (host), n_thres, counts, scratch, stream
    "gt_hit_curve": (ctypes.c_int, [_vp, ctypes.c_int32, _vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_float), ctypes.c_int32, _vp, _vp, _vp]),
    # counts_host, thres, n_thres, rule, thres_out, index_out, scores_out -- all host memory
    "gt_hit_thresholds": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_float), ctypes.c_int32,
                                         ctypes.POINTER(GtThresholdRule), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32),
                                         ctypes.POINTER(ctypes.c_float)]),
    "gt_group_metrics_scratch_words": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    # hvo_pred, hvo_gt, group, cells, n_seq, n_groups, acc, seq_out, scratch, stream
    "gt_group_metrics": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int32, _vp, _vp, _vp, _vp]),
    # hvo_a, hvo_b, n_seq, feat_a, feat_b, pair, stream
    "gt_groove_features": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp]),
    # xs, ys, idx, n_seq, batch, src_dim, x, y, stream
    "gt_gather_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp]),
    # hvo_set, idx, n_seq, batch, io, state, x, y, removed, stream
    "gt_gather_infill": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(GtInfillOpts), _vp, _vp, _vp, _vp, _vp]),
    # hvo_pred, hvo_in, removed, n_seq, mode, hvo_out, stream
    "gt_infill_merge": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int32, _vp, _vp]),
    # hvo_set, idx, n_seq, batch, eo, state, x, y, cells, stream
    "gt_gather_infill_events": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(GtInfillEventOpts), _vp, _vp, _vp, _vp,
                                               _vp]),
    # hvo_pred, hvo_in, cells, n_seq, mode, hvo_out, stream
    "gt_infill_merge_cells": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int32, _vp, _vp]),
    # cfg, algo, params, grads, m, v, ws, state, zero_grads, stream
    "gt_optimizer_step_ws": (ctypes.c_int, [_cfgp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "gt_grad_buckets": (ctypes.c_int, [_cfgp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "gt_profile_enable": (ctypes.c_int, [ctypes.c_int]),
    "gt_set_seq": (ctypes.c_int, [ctypes.c_int]),
    "gt_set_seq_split": (ctypes.c_int, [ctypes.c_int]),
    "gt_set_seq_quad": (ctypes.c_int, [ctypes.c_int]),
    "gt_set_xchg_spin_max": (ctypes.c_int, [ctypes.c_int]),
    "gt_dp_guard": (ctypes.c_int, [_cfgp, _vp, _vp, _vp]),
    "gt_clip_grad_norm_scratch_floats": (ctypes.c_int64, [_cfgp]),
    # cfg, grads, state, max_norm, out, scratch, stream
    "gt_clip_grad_norm": (ctypes.c_int, [_cfgp, _vp, _vp, ctypes.c_float, _vp, _vp, _vp]),
    # cfg, algo, params, grads, mbuf, ws, state, hp, stream
    "gt_optimizer_prepare": (ctypes.c_int, [_cfgp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(GtOptHparams), _vp]),
    "gt_set_ln_exchange": (ctypes.c_int, [ctypes.c_int]),
    "gt_debug_occupy_cus": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _vp]),
    "gt_set_operand_shadows": (ctypes.c_int, [ctypes.c_int]),
    "gt_layout_epoch": (ctypes.c_int, []),
    "gt_operand_shadow_level": (ctypes.c_int, [_cfgp]),
    "gt_precision_in_force": (ctypes.c_int, [_cfgp]),
    "gt_workspace_init": (ctypes.c_int, [_cfgp, _vp, _vp]),
    "gt_set_seq_ride": (ctypes.c_int, [ctypes.c_int]),
    "gt_set_deterministic": (ctypes.c_int, [ctypes.c_int]),
    # cfg, params, grads, x, ws, phase, ksplit, stream
    "gt_debug_seq_wg_phase": (ctypes.c_int, [_cfgp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp]),
    "gt_step_launches": (ctypes.c_int, [ctypes.POINTER(GtConfig)]),
    "gt_profile_report": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]),
}
EXPORTS = tuple(_SIGS)


class GrooveLibError(RuntimeError):
    pass


class GrooveLib:
    """Thin checked wrapper: every entry point raises GrooveLibError(gt_last_error()) on failure."""

    def __init__(self, path=None):
        path = path or DEFAULT_LIB
        if not os.path.exists(path):
            raise GrooveLibError(
                "HIP library %s not found. Build it with transformergrooveinfilling_amd/csrc/build.sh "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback." % path)
        self.path = path
        self.cdll = ctypes.CDLL(path)
        for name, (res, args) in _SIGS.items():
            fn = getattr(self.cdll, name)      # AttributeError if the library lacks a declared symbol
            fn.restype, fn.argtypes = res, args

    def _chk(self, rc, what):
        if rc != 0:
            raise GrooveLibError("%s failed: %s" % (what, self.cdll.gt_last_error().decode()))

    def call(self, name, *args):
        self._chk(getattr(self.cdll, name)(*args), name)

    def param_layout(self, cfg):
        """-> (total_floats, [(offset, size, rows, cols)]) in state-dict order."""
        nt, nf = ctypes.c_int64(), ctypes.c_int64()
        self.call("gt_param_count", ctypes.byref(cfg), ctypes.byref(nt), ctypes.byref(nf))
        n = nt.value
        off, siz = (ctypes.c_int64 * n)(), (ctypes.c_int64 * n)()
        rows, cols = (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)()
        self.call("gt_param_layout", ctypes.byref(cfg), off, siz, rows, cols)
        return nf.value, [(off[i], siz[i], rows[i], cols[i]) for i in range(n)]

    def workspace_floats(self, cfg):
        b = self.cdll.gt_workspace_bytes(ctypes.byref(cfg))
        if b == 0:
            raise GrooveLibError("gt_workspace_bytes failed: %s" % self.cdll.gt_last_error().decode())
        return b // 4

    def grad_buckets(self, cfg):
        """-> [(offset, count)] of the flat gradient buffer in the order backward completes them (1 or 2 buckets)."""
        off, cnt = (ctypes.c_int64 * 2)(), (ctypes.c_int64 * 2)()
        n = self.cdll.gt_grad_buckets(ctypes.byref(cfg), off, cnt)
        if n < 1:
            raise GrooveLibError("gt_grad_buckets failed: %s" % self.cdll.gt_last_error().decode())
        return [(off[i], cnt[i]) for i in range(n)]

    def hit_thresholds(self, counts, grid, criterion=0, beta=1.0, fallback=0.5):
        """gt_hit_thresholds on a HOST copy of gt_hit_curve's counts ((9, 2, K + 1) integers, any array-like) over `grid` (K floats)
        -> (thresholds [9], index [9], scores [9][4] = precision, recall, F-beta, density ratio)."""
        grid = [float(t) for t in grid]
        k = len(grid)
        flat = [int(v) for v in (counts.reshape(-1).tolist() if hasattr(counts, "reshape") else counts)]
        if len(flat) != GT_VOICES * 2 * (k + 1):
            raise ValueError("counts must hold 9 x 2 x %d integers, got %d" % (k + 1, len(flat)))
        cnt = (ctypes.c_uint64 * len(flat))(*flat)
        rule = GtThresholdRule(int(criterion), float(beta), float(fallback))
        th, idx, sc = (ctypes.c_float * GT_VOICES)(), (ctypes.c_int32 * GT_VOICES)(), (ctypes.c_float * (4 * GT_VOICES))()
        self.call("gt_hit_thresholds", cnt, (ctypes.c_float * max(k, 1))(*grid), k, ctypes.byref(rule), th, idx, sc)
        return list(th), list(idx), [list(sc[4 * c:4 * c + 4]) for c in range(GT_VOICES)]

    def ws_find(self, cfg, name, layer=0):
        o, c = ctypes.c_int64(), ctypes.c_int64()
        self.call("gt_ws_find", ctypes.byref(cfg), name.encode(), layer, ctypes.byref(o), ctypes.byref(c))
        return o.value, c.value


_default = None


def get_lib():
    """The process-wide HIP library (loaded on first use; raises if it is not built)."""
    global _default
    if _default is None:
        _default = GrooveLib()
    return _default


# 0 fp32 | 1 bf16 GEMM operands | 2 ... and bf16 storage of the Linear outputs ("autocast": what torch.autocast(bfloat16) keeps in bf16)
PRECISION = {"fp32": 0, "f32": 0, "float32": 0, 0: 0, None: 0, "bf16": 1, "bfloat16": 1, 1: 1, "bf16_storage": 2, "bf16s": 2, "autocast": 2, 2: 2}


def make_voice_sampling(thres=0.5, max_count=32, temperature=1.0, mode=0, mask_vo=False):
    """gt_voice_sampling from scalars (broadcast over the 9 voices) or sequences of 9"""
    def nine(v, conv):
        v = [conv(v)] * GT_VOICES if not hasattr(v, "__len__") else [conv(a) for a in v]
        if len(v) != GT_VOICES:
            raise ValueError("expected %d per-voice values, got %d" % (GT_VOICES, len(v)))
        return v
    return GtVoiceSampling((ctypes.c_float * GT_VOICES)(*nine(thres, float)), (ctypes.c_int32 * GT_VOICES)(*nine(max_count, int)),
                           float(temperature), int(mode), int(bool(mask_vo)))


def make_loss_opts(penalty_h=1.0, penalty_vo=None, pos_weight=1.0, voice_weight=1.0, focal_gamma=0.0, term_weight=(1.0, 1.0, 1.0)):
    """gt_loss_opts from scalars (pos_weight / voice_weight: broadcast over the 9 voices) or sequences of 9; penalty_vo None = penalty_h.
    ValueError for a wrong length or a value the library would refuse (include/groove_hip.h), before the library is called."""
    def many(v, n, what):
        if torch_like(v):
            v = v.detach().reshape(-1).tolist()
        v = [float(v)] * n if not hasattr(v, "__len__") else [float(a) for a in v]
        if len(v) == 1:
            v = v * n
        if len(v) != n:
            raise ValueError("%s: expected 1 or %d values, got %d" % (what, n, len(v)))
        return v
    finite = lambda a: a == a and abs(a) != float("inf")
    ph = float(penalty_h)
    pvo = ph if penalty_vo is None else float(penalty_vo)
    pw, vw, tw = many(pos_weight, GT_VOICES, "pos_weight"), many(voice_weight, GT_VOICES, "voice_weight"), many(term_weight, 3, "term_weight")
    g = float(focal_gamma)
    if not all(finite(a) and a >= 0.0 for a in [ph, pvo] + vw + tw):
        raise ValueError("penalties, voice_weight and term_weight must be >= 0 and finite: %r" % (([ph, pvo], vw, tw),))
    if not all(finite(a) and a > 0.0 for a in pw):
        raise ValueError("pos_weight must be > 0 and finite: %r" % (pw,))
    if not 0.0 <= g <= 8.0:
        raise ValueError("focal_gamma must lie in [0, 8], got %r" % (focal_gamma,))
    return GtLossOpts(ph, pvo, (ctypes.c_float * GT_VOICES)(*pw), (ctypes.c_float * GT_VOICES)(*vw), g, (ctypes.c_float * 3)(*tw))


def _infill_struct(mask, lo, hi, w):
    """the validated GtInfillOpts of (voice_mask, min_remove, max_remove, weights of the sizes min_remove..max_remove); ValueError for what
    the library would refuse (include/groove_hip.h)"""
    if not 0 < mask < (1 << GT_VOICES):
        raise ValueError("infill voices must be a non-empty subset of 0..%d (mask 0x%x)" % (GT_VOICES - 1, mask))
    if not 1 <= lo <= hi <= GT_VOICES:
        raise ValueError("need 1 <= min_remove <= max_remove <= %d, got %d / %d" % (GT_VOICES, lo, hi))
    if len(w) != hi - lo + 1:
        raise ValueError("infill prob needs one weight per size %d..%d, got %d" % (lo, hi, len(w)))
    if any(not 0 <= a <= 1024 for a in w) or not any(w):
        raise ValueError("infill prob: integer weights in 0..1024, not all zero, got %r" % (w,))
    return GtInfillOpts(mask, lo, hi, (ctypes.c_int32 * GT_VOICES)(*(list(w) + [0] * (GT_VOICES - len(w)))))


def make_infill_opts(voices=(2,), min_remove=1, max_remove=None, prob=None):
    """gt_infill_opts from the reference's voices_params (ref:utils.py:69-115): voices = "voice_idx" (the voices that may be removed),
    min_remove / max_remove = "min_n_voices_to_remove" / "max_n_voices_to_remove" (default: min_remove), prob = the integer weight of each
    combination of size min_remove, min_remove + 1, ... (default: all 1).  ValueError for what the library would refuse."""
    voices = [int(v) for v in ([voices] if not hasattr(voices, "__len__") else voices)]
    if any(not 0 <= v < GT_VOICES for v in voices):
        raise ValueError("infill voices must be a non-empty subset of 0..%d, got %r" % (GT_VOICES - 1, voices))
    lo = int(min_remove)
    hi = lo if max_remove is None else int(max_remove)
    w = [1] * max(0, hi - lo + 1) if prob is None else list([prob] if not hasattr(prob, "__len__") else prob)
    if any(float(a) != int(a) for a in w):
        raise ValueError("infill prob must be integer weights, got %r" % (prob,))
    return _infill_struct(sum(1 << v for v in set(voices)), lo, hi, [int(a) for a in w])


def infill_opts_tuple(io):
    """the hashable form of a GtInfillOpts (StepEngine.infill_opts; part of a captured graph's key): its 12 integers in field order"""
    return (io.voice_mask, io.min_remove, io.max_remove) + tuple(io.count_weight)


def infill_opts_struct(t):
    """the validated GtInfillOpts of such a tuple (weights past max_remove - min_remove are ignored, as by the library)"""
    if not isinstance(t, tuple) or len(t) != 12 or any(int(a) != a for a in t):
        raise ValueError("infill options must be the 12-integer tuple infill_opts_tuple() returns, got %r" % (t,))
    return _infill_struct(int(t[0]), int(t[1]), int(t[2]), [int(a) for a in t[3:3 + max(0, int(t[2]) - int(t[1]) + 1)]])


RATIO_ONE = 65536      # gt_infill_event_opts: ratios are integers in 1/65536ths


def _infill_event_struct(mask, lo, hi):
    """the validated GtInfillEventOpts of (voice_mask, ratio_lo, ratio_hi); ValueError for what the library would refuse"""
    if not 0 < mask < (1 << GT_VOICES):
        raise ValueError("infill voices must be a non-empty subset of 0..%d (mask 0x%x)" % (GT_VOICES - 1, mask))
    if not 0 <= lo <= hi <= RATIO_ONE:
        raise ValueError("need 0 <= ratio_lo <= ratio_hi <= %d (1/65536ths), got %d / %d" % (RATIO_ONE, lo, hi))
    return GtInfillEventOpts(mask, lo, hi)


def make_infill_event_opts(voices=range(GT_VOICES), ratio=(0.4, 0.6)):
    """gt_infill_event_opts: voices = the voices whose hits may be removed (default: all nine), ratio = (lo, hi), the share of the candidate
    hits to remove, drawn per groove and visit (the reference's remove_random_events(thres_range=(0.4, 0.6)), ref:dataset.py:464-555); each
    float becomes int(round(r * 65536)).  ValueError for what the library would refuse."""
    voices = [int(v) for v in ([voices] if not hasattr(voices, "__len__") else voices)]
    if any(not 0 <= v < GT_VOICES for v in voices):
        raise ValueError("infill voices must be a non-empty subset of 0..%d, got %r" % (GT_VOICES - 1, voices))
    ratio = [ratio, ratio] if not hasattr(ratio, "__len__") else list(ratio)
    if len(ratio) != 2 or any(not math.isfinite(float(r)) for r in ratio):
        raise ValueError("infill ratio must be two finite numbers (lo, hi), got %r" % (ratio,))
    lo, hi = (int(round(float(r) * RATIO_ONE)) for r in ratio)
    return _infill_event_struct(sum(1 << v for v in set(voices)), lo, hi)


def infill_event_opts_tuple(eo):
    """the hashable form of a GtInfillEventOpts (StepEngine.infill_event_opts; part of a captured graph's key): ("events", voice_mask,
    ratio_lo, ratio_hi) -- the tag keeps it apart from the 12-integer tuple of the voice options"""
    return ("events", eo.voice_mask, eo.ratio_lo, eo.ratio_hi)


def is_infill_event_tuple(t):
    return isinstance(t, tuple) and len(t) == 4 and t[0] == "events"


def infill_event_opts_struct(t):
    """the validated GtInfillEventOpts of such a tuple"""
    if not is_infill_event_tuple(t) or any(not isinstance(a, int) or isinstance(a, bool) for a in t[1:]):
        raise ValueError("event infill options must be the tuple infill_event_opts_tuple() returns, got %r" % (t,))
    return _infill_event_struct(t[1], t[2], t[3])


def torch_like(v):
    return hasattr(v, "detach") and hasattr(v, "reshape")


def loss_opts_tuple(lo):
    """the hashable form of a GtLossOpts (StepEngine.loss_opts; part of a captured graph's key): its 24 floats in field order"""
    return (lo.penalty_h, lo.penalty_vo) + tuple(lo.pos_weight) + tuple(lo.voice_weight) + (lo.focal_gamma,) + tuple(lo.term_weight)


def loss_opts_struct(t):
    return GtLossOpts(t[0], t[1], (ctypes.c_float * GT_VOICES)(*t[2:11]), (ctypes.c_float * GT_VOICES)(*t[11:20]), t[20], (ctypes.c_float * 3)(*t[21:24]))


def make_config(batch, src_dim, d_model, n_heads, dim_ff, n_enc_layers, n_dec_layers=0, dropout=0.0, precision=0, flags=0):
    return GtConfig(int(batch), int(src_dim), int(d_model), int(n_heads), int(dim_ff), int(n_enc_layers),
                    int(n_dec_layers), float(dropout), PRECISION[precision], int(flags))
