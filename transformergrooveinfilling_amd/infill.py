"""Infilling pairs from full grooves: the host side of gt_gather_infill / gt_infill_merge (include/groove_hip.h).

The reference pairs its symbolic infilling data at preprocessing time (GrooveMidiDatasetInfillingSymbolic, ref:dataset.py:380-459: a few
frozen voice combinations per groove, ref:utils.py:69-115, through the un-vendored hvo_sequence package).  Here the resident set is ONE
tensor of full grooves (N,32,27) and the removal is drawn inside the step's gather launch; what stays on the host is deciding which
grooves can be paired at all (`infill_eligible`: the kernel's rule in the same integer arithmetic), pairing an evaluation subset once
with a fixed state (`pair_once`), and putting a prediction back into its input (`merge`).

The event-level pairing (GrooveMidiDatasetInfillingRandom, ref:dataset.py:464-555: remove_random_events takes a random share of the
individual hits out of a groove) has the same three host pieces over gt_gather_infill_events / gt_infill_merge_cells: `events_eligible`,
`pair_once_events` / `gather_events`, and `merge(..., cells=...)`.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

_BINOM = [[math.comb(n, k) for k in range(10)] for n in range(10)]


def as_opts(opts):
    """GtInfillOpts from a GtInfillOpts, the 12-integer tuple of _lib.infill_opts_tuple, or make_infill_opts keywords in a dict; the event
    options likewise -> GtInfillEventOpts: the struct, the tuple of _lib.infill_event_opts_tuple, or a dict with mode="events" beside
    make_infill_event_opts keywords (mode="voices" in a dict names the voice options, as no mode does)"""
    if isinstance(opts, (_lib.GtInfillOpts, _lib.GtInfillEventOpts)):
        return opts
    if isinstance(opts, dict):
        mode = opts.get("mode", "voices")
        if mode not in ("voices", "events"):
            raise ValueError("infill options: mode must be \"voices\" or \"events\", got %r" % (mode,))
        kw = {k: v for k, v in opts.items() if k != "mode"}
        return _lib.make_infill_event_opts(**kw) if mode == "events" else _lib.make_infill_opts(**kw)
    if _lib.is_infill_event_tuple(opts):
        return _lib.infill_event_opts_struct(opts)
    if isinstance(opts, tuple) and len(opts) == 12:
        return _lib.infill_opts_struct(opts)
    raise ValueError("infill options: a GtInfillOpts / GtInfillEventOpts, the tuple of infill_opts_tuple() / infill_event_opts_tuple() or a dict of "
                     "make_infill_opts / make_infill_event_opts keywords, got %r" % (opts,))


def infill_eligible(hvo, opts):
    """int64 indices (on hvo's device) of the grooves gt_gather_infill can pair: T > 0 in the header's terms -- at least one removable size k
    in min_remove..min(max_remove, n_act, n_tot - 1) has a non-zero weight.  hvo: (N,32,27) full grooves."""
    io = as_opts(opts)
    if is_events(io):
        raise ValueError("infill_eligible takes the voice options; event options go to events_eligible")
    hvo = torch.as_tensor(hvo)
    if hvo.dim() != 3 or hvo.shape[1:] != (32, 27):
        raise ValueError("hvo must be (N, 32, 27) full grooves, got %s" % (tuple(hvo.shape),))
    active = (hvo[:, :, :_lib.GT_VOICES] != 0).any(1)                                             # (N,9)
    cand = torch.tensor([(io.voice_mask >> c) & 1 for c in range(_lib.GT_VOICES)], dtype=torch.bool, device=hvo.device)
    n_tot, n_act = active.sum(1), (active & cand).sum(1)
    hi = torch.minimum(torch.minimum(n_act, n_tot - 1), torch.full_like(n_act, io.max_remove))
    binom = torch.tensor(_BINOM, dtype=torch.int64, device=hvo.device)
    T = torch.zeros_like(n_act)
    for k in range(io.min_remove, io.max_remove + 1):
        T += (k <= hi) * (int(io.count_weight[k - io.min_remove]) * binom[n_act, k])
    return torch.nonzero(T > 0).reshape(-1)


def is_events(opts):
    """do these (as_opts-normalised) options select the event-level pairing?"""
    return isinstance(opts, _lib.GtInfillEventOpts)


def opts_tuple(opts):
    """the hashable form of either options struct (StepEngine.infill_opts / infill_event_opts)"""
    return _lib.infill_event_opts_tuple(opts) if is_events(opts) else _lib.infill_opts_tuple(opts)


def events_eligible(hvo, opts):
    """int64 indices (on hvo's device) of the grooves gt_gather_infill_events can pair: cap = min(n_cand, n_ev - 1) >= 1 in the header's
    terms -- at least one hit in a voice of voice_mask, and at least two hits in all.  hvo: (N,32,27) full grooves."""
    eo = as_opts(opts)
    if not is_events(eo):
        raise ValueError("events_eligible takes the event options; voice options go to infill_eligible")
    hvo = torch.as_tensor(hvo)
    if hvo.dim() != 3 or hvo.shape[1:] != (32, 27):
        raise ValueError("hvo must be (N, 32, 27) full grooves, got %s" % (tuple(hvo.shape),))
    event = hvo[:, :, :_lib.GT_VOICES] != 0                                                        # (N,32,9)
    cand = torch.tensor([(eo.voice_mask >> c) & 1 for c in range(_lib.GT_VOICES)], dtype=torch.bool, device=hvo.device)
    n_ev, n_cand = event.sum((1, 2)), (event & cand).sum((1, 2))
    return torch.nonzero(torch.minimum(n_cand, n_ev - 1) >= 1).reshape(-1)


def eligible(hvo, opts):
    """infill_eligible or events_eligible, whichever the options select"""
    io = as_opts(opts)
    return events_eligible(hvo, io) if is_events(io) else infill_eligible(hvo, io)


def make_state(seed, step=0, device="cuda"):
    """a 48-byte device gt_step_state that carries a seed and a step only (what gt_gather_infill reads)"""
    st = _lib.GtStepState(int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF, 0, 0.0, 1.0, 0.9, 0.999, 1e-8)
    return torch.from_numpy(np.frombuffer(bytes(st), dtype=np.uint8).copy()).to(device)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else 0)


def check_set(hvo_set):
    """the kernel reads dense fp32 (N,32,27) memory with 16-byte loads: anything else would be read wrongly, silently"""
    if (not torch.is_tensor(hvo_set) or hvo_set.dim() != 3 or tuple(hvo_set.shape[1:]) != (32, _lib.GT_TGT) or hvo_set.dtype != torch.float32
            or not hvo_set.is_contiguous()):
        raise ValueError("hvo_set must be a contiguous fp32 (N, 32, 27) tensor of full grooves, got %s"
                         % ((tuple(hvo_set.shape), hvo_set.dtype) if torch.is_tensor(hvo_set) else type(hvo_set),))


def gather(hvo_set, idx, opts, state, lib=None, out=None):
    """gt_gather_infill on tensors: -> (x, y, removed) for the int64 indices idx (same device as hvo_set).  out: (x, y, removed) to fill."""
    lib = lib or _lib.get_lib()
    check_set(hvo_set)
    B = int(idx.shape[0])
    if out is None:
        out = (torch.empty(B, 32, 27, dtype=torch.float32, device=hvo_set.device), torch.empty(B, 32, 27, dtype=torch.float32, device=hvo_set.device),
               torch.empty(B, dtype=torch.int32, device=hvo_set.device))
    idx = idx.to(hvo_set.device, torch.int64).contiguous()
    lib.call("gt_gather_infill", _p(hvo_set), _p(idx), ctypes.c_int64(hvo_set.shape[0]), B, ctypes.byref(as_opts(opts)), _p(state),
             _p(out[0]), _p(out[1]), _p(out[2]), _stream(hvo_set))
    return out


def pair_once(hvo, opts, seed=0, step=0, device="cuda", lib=None):
    """An evaluation subset paired ONCE with a fixed state (step 0, the run's seed) through the same call as training, so that epoch-to-epoch
    metrics compare like with like.  Ineligible grooves are left out.  -> (x, y, removed) on the device."""
    hvo = torch.as_tensor(hvo, dtype=torch.float32).to(device).contiguous()
    return gather(hvo, infill_eligible(hvo, opts), opts, make_state(seed, step, hvo.device), lib)


def gather_events(hvo_set, idx, opts, state, lib=None, out=None):
    """gt_gather_infill_events on tensors: -> (x, y, cells) for the int64 indices idx (same device as hvo_set); cells (B,9) int32 bit words
    (bit t of cells[b, c]: cell (t, c) was removed).  out: (x, y, cells) to fill."""
    lib = lib or _lib.get_lib()
    check_set(hvo_set)
    eo = as_opts(opts)
    if not is_events(eo):
        raise ValueError("gather_events takes the event options (make_infill_event_opts), got %r" % (opts,))
    B = int(idx.shape[0])
    if out is None:
        out = (torch.empty(B, 32, 27, dtype=torch.float32, device=hvo_set.device), torch.empty(B, 32, 27, dtype=torch.float32, device=hvo_set.device),
               torch.empty(B, _lib.GT_VOICES, dtype=torch.int32, device=hvo_set.device))
    idx = idx.to(hvo_set.device, torch.int64).contiguous()
    lib.call("gt_gather_infill_events", _p(hvo_set), _p(idx), ctypes.c_int64(hvo_set.shape[0]), B, ctypes.byref(eo), _p(state),
             _p(out[0]), _p(out[1]), _p(out[2]), _stream(hvo_set))
    return out


def pair_once_events(hvo, opts, seed=0, step=0, device="cuda", lib=None):
    """pair_once for the event options: an evaluation subset paired ONCE with a fixed state.  Ineligible grooves are left out.
    -> (x, y, cells) on the device."""
    hvo = torch.as_tensor(hvo, dtype=torch.float32).to(device).contiguous()
    return gather_events(hvo, events_eligible(hvo, opts), opts, make_state(seed, step, hvo.device), lib)


def cell_words(cells, n, device):
    """(n,9) int32 bit words from what merge(cells=...) accepts: (n,9) int32 / uint32 words, or an (n,32,9) bool tensor (True: the model may
    fill cell (t, c))"""
    cells = torch.as_tensor(cells)
    if cells.dtype == torch.bool:
        if tuple(cells.shape) != (n, 32, _lib.GT_VOICES):
            raise ValueError("a bool cells tensor must be (%d, 32, 9), got %s" % (n, tuple(cells.shape)))
        w = (cells.to(device).to(torch.int64) << torch.arange(32, device=device, dtype=torch.int64).view(1, 32, 1)).sum(1)      # (n,9) in 0..2^32-1
        return torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32).contiguous()
    if tuple(cells.shape) != (n, _lib.GT_VOICES):
        raise ValueError("cells needs nine bit words per sequence, (%d, 9), got %s" % (n, tuple(cells.shape)))
    if cells.dtype == torch.int32:
        return cells.to(device).contiguous()
    if cells.dtype == getattr(torch, "uint32", None):
        return cells.to(device).contiguous().view(torch.int32)
    raise ValueError("cells must be int32 / uint32 bit words or bool, got %s" % (cells.dtype,))


def merge(hvo_pred, hvo_in, removed=None, mode=1, lib=None, out=None, cells=None):
    """gt_infill_merge on (N,32,27) tensors -> the finished grooves (a new tensor, or `out`, which may be hvo_pred).  cells (instead of
    removed): the mask per cell (gt_infill_merge_cells) -- (N,9) int32 / uint32 bit words as gather_events reports them, or (N,32,9) bool."""
    lib = lib or _lib.get_lib()
    if removed is not None and cells is not None:
        raise ValueError("merge takes removed (a bitmask of voices per sequence) or cells (a mask per cell), not both")
    if mode not in (0, 1):
        raise ValueError("merge mode must be 0 (the reference's sum) or 1 (the input's hits win whole), got %r" % (mode,))
    hvo_pred = hvo_pred.contiguous()
    hvo_in = torch.as_tensor(hvo_in, dtype=torch.float32).to(hvo_pred.device).contiguous()
    if hvo_pred.shape != hvo_in.shape or hvo_in.shape[-1] != 27:
        raise ValueError("merge needs two (N,32,27) HVO tensors, got %s / %s" % (tuple(hvo_pred.shape), tuple(hvo_in.shape)))
    n = hvo_in.numel() // (32 * 27)
    if removed is not None:
        removed = torch.as_tensor(removed).to(hvo_pred.device, torch.int32).contiguous()
        if removed.numel() != n:
            raise ValueError("removed needs one bitmask per sequence (%d), got %d" % (n, removed.numel()))
    out = torch.empty_like(hvo_pred) if out is None else out
    if cells is not None:
        cells = cell_words(cells, n, hvo_pred.device)
        lib.call("gt_infill_merge_cells", _p(hvo_pred), _p(hvo_in), _p(cells), ctypes.c_int64(n), int(mode), _p(out), _stream(hvo_pred))
        return out
    lib.call("gt_infill_merge", _p(hvo_pred), _p(hvo_in), _p(removed), ctypes.c_int64(n), int(mode), _p(out), _stream(hvo_pred))
    return out
