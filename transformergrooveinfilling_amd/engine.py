"""StepEngine: device-resident state of one GrooveTransformer replica and the per-step hot path.

Everything a train step touches lives in HBM for the life of the engine: ONE flat fp32 parameter
buffer (state-dict order, gt_param_layout), one flat gradient buffer of the same layout (a single RCCL
all-reduce and a single fused optimizer launch), optimizer moments, the positional-encoding buffer and
the 48-byte device step state (dropout seed/step, lr, Adam betas).  Per batch size there is a "slot":
activation workspace, static input/output buffers and the captured hipGraph of the whole step
(forward, loss, backward, update = one call into libgroove_hip.so, captured once, replayed).

Replaces, for the hot path only, the body of the reference's train_loop batch iteration
(ref:train.py:195-215: zero_grad / forward / calculate_loss / backward / opt.step) and
model.predict (ref:evaluator.py:173).  Data-parallel: one process per GPU, gradients summed with one
all-reduce over the flat buffer and averaged inside the optimizer kernel (grad_scale = 1/world).
"""
import ctypes
import os
import warnings
import weakref

import numpy as np
import torch

from . import _lib, infill, layout

ALGO = {"sgd": 0, "adam": 1, "adamw": 1}      # "adamw": adam with DECOUPLED weight decay (StepEngine.decoupled)
OVERLAP_MIN_BYTES = 16 << 20
EAGER_MAX_LAUNCHES = 24                # use_graph="auto": steps of at most this many launches are enqueued directly, not replayed
PREDICT_CHUNK = 512                    # floor of the sequences per gt_predict call
PREDICT_WS_BYTES = 32 << 30            # ... the chunk grows (x2) while its workspace stays under this and under half the free HBM
PREDICT_WS_KEEP = 4 << 30              # predict() keeps a workspace between calls only up to this size (a per-epoch evaluation must not pin tens of GiB)
MAX_GRAPHS = 4                         # captured step graphs kept per slot (least recently used dropped first)
MAX_SLOTS = 6                          # per-batch-size step slots kept (least recently created dropped first; the engine's own batch size stays)
XCHG_POLL_EVERY = 16                   # train steps between two asynchronous reads of the in-launch exchanges' error word (see poll_exchange; the first
                                       # read starts with the slot's first step)


_ENGINES = weakref.WeakSet()           # every live engine (clip_grad_norm_ in training.py finds the one that owns a parameter set)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _Slot:
    """Buffers and captured graph for one batch size."""

    def __init__(self, eng, B):
        f32 = dict(dtype=torch.float32, device=eng.device)
        d = eng.dims
        self.B = B
        self.cfg = _lib.make_config(B, d["embedding_size_src"], d["d_model"], d["n_heads"], d["dim_feedforward"],
                                    d["num_encoder_layers"], d["num_decoder_layers"], d["dropout"], d["precision"], eng.cfg_flags)
        self.layout_epoch = eng.lib.cdll.gt_layout_epoch()      # (the workspace below is laid out for the switches in force NOW: StepEngine.slot)
        self.ws = torch.empty(eng.lib.workspace_floats(self.cfg), **f32)
        eng.lib.call("gt_workspace_init", ctypes.byref(self.cfg), _ptr(self.ws), eng.stream)   # (zeroes the regions whose protocol relies on it)
        self.x = torch.zeros(B, 32, d["embedding_size_src"], **f32)
        self.y = torch.zeros(B, 32, 27, **f32)
        self.hvo = torch.zeros(B, 32, 27, **f32)
        self.tgt = torch.zeros(B, 32, 27, **f32)
        self.stats = torch.zeros(8, **f32)
        self.voice_stats = None        # gt_train_step_loss's per-voice statistics and its scratch: made by the first step with loss
        self.loss_scratch = None       # options (StepEngine._loss_ready); the scratch is zeroed once, every call leaves it zero
        self.idx = torch.zeros(B, dtype=torch.int64, device=eng.device)     # static batch indices of the indexed step
        self.removed = None            # train_step_indexed_infill: the removal bitmasks of the step's B draws (int32; made by its first step)
        self.cells = None              # train_step_indexed_infill_events: the removed cells of the step's B draws ((B,9) int32 bit words)
        self.graphs = {}               # step recipe -> captured hipGraph
        self.keep = {}                 # step recipe -> tensors whose raw pointers its graph holds
        self.use_graph = None          # StepEngine.graph_for's decision for this slot (use_graph="auto")
        self.fwd_id = 0                # bumped by every call that overwrites the saved activations (see StepEngine.forward)
        self.pack_epoch = -1           # StepEngine._pepoch at which this workspace's fragment-ordered weight copies were written
        self.xchg_off = None           # workspace offset of the QUAD pair-exchange region's error word (-1: none; looked up lazily)
        self.xchg_host = None          # pinned [error word, skipped updates] (data-parallel: the all-reduced guard element) copied asynchronously,
        self.xchg_event = None         # every XCHG_POLL_EVERY-th train step ... and the event behind that copy
        self.xchg_count = 0
        self.xchg_skipped_seen = 0     # value of the region's skipped-update counter at the last look (the counter restarts with the region)


class _LossSlot:
    """Buffers of one calculate_loss call size (no activation workspace: an evaluation set of thousands of sequences only
    needs its (N,32,27) predictions and targets here)."""

    def __init__(self, eng, B):
        f32 = dict(dtype=torch.float32, device=eng.device)
        d = eng.dims
        self.B = B
        self.cfg = _lib.make_config(B, d["embedding_size_src"], d["d_model"], d["n_heads"], d["dim_feedforward"],
                                    d["num_encoder_layers"], d["num_decoder_layers"], d["dropout"], d["precision"])
        self.hvo = torch.zeros(B, 32, 27, **f32)
        self.y = torch.zeros(B, 32, 27, **f32)
        self.stats = torch.zeros(8, **f32)
        self.voice_stats = None        # (as _Slot's)
        self.loss_scratch = None


class StepEngine:
    def __init__(self, d_model, n_heads, dim_feedforward, num_encoder_layers, num_decoder_layers=0,
                 dropout=0.0, embedding_size_src=16, batch_size=None, optimizer="sgd", learning_rate=0.05,
                 hit_loss_penalty=1.0, seed=0, device="cuda", world_size=1, use_graph="auto", lib=None, precision="fp32",
                 max_grad_norm=None, weight_decay=0.0, momentum=0.0, nesterov=False, loss_opts=None, infill_opts=None, infill_event_opts=None):
        self.device = torch.device(device)
        # The only way onto host memory is an EXPLICITLY passed library object (tests hand in the host-emulator build of
        # the same kernel sources to cover the multi-rank step sequence over gloo); nothing in the package does that.
        self.on_host = self.device.type == "cpu"
        if (self.on_host and lib is None) or (not self.on_host and not torch.cuda.is_available()):
            raise RuntimeError("StepEngine needs a ROCm GPU (torch.cuda.is_available() is False); "
                               "there is no CPU fallback for the hot path")
        self.lib = lib or _lib.get_lib()
        if not self.on_host and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.encoder_only = num_decoder_layers == 0
        self.algo = ALGO[optimizer.lower()]
        self.penalty = float(hit_loss_penalty)
        self.world_size = int(world_size)
        self.force_dp = False          # measurement aid: take the data-parallel step sequence even with one rank
        # True: one captured hipGraph per step recipe; False: plain launches; "auto" (default): a graph unless the step is a dozen
        # launches (sequence-resident path, gt_step_launches) -- there the graph's per-node cost (~0.4 us) exceeds what it saves
        # (headline shape: 0.246 ms replayed, 0.241 ms enqueued directly) and the one C call per step keeps the host ahead anyway
        self.use_graph = False if self.on_host else use_graph
        self.dims = dict(d_model=int(d_model), n_heads=int(n_heads), dim_feedforward=int(dim_feedforward),
                         num_encoder_layers=int(num_encoder_layers), num_decoder_layers=int(num_decoder_layers),
                         dropout=float(dropout), embedding_size_src=int(embedding_size_src),
                         precision=_lib.PRECISION[precision])     # 0 fp32 | 1 bf16 GEMM operands (BASELINE configs[4])
        probe = _lib.make_config(1, embedding_size_src, d_model, n_heads, dim_feedforward, num_encoder_layers,
                                 num_decoder_layers, dropout)
        self.total, self.entries = self.lib.param_layout(probe)
        self._probe_cfg = probe
        # global-norm gradient clipping of every train step (torch.nn.utils.clip_grad_norm_ between backward and update); None = off: the
        # step is the fused one, unchanged.  Settable at any time; the norm and the coefficient of a clipped step land in stats[6] / stats[7]
        self.max_grad_norm = max_grad_norm
        self._clip_scratch = None      # gt_clip_grad_norm's scratch (zeroed once; every call leaves it zero)
        # the optimizer's knobs beyond the defaults: torch.optim.SGD(momentum, nesterov, weight_decay; dampening 0), torch.optim.Adam(weight_decay)
        # (L2: added to the gradient) and, with optimizer="adamw", torch.optim.AdamW's decoupled decay.  All off (the default): the step is
        # the fused one, unchanged.  Settable at any time, like max_grad_norm; see _opt_extras
        self.weight_decay, self.momentum, self.nesterov = weight_decay, momentum, nesterov
        self.decoupled = optimizer.lower() == "adamw"
        # the loss's options beyond hit_loss_penalty (gt_loss_opts: separate hit and velocity / offset penalties, pos_weight, voice and term
        # weights, focal modulation): None = off, the step is the fused one, unchanged; else the tuple make_loss_opts() returns -- every step
        # then goes through gt_train_step_loss (the loss as a launch of its own) and fills the slot's voice_stats.  Settable at any time
        self.loss_opts = loss_opts
        self._lo_struct = (None, None)     # (tuple, its validated GtLossOpts)
        self.last_voice_stats = None       # module API: the 36 per-voice statistics of the last calculate_loss with options
        # the voice removal train_step_indexed_infill's gather draws (gt_infill_opts): None, or the tuple _lib.infill_opts_tuple() returns
        # (make_infill_opts).  Settable at any time; part of that step's graph key
        self.infill_opts = infill_opts
        self._io_struct = (None, None)     # (tuple, its validated GtInfillOpts)
        # the event removal train_step_indexed_infill_events' gather draws (gt_infill_event_opts): None, or the tuple
        # _lib.infill_event_opts_tuple() returns (make_infill_event_opts).  Settable at any time; part of that step's graph key
        self.infill_event_opts = infill_event_opts
        self._eo_struct = (None, None)     # (tuple, its validated GtInfillEventOpts)
        self.mbuf = None               # SGD's momentum buffers, flat like the gradients (zeros when momentum is first non-zero: torch's first step)
        self.names = layout.param_names(d_model, dim_feedforward, embedding_size_src, num_encoder_layers, num_decoder_layers)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(self.total, **f32)
        self.grads = torch.zeros(self.total, **f32)
        self.m = torch.zeros(self.total, **f32) if self.algo == 1 else None
        self.v = torch.zeros(self.total, **f32) if self.algo == 1 else None
        self.pe = torch.from_numpy(layout.positional_encoding(d_model)).to(self.device)
        st = _lib.GtStepState(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, 0, 0, learning_rate,
                              1.0 / self.world_size, 0.9, 0.999, 1e-8)
        self.state = torch.from_numpy(np.frombuffer(bytes(st), dtype=np.uint8).copy()).to(self.device)
        # Two gradient buckets, the first all-reduced under the rest of backward.  Splitting the step into two graphs costs
        # ~90 us per step on one GPU (0.434 vs 0.344 ms at the C2 shape, bench.py --force-dp), more than a 2.4 MB all-reduce
        # takes, so it is chosen by gradient bytes: from 16 MB (C3 31.7 MB, C4 38 MB) the all-reduce is several hundred
        # microseconds and worth hiding.  GT_DP_OVERLAP=0 / 1 forces it off / on.
        env = os.environ.get("GT_DP_OVERLAP")
        self.overlap_allreduce = (env == "1") if env in ("0", "1") else (4 * self.total >= OVERLAP_MIN_BYTES)
        self.reduce_stats = True       # data-parallel: the logged 8-float stats are averaged over ranks (one tiny all-reduce)
        # GT_DP_GRAPH=1: the whole data-parallel step (collectives included) as ONE captured hipGraph per step (measured with
        # bench.py --force-dp; off by default: it could not be exercised with more than one rank on the 1-GPU boxes of the build)
        self.dp_graph = os.environ.get("GT_DP_GRAPH", "0") == "1"
        self.dp_graph_failed = False   # a capture of the one-enqueue step failed once: eager sequence from then on (_dp_whole)
        self.dp_tune = None            # autotune_dp's table: {mode: ms per step (max over ranks)} and the mode kept
        self._capturing = False        # inside _replay's warm-up launch / capture: the recipe being recorded must not depend on the moment
        self._slots = {}
        # Fused whole steps on the sequence-resident path end with an update that also writes the next step's fragment-ordered
        # weights into the slot's workspace (GT_STEP_PACKS_CURRENT): valid while nothing else has written the parameters --
        # _pepoch counts the engine's own writes, params._version torch's (load_state_dict, init, in-place ops on the Parameters)
        self._pepoch, self._pver = 0, -1
        self.fold_pack = os.environ.get("GT_PACK_FOLD", "1") != "0"
        self._loss_slots = {}
        self._train_B = None           # batch size of the most recent train step (its slot is never evicted)
        self._predict_ws = {}          # chunk size -> (cfg, workspace, tgt scratch) of predict()
        self._predict_prob = {}        # chunk size -> (m,32,9) probabilities of gt_predict_voices; lives as long as that chunk's workspace
        self._predict_epoch = None     # gt_layout_epoch() those were sized at
        self._curve_buf = {}           # chunk size -> (HVO output, gt_hit_curve scratch) of hit_curve(); lives as long as that chunk's workspace
        self.voice_thresholds = None   # the nine thresholds of the last calibration (predict(voice_thresholds="calibrated"))
        # gt_config.flags of every configuration this engine hands to the library (per ENGINE, not per process: train.py's evaluation engines and
        # bench.py's second engine keep their own).  _flags_fallback: set for good once an in-launch exchange timed out (no QUAD, no row exchange);
        # _flags_recipe: what the data-parallel recipe in force asks for (bucketed overlap: no row exchange beside a collective's workgroups)
        self._flags_fallback, self._flags_recipe = 0, 0
        self.exchange_timeouts = 0     # in-launch exchanges that timed out (each: updates skipped until noticed, then the exchange-free schedule)
        self.skipped_updates = 0       # updates the device refused because of them (its own count: word 1 of the region's header), as far as seen
        self._ar_plan, self._ar_issued = [], 0      # data-parallel: the gradient all-reduces of the step in flight, and how many were issued (autotune_dp)
        self._bwd_slot = None          # module API: the slot of the last backward() (its workspace's error word guards the optimizer step)
        self._fused_opt = False        # ... a GrooveSGD / GrooveAdam is bound (training._FusedMixin): the update kernel itself honours the word
        self.xchg_strict = os.environ.get("GT_XCHG_STRICT", "0") == "1"       # raise instead of recovering
        self.B = int(batch_size) if batch_size else None
        if self.B:
            self.slot(self.B)
        _ENGINES.add(self)

    cfg_flags = property(lambda self: self._flags_fallback | self._flags_recipe)

    def _apply_flags(self):
        """Push cfg_flags into every configuration the engine keeps; schedules change with them, so captured graphs and the per-slot
        graph decision go (the workspace layout does not depend on them)."""
        f = self.cfg_flags
        for t in self._slots.values():
            if t.cfg.flags != f:
                t.cfg.flags = f
                t.graphs.clear(); t.keep.clear(); t.use_graph = None
        for cfg, _, _ in self._predict_ws.values():
            cfg.flags = f

    # ---- buffers ---------------------------------------------------------------------------------
    def slot(self, B):
        B = int(B)
        s = self._slots.get(B)
        if s is not None and s.layout_epoch != self.lib.cdll.gt_layout_epoch():
            # a layout switch (gt_set_operand_shadows) changed after this slot's workspace was sized: every offset may have moved and the
            # bf16-only regions may no longer fit -- the slot is re-made (its saved activations, graphs and weight packs go with it)
            warnings.warn("StepEngine: the workspace layout changed after the batch-%d slot was sized; re-making the slot" % B)
            del self._slots[B]
            self._predict_ws.clear()
        if B not in self._slots:
            if len(self._slots) >= MAX_SLOTS:                     # evaluation remainders etc.: bounded, like the loss slots
                # least recently USED first; never the engine's own batch size nor the slot the last train step ran on
                # (its captured graphs, kept tensors and weight packs would be re-made every epoch)
                keep = {self.B, self._train_B}
                self._slots.pop(next((k for k in self._slots if k not in keep), next(iter(self._slots))))
            self._slots[B] = _Slot(self, B)
        else:
            self._slots[B] = self._slots.pop(B)                   # (most recently used last)
        return self._slots[B]

    def loss_slot(self, B):
        """Buffers for a stand-alone calculate_loss over B sequences (kept apart from the train slots: the loss of an
        evaluation forward must not touch the activations a pending backward still needs)."""
        B = int(B)
        if B not in self._loss_slots:
            if len(self._loss_slots) >= 4:
                self._loss_slots.pop(next(iter(self._loss_slots)))
            self._loss_slots[B] = _LossSlot(self, B)
        return self._loss_slots[B]

    # convenience views of the default slot (bench / tests)
    x = property(lambda self: self.slot(self.B).x)
    y = property(lambda self: self.slot(self.B).y)
    hvo = property(lambda self: self.slot(self.B).hvo)
    stats = property(lambda self: self.slot(self.B).stats)
    cfg = property(lambda self: self.slot(self.B).cfg)

    def ensure_adam(self):
        if self.m is None:
            self.m = torch.zeros_like(self.params)
            self.v = torch.zeros_like(self.params)

    def views(self, flat=None):
        """name -> view into the flat parameter (or gradient/moment) buffer, state-dict order."""
        flat = self.params if flat is None else flat
        return {n: flat[off:off + size].view(*shp) for (n, shp), (off, size, _, _) in zip(self.names, self.entries)}

    def load_named(self, tensors):
        """Copy {state-dict name: tensor/ndarray} into the flat buffer (pe buffers are ignored)."""
        v = self.views()
        for n, t in tensors.items():
            if n in layout.PE_KEYS:
                continue
            if n not in v:
                raise KeyError("unexpected parameter %r" % n)
            src = t if torch.is_tensor(t) else torch.from_numpy(np.asarray(t, np.float32))
            v[n].copy_(src.to(self.device).view_as(v[n]))

    def state_struct(self):
        return _lib.GtStepState.from_buffer_copy(self.state.cpu().numpy().tobytes())

    def set_state(self, **kw):
        st = self.state_struct()
        for k, val in kw.items():
            setattr(st, k, val)
        self.state.copy_(torch.from_numpy(np.frombuffer(bytes(st), dtype=np.uint8).copy()))   # graphs stay valid

    def set_step_async(self, step):
        """Overwrite only the dropout step counter (bytes 8..11 of the device state), stream-ordered."""
        t = torch.tensor([step & 0x7FFFFFFF], dtype=torch.int32).view(torch.uint8)
        self.state[8:12].copy_(t, non_blocking=True)

    @property
    def stream(self):
        if self.on_host:
            return ctypes.c_void_p(0)
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- the hot path ----------------------------------------------------------------------------
    def _packs_current(self, s):
        """Are the fragment-ordered weight copies in slot s's workspace those of the current parameters?  (written by the last
        fused update on THIS slot, nothing -- the engine or torch -- has written the parameters since; never under graph replay:
        a captured graph would replay the flag blindly)"""
        return (self.fold_pack and not self._capturing and not self.graph_for(s) and s.pack_epoch == self._pepoch
                and self._pver == self.params._version)

    def _note_fused_step(self, s):
        """A fused whole step is about to update the parameters and write the NEXT step's weight copies into slot s's workspace:
        every other slot's copies go stale.  Called for every such step however it is issued -- also before a graph REPLAY, which
        runs none of _enqueue_step's Python (an eager slot would otherwise keep passing GT_STEP_PACKS_CURRENT over weights that
        a graphed slot's replay has updated)."""
        self._pepoch += 1
        s.pack_epoch, self._pver = self._pepoch, self.params._version

    # ---- the loss's options (gt_loss_opts): the loss as a launch of its own ----------------------------------------------------------------
    def _loss_ready(self, s, opts=None):
        """Before a call with loss options on slot s (train or loss slot), OUTSIDE any capture: the options validated, the slot's 36
        per-voice statistics and the kernel's scratch allocated (zeroed once; every call leaves it zero).  -> the GtLossOpts"""
        lo = self._loss_struct(opts)
        if s.loss_scratch is None:
            n = int(self.lib.cdll.gt_loss_scratch_floats(ctypes.byref(s.cfg)))
            if n <= 0:
                raise _lib.GrooveLibError("gt_loss_scratch_floats failed: %s" % self.lib.cdll.gt_last_error().decode())
            s.voice_stats = torch.zeros(36, dtype=torch.float32, device=self.device)
            s.loss_scratch = torch.zeros(n, dtype=torch.float32, device=self.device)
        return lo

    def make_loss_opts(self, vo_penalty=None, pos_weight=1.0, voice_weight=1.0, focal_gamma=0.0, term_weights=(1.0, 1.0, 1.0), hit_penalty=None):
        """A value for self.loss_opts: the validated, hashable tuple of a gt_loss_opts (its 24 floats in field order).  hit_penalty /
        vo_penalty default to the engine's hit_loss_penalty; pos_weight / voice_weight: a scalar or 9 values.  ValueError for a wrong length
        or a value outside its range."""
        ph = self.penalty if hit_penalty is None else hit_penalty
        return _lib.loss_opts_tuple(_lib.make_loss_opts(ph, ph if vo_penalty is None else vo_penalty, pos_weight, voice_weight, focal_gamma,
                                                        term_weights))

    def _loss_struct(self, opts=None):
        """the GtLossOpts of self.loss_opts (or of `opts`), validated once per value"""
        t = self.loss_opts if opts is None else opts
        if self._lo_struct[0] != t:
            if not isinstance(t, tuple) or len(t) != 24:
                raise ValueError("loss_opts must be None or the tuple StepEngine.make_loss_opts() returns, got %r" % (t,))
            lo = _lib.make_loss_opts(t[0], t[1], t[2:11], t[11:20], t[20], t[21:24])
            self._lo_struct = (_lib.loss_opts_tuple(lo), lo)
            if self._lo_struct[0] != t:
                raise ValueError("loss_opts holds values that are not fp32 numbers (use StepEngine.make_loss_opts): %r" % (t,))
        return self._lo_struct[1]

    @property
    def _lk(self):
        """what the loss's options add to a graph key (nothing while they are off: the keys are the fused step's own)"""
        return () if self.loss_opts is None else (self.loss_opts,)

    def _enqueue_step(self, s, skip_update):
        flags = skip_update
        if skip_update != 3 and self._packs_current(s):
            flags |= 4                         # GT_STEP_PACKS_CURRENT: no packing launch at the head of the step
        if skip_update == 0:                   # whole step: its update writes the next step's copies into this slot
            self._note_fused_step(s)
        if self.loss_opts is not None:
            self.lib.call("gt_train_step_loss", ctypes.byref(s.cfg), self.algo, _ptr(self.params), _ptr(self.grads),
                          _ptr(self.m), _ptr(self.v), _ptr(self.pe), _ptr(s.x), _ptr(s.y), ctypes.byref(self._loss_ready(s)),
                          _ptr(s.voice_stats), _ptr(s.loss_scratch), _ptr(s.hvo), _ptr(s.stats), _ptr(s.tgt), _ptr(s.ws),
                          _ptr(self.state), int(flags), self.stream)
            return
        self.lib.call("gt_train_step", ctypes.byref(s.cfg), self.algo, _ptr(self.params), _ptr(self.grads),
                      _ptr(self.m), _ptr(self.v), _ptr(self.pe), _ptr(s.x), _ptr(s.y),
                      ctypes.c_float(self.penalty), _ptr(s.hvo), _ptr(s.stats), _ptr(s.tgt), _ptr(s.ws),
                      _ptr(self.state), int(flags), self.stream)

    # ---- the optimizer's extras (momentum / Nesterov / weight decay / AdamW): one launch in front of the update ------------------------------
    # gt_optimizer_prepare rewrites the gradient buffer (AdamW: the parameter buffer) so that the unchanged update kernels apply the optimizer
    # torch would.  It sits at the head of enqueue_update, so every split sequence gets it: the data-parallel recipes (after the last
    # all-reduce and the clip), _watched_step, the module API's opt.step().  The single-process fused step takes the split sequence while
    # any extra is on (_split_step).
    def _opt_extras(self):
        """(weight_decay, momentum, nesterov, decoupled) of the pass, validated, or None while everything is off (no launch, the fused step)"""
        wd, mom, nest = float(self.weight_decay), float(self.momentum), bool(self.nesterov)
        if not wd >= 0.0 or not mom >= 0.0:
            raise ValueError("weight_decay and momentum must be >= 0, got %r / %r" % (self.weight_decay, self.momentum))
        if mom != 0.0 and self.algo != 0:
            raise ValueError("momentum belongs to the sgd optimizer (adam has its own moments), got momentum=%r" % (self.momentum,))
        if nest and mom == 0.0:
            raise ValueError("nesterov needs a momentum > 0 (torch.optim.SGD: 'Nesterov momentum requires a momentum and zero dampening')")
        if self.decoupled and self.algo != 1:
            raise ValueError("decoupled weight decay (optimizer='adamw') belongs to the adam update")
        if wd == 0.0 and mom == 0.0:
            return None
        if mom != 0.0 and self.mbuf is None:
            self.mbuf = torch.zeros_like(self.params)
        return (wd, mom, nest, bool(self.decoupled))

    def _enqueue_prepare(self, cfg, ws, hp):
        self.lib.call("gt_optimizer_prepare", ctypes.byref(cfg), self.algo, _ptr(self.params), _ptr(self.grads), _ptr(self.mbuf), _ptr(ws),
                      _ptr(self.state), ctypes.byref(_lib.GtOptHparams(hp[0], hp[1], int(hp[2]), int(hp[3]))), self.stream)

    def enqueue_update(self, zero_grads=True, slot=None):
        """Fused update over the flat buffers, behind the optimizer's extras (_opt_extras) when any is on.  zero_grads=True also clears
        the consumed gradients (fused step path); the torch.optim-style front keeps them until zero_grad() like torch does -- what it keeps
        is then the gradient as the extras left it.  slot: the step's slot -- its workspace then receives the next step's weight copies
        (gt_optimizer_step_ws)."""
        self._pepoch += 1
        if slot is None:
            slot = self._bwd_slot          # module API (loss.backward(); opt.step()): the slot backward() ran on
        hp = self._opt_extras()
        if slot is not None and slot.B in self._slots and self._slots[slot.B] is slot:
            if hp is not None:             # (with the workspace, like the update: the pass refuses whatever the update refuses)
                self._enqueue_prepare(slot.cfg, slot.ws, hp)
            # with the configuration and its workspace at hand the update honours the exchange region's error word and the data-parallel
            # guard element (gt_optimizer_step_ws: a timed-out exchange never reaches the parameters, Adam's t does not advance)
            if zero_grads and self.fold_pack:
                slot.pack_epoch, self._pver = self._pepoch, self.params._version
            self.lib.call("gt_optimizer_step_ws", ctypes.byref(slot.cfg), self.algo, _ptr(self.params), _ptr(self.grads), _ptr(self.m),
                          _ptr(self.v), _ptr(slot.ws), _ptr(self.state), int(zero_grads), self.stream)
            return
        if hp is not None:
            self._enqueue_prepare(self._probe_cfg, None, hp)
        self.lib.call("gt_optimizer_step", self.algo, _ptr(self.params), _ptr(self.grads), _ptr(self.m), _ptr(self.v),
                      ctypes.c_int64(self.total), _ptr(self.state), int(zero_grads), self.stream)

    # ---- global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) -------------------------------------------------
    # A clipped step (like one with the optimizer's extras on: _split_step) is the split sequence the data-parallel step already uses:
    # forward + loss + backward (skip_update = 1), the two
    # launches of gt_clip_grad_norm (norm into stats[6], coefficient into stats[7]; the loss kernels zero both, the 8-float stats copy
    # carries them), then the update.  Single process it is one captured graph per max_norm.  The exchanges' fail-safe stays with the
    # update: clipping never touches the guard element, and gt_optimizer_step_ws still refuses a step whose error word is set.
    def _clip_norm(self, max_norm):
        mn = float(max_norm)
        if not mn > 0.0:
            raise ValueError("max_grad_norm must be > 0 (inf: log the norm, never clip), got %r" % (max_norm,))
        if self._clip_scratch is None:            # (zeroed once, outside any capture; every call leaves it zero)
            n = int(self.lib.cdll.gt_clip_grad_norm_scratch_floats(ctypes.byref(self._probe_cfg)))
            if n <= 0:
                raise _lib.GrooveLibError("gt_clip_grad_norm_scratch_floats failed: %s" % self.lib.cdll.gt_last_error().decode())
            self._clip_scratch = torch.zeros(n, dtype=torch.float32, device=self.device)
        return mn

    def _enqueue_clip(self, cfg, out, max_norm):
        self.lib.call("gt_clip_grad_norm", ctypes.byref(cfg), _ptr(self.grads), _ptr(self.state), ctypes.c_float(max_norm), out,
                      _ptr(self._clip_scratch), self.stream)

    def _clip_step(self, s, max_norm):
        self._enqueue_clip(s.cfg, ctypes.c_void_p(s.stats.data_ptr() + 6 * 4), max_norm)     # -> stats[6] norm, stats[7] coefficient

    def _split_step(self, s, max_norm):
        """The single-process step as the split sequence: backward, [clip,] [the optimizer's extras +] update (max_norm None: no clip)"""
        self._enqueue_step(s, 1)
        if max_norm is not None:
            self._clip_step(s, max_norm)
        self.enqueue_update(slot=s)

    def _graph_for_split(self, s, clip=True, extras=False):
        """graph_for for the split step: use_graph="auto" counts its launches (the fused step's + 1: update and step_inc apart) plus the
        two of the clip and the one of the optimizer's extras"""
        if self.use_graph == "auto":
            n = self.lib.cdll.gt_step_launches(ctypes.byref(s.cfg))
            return not (0 < n and n + 1 + 2 * bool(clip) + bool(extras) + (self.loss_opts is not None) <= EAGER_MAX_LAUNCHES)
        return bool(self.use_graph)

    _graph_for_clip = _graph_for_split         # (the clipped step without extras)

    def _split_recipe(self, s, name, tail=()):
        """(graph key, decision, max_norm) of the split step in force, or None while neither clipping nor an extra is on.  The key
        carries everything baked into the launches: max_norm and the hyper-parameter tuple."""
        if self.max_grad_norm is None and not (self.weight_decay or self.momentum or self.nesterov):
            return None                            # (the default, on every step of the fused path: decided without more ado)
        hp = self._opt_extras()
        if self.max_grad_norm is None and hp is None:
            return None
        mn = None if self.max_grad_norm is None else self._clip_norm(self.max_grad_norm)
        key = (name + ("_clip" if mn is not None else "_prep"), self.algo, self.penalty) + self._lk + (() if mn is None else (mn,)) + (hp or ()) + tail
        return key, self._graph_for_split(s, mn is not None, hp is not None), mn

    def clip_grad_norm_(self, max_norm):
        """torch.nn.utils.clip_grad_norm_(parameters, max_norm) over the flat gradient buffer (module API: between loss.backward() and
        opt.step()): the same two launches as a clipped step, no synchronisation.  -> the total norm before clipping, a 0-dim device
        tensor.  Data-parallel: call it on the all-reduced sums (grad_scale = 1/world makes it the norm of the averaged gradient)."""
        mn = self._clip_norm(max_norm)
        out = torch.empty(2, dtype=torch.float32, device=self.device)
        self._enqueue_clip(self._probe_cfg, _ptr(out), mn)
        return out[0]

    def graph_for(self, s):
        """Does slot s replay captured graphs?  (use_graph True / False / "auto": by the step's launch count)"""
        if self.use_graph == "auto":
            if self.loss_opts is not None:    # (the loss as a launch of its own: one more; not cached -- the options come and go)
                n = self.lib.cdll.gt_step_launches(ctypes.byref(s.cfg))
                return not (0 < n and n + 1 <= EAGER_MAX_LAUNCHES)
            if s.use_graph is None:
                n = self.lib.cdll.gt_step_launches(ctypes.byref(s.cfg))
                s.use_graph = not (0 < n <= EAGER_MAX_LAUNCHES)
            return s.use_graph
        return bool(self.use_graph)

    def _replay(self, s, key, fn, aux=False, force=False, graph=None):
        """Replay the hipGraph captured for `key` on slot s (captured on first use).  aux=True: a graph that continues a
        step another graph began (second half of a bucketed backward) -- it keeps the slot's other graphs.  force=True: a graph
        whatever graph_for says (the one-enqueue data-parallel step).  graph: the decision, when it is not graph_for's (clipped step)."""
        if not (force or (self.graph_for(s) if graph is None else graph)):
            fn()
            return
        if key not in s.graphs:
            if not aux and len(s.graphs) >= MAX_GRAPHS:      # a small LRU instead of dropping everything: alternating recipes (train_step /
                s.graphs.pop(next(iter(s.graphs)))          # train_step_indexed, a second resident dataset) must not re-capture every call
            # one launch outside capture (code-object load), every buffer it touched restored, then capture once
            side = torch.cuda.Stream(self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            snap = (self.params.clone(), self.state.clone(), None if self.m is None else (self.m.clone(), self.v.clone()),
                    self.grads.clone(), None if self.mbuf is None else self.mbuf.clone())
            self._capturing = True                # (no GT_STEP_PACKS_CURRENT in a recorded recipe: a replay would pass it blindly)

            def restore():
                torch.cuda.current_stream(self.device).wait_stream(side)
                torch.cuda.synchronize(self.device)
                self.params.copy_(snap[0]); self.state.copy_(snap[1])
                if snap[2] is not None:
                    self.m.copy_(snap[2][0]); self.v.copy_(snap[2][1])
                if snap[4] is not None:
                    self.mbuf.copy_(snap[4])
                self.grads.copy_(snap[3])         # zeros for a whole-step graph (gt_train_step's precondition), else what the first half left
            try:
                try:
                    with torch.cuda.stream(side):
                        fn()
                finally:
                    restore()                     # (also when the warm-up raised half-way: a caller that falls back to the eager sequence
                                                  #  must not apply part of this step twice)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
            finally:
                self._capturing = False
            s.graphs[key] = g
        g = s.graphs.pop(key)
        s.graphs[key] = g                         # (most recently used last)
        g.replay()

    def _dp_whole(self, s, key, whole):
        """The data-parallel step as ONE captured hipGraph (collectives included) -- with a way back: a capture that fails (a collective
        that cannot be recorded on this stack, an allocator call inside the capture) is logged once and the step, like every later one,
        runs as the eager sequence in this same process.  A FIRST capture runs one real warm-up step (collectives included) before it records,
        so it must happen on the same step on every rank: it does at the first step, and again after a recovery from an exchange time-out --
        which is collective in a multi-rank run for exactly this reason (_recover_exchange).  When the capture itself fails on one rank, that
        rank's eager step stands in for the replay the others run: the same collectives in the same order."""
        if not self.dp_graph_failed:
            try:
                self._replay(s, key, whole, force=True)
                self._note_fused_step(s)          # (after the replay: the update inside it wrote the next step's weight copies)
                return
            except Exception as e:                # noqa: BLE001 -- whatever the capture raised
                import warnings
                self.dp_graph_failed = True
                s.graphs.pop(key, None)
                if not self.on_host:
                    torch.cuda.synchronize(self.device)
                warnings.warn("data-parallel step: hipGraph capture failed (%s: %s); falling back to the eager sequence" %
                              (type(e).__name__, e), RuntimeWarning)
        whole()

    def _ar(self, t, async_op=False):
        """A gradient all-reduce of the data-parallel step (counted: autotune_dp keeps a failing rank in step with the others)."""
        import torch.distributed as dist
        self._ar_issued += 1
        return dist.all_reduce(t, async_op=async_op)

    def _dp_recipe(self, overlap, graph):
        """Select a data-parallel recipe: {one all-reduce after backward | two buckets, the first under the rest of backward} x {eager
        sequence | one hipGraph per step}.  The bucketed recipe runs a collective's workgroups beside the backward's launches, whose
        LayerNorm row exchange needs its whole grid resident: this ENGINE's configurations then carry GT_CFG_NO_LN_XCHG (the norm as a row pass
        of its own); captured graphs of another recipe are dropped with the flag change."""
        self.overlap_allreduce, self.dp_graph, self.dp_graph_failed = bool(overlap), bool(graph), False
        two = bool(overlap) and self.B is not None and len(self.lib.grad_buckets(self.slot(self.B).cfg)) == 2
        self._flags_recipe = _lib.CFG_NO_LN_XCHG if two else 0
        self._apply_flags()

    def autotune_dp(self, steps=30, warmup=3, modes=None):
        """world > 1: time `steps` steps of every data-parallel recipe -- {single all-reduce, two overlapped buckets} x {eager sequence,
        one hipGraph per step} -- on the engine's static batch, keep the fastest.  Every rank takes the MAX over ranks of each time (one
        tiny all-reduce per recipe), so all ranks keep the same recipe.  Parameters, optimizer state and step counters are restored:
        the run that follows is the run that would have been.  -> {"modes": {name: ms}, "chosen": name}

        A rank on which a recipe RAISES must not leave the others inside that recipe's collectives: it completes the gradient all-reduces
        of the step it failed in (those of the step's plan not yet issued), then issues the plan of every remaining step of the recipe --
        garbage sums, thrown away with the snapshot restore -- and reports +inf, so the MAX all-reduce that closes the recipe is reached by
        every rank after the same number of collectives and the recipe is simply not chosen (tests/test_exchange_failsafe.py)."""
        import time
        import torch.distributed as dist
        s = self.slot(self.B)
        two = len(self.lib.grad_buckets(s.cfg)) == 2
        cand = [(False, False)] + ([(True, False)] if two else [])
        # the one-hipGraph-per-step recipes (collectives recorded as graph nodes) join the comparison only on request (GT_DP_TUNE_GRAPH=1):
        # they have run with a 1-rank RCCL group only, and a collective that HANGS under capture on real ranks -- unlike one that raises,
        # which _dp_whole survives -- would take the whole run with it.  The eager recipes are the safe set for a first multi-GPU run.
        if not self.on_host and os.environ.get("GT_DP_TUNE_GRAPH", "0") == "1":
            cand += [(False, True)] + ([(True, True)] if two else [])
        if modes is not None:
            cand = [c for c in cand if c in modes]
        name = lambda c: ("buckets" if c[0] else "plain") + ("_graph" if c[1] else "_eager")
        snap = (self.params.clone(), self.state.clone(), None if self.m is None else (self.m.clone(), self.v.clone()),
                None if self.mbuf is None else self.mbuf.clone())
        sync = (lambda: None) if self.on_host else (lambda: torch.cuda.synchronize(self.device))
        table, errors = {}, {}
        for c in cand:
            self._dp_recipe(*c)                    # (flags and graphs are this candidate's own: like is compared with like)
            t, t0, failed = float("inf"), None, None
            for i in range(warmup + steps):
                if i == warmup and failed is None:
                    sync(); dist.barrier(); t0 = time.perf_counter()
                elif i == warmup:
                    dist.barrier()                 # (a failed rank still joins the barrier the others time from)
                if failed is None:
                    try:
                        self.train_step()
                        continue
                    except Exception as e:         # noqa: BLE001 -- a recipe that cannot run on this stack is simply not chosen
                        failed = e
                        errors[name(c)] = "%s: %s" % (type(e).__name__, e)
                        plan = list(self._ar_plan)
                        done = self._ar_issued % len(plan) if plan else 0
                        self.grads[self.total - 1:].zero_()       # (the guard element: this rank's garbage must not read as an exchange time-out)
                        if not (plan and self._ar_issued and done == 0):       # (all of the step's collectives were out already)
                            for o, n in plan[done:]:
                                dist.all_reduce(self.grads[o:o + n])
                        continue
                for o, n in self._ar_plan:         # a failed rank: the collectives of the steps the others still run
                    dist.all_reduce(self.grads[o:o + n])
            sync()
            if failed is None:
                t = (time.perf_counter() - t0) / steps * 1e3
                if c[1] and self.dp_graph_failed:
                    t = float("inf")               # (it ran, but as the eager sequence)
            tt = torch.tensor([t if t != float("inf") else 1e30], dtype=torch.float64, device=self.device if not self.on_host else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            table[name(c)] = float(tt)
            self.params.copy_(snap[0]); self.state.copy_(snap[1]); self.grads.zero_()
            if snap[2] is not None:
                self.m.copy_(snap[2][0]); self.v.copy_(snap[2][1])
            if snap[3] is not None:
                self.mbuf.copy_(snap[3])
            self._pepoch += 1                      # (the parameters were rewritten: every slot's weight copies are stale)
            for t_ in self._slots.values():        # (graphs of this candidate go: the next one -- and the run -- record their own)
                t_.graphs.clear(); t_.keep.clear()
        best = min(cand, key=lambda c: table[name(c)])
        self._dp_recipe(*best)
        self.dp_tune = {"modes": {k: (None if v >= 1e29 else round(v, 5)) for k, v in table.items()}, "chosen": name(best), "steps": steps}
        if errors:
            self.dp_tune["errors"] = errors
        return self.dp_tune

    def _watched_step(self, s, on_grads):
        """One step with the gradients VISIBLE between backward and update: forward + loss + backward (skip_update = 1), on_grads() --
        the caller reads self.grads / the Parameters' .grad views --, then the fused update.  The fused whole step consumes and
        re-zeroes the gradients inside its last launch, so nothing (wandb.watch's hooks included, ref:train.py:150) ever sees them;
        train_loop takes this path every `watch_log_freq` batches instead."""
        self._enqueue_step(s, 1)
        on_grads()
        if self.max_grad_norm is not None:     # (the hooks see the gradients before clipping, as torch's backward hooks would)
            self._clip_step(s, self._clip_norm(self.max_grad_norm))
        self.enqueue_update(slot=s)

    def train_step(self, x=None, y=None, B=None, on_grads=None):
        """One optimisation step on (x, y) (device or host tensors; None = reuse the static buffers).
        Returns the device stats tensor [loss, hit_acc, -, bce, mse_v, mse_o, -, -] without syncing.
        on_grads: called between backward and update of THIS step (single process; see _watched_step)."""
        s = self.slot(x.shape[0] if x is not None else (B or self.B))
        self._train_B = s.B
        s.fwd_id += 1
        if self.loss_opts is not None:
            self._loss_ready(s)
        if x is not None:
            s.x.copy_(x, non_blocking=True)
        if y is not None:
            s.y.copy_(y, non_blocking=True)
        single = self.world_size == 1 and not self.force_dp
        split = self._split_recipe(s, "fused") if single and on_grads is None else None
        if single and on_grads is not None:
            self._watched_step(s, on_grads)
        elif split is not None:
            key, use, mn = split
            if use:
                self._note_fused_step(s)          # (the replay updates the parameters and writes the next step's weight copies)
            self._replay(s, key, lambda: self._split_step(s, mn), graph=use)
        elif single:
            if self.graph_for(s):
                self._note_fused_step(s)          # (a replay updates the parameters without running _enqueue_step)
            key = ("fused", self.algo, self.penalty)
            self._replay(s, key if self.loss_opts is None else key + self._lk, lambda: self._enqueue_step(s, 0))
        else:
            buckets = self.lib.grad_buckets(s.cfg) if self.overlap_allreduce else []
            two = len(buckets) == 2
            if two != bool(self._flags_recipe & _lib.CFG_NO_LN_XCHG):
                # bucket 0's all-reduce runs UNDER the rest of backward: a collective's workgroups beside launches whose workgroups wait for each
                # other (the LayerNorm row exchange needs its whole grid resident) -- the norm runs as a row pass of its own in this recipe.
                # A flag of THIS engine's configurations (gt_config.flags), not a process-wide switch.
                self._flags_recipe = _lib.CFG_NO_LN_XCHG if two else 0
                self._apply_flags()
            # the step's gradient all-reduces, in issue order (autotune_dp completes them on a rank whose step raised)
            self._ar_plan = [tuple(b) for b in buckets] if two else [(0, self.total)]
            self._ar_issued = 0
            guard = self._guard_fn(s)
            mn = None if self.max_grad_norm is None else self._clip_norm(self.max_grad_norm)     # clipping: after the last all-reduce, before the update
            hp = self._opt_extras()               # the optimizer's extras: at the head of enqueue_update, so after the clip (validated here, before any launch)
            if self.dp_graph and on_grads is None and not self.on_host:
                # ONE enqueue per step: forward + backward, the all-reduce(s) and the update captured in one hipGraph -- the collectives are
                # nodes of the graph (RCCL enqueues on its own stream: fork / join edges), nothing returns to Python between the halves
                def whole():
                    if two:
                        (o0, c0), (o1, c1) = buckets
                        self._enqueue_step(s, 2)
                        guard()
                        w0 = self._ar(self.grads[o0:o0 + c0], async_op=True)
                        self._enqueue_step(s, 3)
                        w1 = self._ar(self.grads[o1:o1 + c1], async_op=True)
                        w0.wait(); w1.wait()
                    else:
                        self._enqueue_step(s, 1)
                        guard()
                        self._ar(self.grads)
                    if mn is not None:
                        self._clip_step(s, mn)
                    self.enqueue_update(slot=s)
                key = ("dp_whole", self.algo, self.penalty, len(buckets)) + self._lk + (() if mn is None else (mn,)) + (hp or ())
                self._dp_whole(s, key, whole)
                self.poll_exchange(s)
                return s.stats
            if two:
                # bucketed overlap: graph A ends as soon as the upper bucket's gradients are final; its
                # all-reduce (RCCL stream) runs under graph B, the rest of backward.  The collectives stay OUTSIDE the
                # captured graphs.  Sums over ranks; averaged by grad_scale inside the optimizer kernel.
                (o0, c0), (o1, c1) = buckets
                self._replay(s, ("bwd_top", self.algo, self.penalty) + self._lk, lambda: self._enqueue_step(s, 2))
                guard()
                w0 = self._ar(self.grads[o0:o0 + c0], async_op=True)
                if self.graph_for(s) and ("bwd_rest", self.algo, self.penalty) + self._lk not in s.graphs:
                    w0.wait()                     # first step only: the capture warm-up snapshots and restores the gradient buffer
                self._replay(s, ("bwd_rest", self.algo, self.penalty) + self._lk, lambda: self._enqueue_step(s, 3), aux=True)
                w1 = self._ar(self.grads[o1:o1 + c1], async_op=True)
                w0.wait(); w1.wait()
            else:
                self._replay(s, ("fwdbwd", self.algo, self.penalty) + self._lk, lambda: self._enqueue_step(s, 1))
                guard()
                self._ar(self.grads)                         # RCCL sum over xGMI; averaged by grad_scale
            if on_grads is not None:
                on_grads()                        # (data-parallel: the all-reduced sums; the update averages them by grad_scale)
            if mn is not None:
                self._clip_step(s, mn)
            self.enqueue_update(slot=s)
        self.poll_exchange(s)
        return s.stats

    def train_step_indexed(self, xs, ys, idx, on_grads=None):
        """One optimisation step on rows `idx` (device int64, len B) of a dataset resident in HBM (xs (N,32,S), ys (N,32,27)):
        the gather into the static step inputs is the first launch of the step's hipGraph (gt_gather_batch), nothing is
        copied on the host side but the B indices into their static buffer.  Data-parallel: as train_step."""
        s = self.slot(idx.shape[0])
        self._train_B = s.B
        s.fwd_id += 1
        if self.loss_opts is not None:
            self._loss_ready(s)
        s.idx.copy_(idx, non_blocking=True)

        def gather():
            self.lib.call("gt_gather_batch", _ptr(xs), _ptr(ys), _ptr(s.idx), ctypes.c_int64(xs.shape[0]), int(s.B),
                          int(self.dims["embedding_size_src"]), _ptr(s.x), _ptr(s.y), self.stream)

        return self._indexed_step(s, (xs.data_ptr(), ys.data_ptr(), xs.shape[0]), gather, (xs, ys), on_grads)

    def _indexed_step(self, s, key, gather, keep, on_grads):
        """The step behind an indexed gather (train_step_indexed / train_step_indexed_infill / _infill_events): `gather` enqueues the launch that fills the
        slot's static inputs, `key` is what it bakes into a captured graph, `keep` the resident tensors whose raw pointers that graph holds."""
        if on_grads is not None:
            gather()
            return self.train_step(B=s.B, on_grads=on_grads)
        if self.world_size == 1 and not self.force_dp:
            split = self._split_recipe(s, "fused_idx", key)
            if split is not None:
                gkey, use, mn = split
                if use:
                    self._note_fused_step(s)
                self._replay(s, gkey, lambda: (gather(), self._split_step(s, mn)), graph=use)
            else:
                gkey = ("fused_idx", self.algo, self.penalty) + self._lk + key
                if self.graph_for(s):
                    self._note_fused_step(s)
                self._replay(s, gkey, lambda: (gather(), self._enqueue_step(s, 0)))
            if gkey in s.graphs:
                s.keep[gkey] = keep               # the captured graph holds their raw pointers: keep the tensors alive with it
                for k in [k for k in s.keep if k not in s.graphs]:
                    del s.keep[k]
            self.poll_exchange(s)
            return s.stats
        gather()
        return self.train_step(B=s.B)

    def make_infill_opts(self, voices=(2,), min_remove=1, max_remove=None, prob=None):
        """A value for self.infill_opts: the validated, hashable tuple of a gt_infill_opts (the reference's voices_params: voice_idx,
        min / max_n_voices_to_remove, prob)."""
        return _lib.infill_opts_tuple(_lib.make_infill_opts(voices, min_remove, max_remove, prob))

    def train_step_indexed_infill(self, hvo_set, idx, on_grads=None):
        """train_step_indexed for the symbolic infilling experiments: ONE resident tensor of FULL grooves hvo_set (N,32,27); the gather at the
        head of the step's hipGraph (gt_gather_infill) draws, per batch element, the voices to remove (self.infill_opts) from the engine's own
        device step state -- every replay draws afresh once the update has advanced the step -- and fills both static step inputs: x = the
        groove without them, y = the removed part.  The slot's `removed` (int32, B) holds the bitmasks of the last step."""
        if self.dims["embedding_size_src"] != _lib.GT_TGT:
            raise ValueError("train_step_indexed_infill needs a symbolic model (embedding_size_src 27: the input is an HVO groove), got %d"
                             % self.dims["embedding_size_src"])
        if self.infill_opts is None:
            raise ValueError("train_step_indexed_infill: set infill_opts first (StepEngine.make_infill_opts)")
        infill.check_set(hvo_set)
        s = self.slot(idx.shape[0])
        self._train_B = s.B
        s.fwd_id += 1
        if self.loss_opts is not None:
            self._loss_ready(s)
        if s.removed is None:
            s.removed = torch.zeros(s.B, dtype=torch.int32, device=self.device)
        s.idx.copy_(idx, non_blocking=True)
        if self._io_struct[0] != self.infill_opts:           # (validated once per value, like the loss's options)
            self._io_struct = (self.infill_opts, _lib.infill_opts_struct(self.infill_opts))
        io = self._io_struct[1]
        key = ("infill",) + self.infill_opts + (hvo_set.data_ptr(), hvo_set.shape[0])

        def gather():
            self.lib.call("gt_gather_infill", _ptr(hvo_set), _ptr(s.idx), ctypes.c_int64(hvo_set.shape[0]), int(s.B), ctypes.byref(io),
                          _ptr(self.state), _ptr(s.x), _ptr(s.y), _ptr(s.removed), self.stream)

        return self._indexed_step(s, key, gather, (hvo_set,), on_grads)

    def make_infill_event_opts(self, voices=range(_lib.GT_VOICES), ratio=(0.4, 0.6)):
        """A value for self.infill_event_opts: the validated, hashable tuple of a gt_infill_event_opts (the voices whose hits may be removed,
        the share of them to remove: the reference's remove_random_events thres_range)."""
        return _lib.infill_event_opts_tuple(_lib.make_infill_event_opts(voices, ratio))

    def train_step_indexed_infill_events(self, hvo_set, idx, on_grads=None):
        """train_step_indexed_infill with the event-level pairing: the gather at the head of the step (gt_gather_infill_events) removes, per
        batch element, a random share of the individual hits (self.infill_event_opts), drawn from the engine's own device step state -- every
        replay draws afresh -- and fills both static step inputs: x = the groove without those hits, y = the removed hits.  The slot's
        `cells` ((B,9) int32 bit words: bit t of cells[b, c] = cell (t, c) was removed) holds the draws of the last step."""
        if self.dims["embedding_size_src"] != _lib.GT_TGT:
            raise ValueError("train_step_indexed_infill_events needs a symbolic model (embedding_size_src 27: the input is an HVO groove), got %d"
                             % self.dims["embedding_size_src"])
        if self.infill_event_opts is None:
            raise ValueError("train_step_indexed_infill_events: set infill_event_opts first (StepEngine.make_infill_event_opts)")
        infill.check_set(hvo_set)
        s = self.slot(idx.shape[0])
        self._train_B = s.B
        s.fwd_id += 1
        if self.loss_opts is not None:
            self._loss_ready(s)
        if s.cells is None:
            s.cells = torch.zeros(s.B, _lib.GT_VOICES, dtype=torch.int32, device=self.device)
        s.idx.copy_(idx, non_blocking=True)
        if self._eo_struct[0] != self.infill_event_opts:     # (validated once per value, like the loss's options)
            self._eo_struct = (self.infill_event_opts, _lib.infill_event_opts_struct(self.infill_event_opts))
        eo = self._eo_struct[1]
        key = ("infill",) + self.infill_event_opts + (hvo_set.data_ptr(), hvo_set.shape[0])

        def gather():
            self.lib.call("gt_gather_infill_events", _ptr(hvo_set), _ptr(s.idx), ctypes.c_int64(hvo_set.shape[0]), int(s.B), ctypes.byref(eo),
                          _ptr(self.state), _ptr(s.x), _ptr(s.y), _ptr(s.cells), self.stream)

        return self._indexed_step(s, key, gather, (hvo_set,), on_grads)

    def voice_metrics(self, hvo_pred, hvo_gt):
        """Per-voice evaluation metrics of predictions against ground truth, both (N,32,27) HVO tensors on the device
        (gt_voice_metrics; ref:evaluator.py:522-525) -> 30-float device tensor (layout: include/groove_hip.h)."""
        p = torch.as_tensor(hvo_pred, dtype=torch.float32).to(self.device).contiguous()
        g = torch.as_tensor(hvo_gt, dtype=torch.float32).to(self.device).contiguous()
        assert p.shape == g.shape and p.shape[-1] == 27
        rows = p.numel() // 27
        out = torch.empty(30, dtype=torch.float32, device=self.device)
        scratch = torch.empty(int(self.lib.cdll.gt_voice_metrics_scratch_floats(ctypes.c_int64(rows))), dtype=torch.float32, device=self.device)
        self.lib.call("gt_voice_metrics", _ptr(p), _ptr(g), ctypes.c_int64(rows), _ptr(out), _ptr(scratch), self.stream)
        return out

    def forward_eval_chunked(self, x, tgt_in=None, chunk=PREDICT_CHUNK):
        """Eval forward of a large set (the reference hands the whole test / validation set to the model at once,
        ref:train.py:195-215) in chunks of `chunk` sequences through ONE reusable slot: the activation workspace of N = 4096
        sequences would be 18.7 GiB at d512 / F2048.  Returns a fresh (N,32,27) tensor; no saved activations (not differentiable)."""
        n = x.shape[0]
        out = torch.empty(n, 32, 27, dtype=torch.float32, device=self.device)
        for i in range(0, n, chunk):
            j = min(n, i + chunk)
            out[i:j].copy_(self.forward(x[i:j], None if tgt_in is None else tgt_in[i:j], train=False))
        return out

    def forward(self, x, tgt_in=None, train=False):
        """Eval/train forward for any batch size -> (B,32,27) [h logits | v | o] buffer of that slot."""
        s = self.slot(x.shape[0])
        s.fwd_id += 1
        s.x.copy_(x)
        if tgt_in is not None:
            s.tgt.copy_(tgt_in)
        def run():
            self.lib.call("gt_forward", ctypes.byref(s.cfg), _ptr(self.params), _ptr(self.pe), _ptr(s.x),
                          None if self.encoder_only else _ptr(s.tgt), _ptr(s.hvo), _ptr(s.ws), _ptr(self.state),
                          int(train), self.stream)
        run()
        # evaluation forwards are consumed on the host right away: a timed-out exchange is noticed here and the forward repeated on the
        # exchange-free schedule (a forward has no side effects).  Rank-LOCAL by construction (an evaluation may run on one rank only): in a
        # multi-rank run the repeat borrows the fallback flags for this call alone, see _local_retry.  Training forwards of the module API are
        # covered by the optimizer step: the update kernel applies nothing while the word is set (backward() starts the asynchronous poll).
        if not train and self._xchg_word(s) is not None and int(self._xchg_word(s)[0].item()) != 0:
            self._local_retry(s.ws, s.cfg, "an evaluation forward", run)
        return s.hvo

    def loss(self, s, y, penalty, want_grad=True, opts=None):
        """calculate_loss on slot s's current hvo.  -> (stats, d_hvo) device tensors.  opts: a make_loss_opts() tuple -- the loss with
        options (gt_loss_ex; `penalty` is then the tuple's own), which also fills s.voice_stats."""
        s.y.copy_(y)
        d_hvo = torch.empty_like(s.hvo) if want_grad else None
        if opts is not None:
            self.lib.call("gt_loss_ex", ctypes.byref(s.cfg), _ptr(s.hvo), _ptr(s.y), ctypes.byref(self._loss_ready(s, opts)), _ptr(s.stats),
                          _ptr(s.voice_stats), _ptr(d_hvo), 0, _ptr(s.loss_scratch), self.stream)
            return s.stats, d_hvo
        self.lib.call("gt_loss", ctypes.byref(s.cfg), _ptr(s.hvo), _ptr(s.y), ctypes.c_float(penalty), _ptr(s.stats),
                      _ptr(d_hvo), self.stream)
        return s.stats, d_hvo

    def backward(self, s, d_hvo, train, accumulate=True):
        self.lib.call("gt_backward", ctypes.byref(s.cfg), _ptr(self.params), _ptr(self.grads), _ptr(s.x),
                      None if self.encoder_only else _ptr(s.tgt), _ptr(s.hvo), _ptr(d_hvo), _ptr(s.ws), _ptr(self.state),
                      int(train), int(accumulate), self.stream)
        # module API (loss.backward(); opt.step()): gradients computed through a timed-out exchange are garbage.  With the package's own
        # optimizers (GrooveSGD / GrooveAdam: initialize_model's) the UPDATE KERNEL refuses them -- enqueue_update hands it this slot's error
        # word: parameters, moments and Adam's t stay, the skip is counted -- and the asynchronous poll started here notices the word and
        # falls back.  Only for a foreign torch optimizer stepping the Parameters directly are the gradients zeroed on the device (no
        # synchronisation); that costs a pass over the gradient buffer and still lets weight decay / old moments move the weights.
        self._bwd_slot = s
        w = self._xchg_word(s)
        if w is not None and not self.on_host:
            if not self._fused_opt:
                self.grads.masked_fill_((w[:1] != 0).expand(self.total), 0.0)
            self.poll_exchange(s)

    def predict_chunk(self, n):
        """Sequences per gt_predict call for a set of n: as many as fit the workspace budget (greedy decoding is launch-bound --
        2240 launches per call whatever the batch -- so 8 calls of 512 cost 2.4x one call of 4096)."""
        d = self.dims
        budget = PREDICT_WS_BYTES
        if not self.on_host:
            budget = min(budget, torch.cuda.mem_get_info(self.device)[0] // 2)
        chunk = PREDICT_CHUNK
        while chunk < n:
            cfg = _lib.make_config(2 * chunk, d["embedding_size_src"], d["d_model"], d["n_heads"], d["dim_feedforward"],
                                   d["num_encoder_layers"], d["num_decoder_layers"], d["dropout"], d["precision"])
            if 4 * self.lib.workspace_floats(cfg) > budget:
                break
            chunk *= 2
        return chunk

    def voice_sampling(self, use_thres=True, thres=0.5, pd_seed=None, voice_thresholds=None, voice_max_count=None, temperature=1.0,
                       mask_vo=False):
        """The gt_voice_sampling of a predict call, or None when every per-voice keyword has its default (the call then runs exactly as
        gt_predict / gt_predict_pd_at).  voice_thresholds (9 values in [0,1]) override thres; pd_seed selects the sampled mode, whose
        thresholds are 0 unless given.  ValueError for a wrong length or range, before the library is called."""
        if voice_thresholds is None and voice_max_count is None and float(temperature) == 1.0 and not mask_vo:
            return None
        if not use_thres and pd_seed is None:
            raise ValueError("voice_thresholds / voice_max_count / temperature / mask_vo need decided hits: use_thres=False returns probabilities")
        th = voice_thresholds if voice_thresholds is not None else (0.0 if pd_seed is not None else thres)
        vs = _lib.make_voice_sampling(th, 32 if voice_max_count is None else voice_max_count, temperature, 0 if pd_seed is None else 1, mask_vo)
        if not all(0.0 <= t <= 1.0 for t in vs.thres):
            raise ValueError("voice thresholds must lie in [0, 1]: %s" % list(vs.thres))
        if not all(0 <= c <= 32 for c in vs.max_count):
            raise ValueError("voice_max_count must lie in 0..32: %s" % list(vs.max_count))
        if not (0.0 < vs.temperature < float("inf")):
            raise ValueError("temperature must be > 0 and finite, got %r" % (temperature,))
        return vs

    def predict(self, x, use_thres=True, thres=0.5, chunk=None, pd_seed=None, voice_thresholds=None, voice_max_count=None, temperature=1.0,
                mask_vo=False):
        """voice_thresholds / voice_max_count / temperature / mask_vo: the per-voice controls of gt_predict_voices (include/groove_hip.h);
        with all four at their defaults the call sequence is that of gt_predict / gt_predict_pd_at.  voice_thresholds="calibrated": the
        nine thresholds the last calibrate_thresholds stored (ValueError when there are none)."""
        voice_thresholds = self._calibrated(voice_thresholds)
        vs = self.voice_sampling(use_thres, thres, pd_seed, voice_thresholds, voice_max_count, temperature, mask_vo)
        out = self._predict(x, use_thres, thres, chunk, pd_seed, vs)
        # a timed-out exchange inside the call (its own workspaces): noticed when the call ends, the call repeated on the exchange-free schedule
        # (predict has no side effects; rank-local like an evaluation forward)
        bad = [(cfg, ws) for cfg, ws, _ in self._predict_ws.values()
               if self._xchg_word(ws, cfg) is not None and int(self._xchg_word(ws, cfg)[0].item()) != 0]
        if bad:
            for cfg, ws in bad:
                self.lib.call("gt_workspace_init", ctypes.byref(cfg), _ptr(ws), self.stream)

            def again():
                nonlocal out
                out = self._predict(x, use_thres, thres, chunk, pd_seed, vs)
            self._local_retry(None, None, "predict", again)
        self._trim_predict_ws()
        return out

    def _predict(self, x, use_thres=True, thres=0.5, chunk=None, pd_seed=None, vs=None):
        """model.predict for ANY batch size (ref:evaluator.py:173 passes the whole evaluation set at once):
        returns a (N,32,27) HVO tensor on the device ([h | v | o], one D2H for the evaluator).  The set is walked in chunks
        of `chunk` sequences (default: predict_chunk) over one cached workspace (sized for a chunk, not for N)."""
        x = torch.as_tensor(x, dtype=torch.float32).to(self.device).contiguous()
        n = x.shape[0]
        if chunk is None:
            chunk = self.predict_chunk(n)
        out = torch.empty(n, 32, 27, dtype=torch.float32, device=self.device)
        for i in range(0, n, chunk):
            m = min(chunk, n - i)
            cfg, ws, tgt = self._chunk_ws(m, chunk)
            if vs is not None:              # per-voice controls: the chunk's probabilities go to a buffer kept beside its workspace
                self.lib.call("gt_predict_voices", ctypes.byref(cfg), _ptr(self.params), _ptr(self.pe), _ptr(x[i:i + m]), _ptr(out[i:i + m]),
                              ctypes.byref(vs), ctypes.c_uint32(int(pd_seed or 0) & 0xFFFFFFFF), ctypes.c_int64(i),
                              _ptr(self._chunk_prob(m)), _ptr(tgt), _ptr(ws), self.stream)
                continue
            if pd_seed is not None:         # use_pd: hits sampled from the probabilities, hashed from the element's index in the WHOLE set
                self.lib.call("gt_predict_pd_at", ctypes.byref(cfg), _ptr(self.params), _ptr(self.pe), _ptr(x[i:i + m]), _ptr(out[i:i + m]),
                              ctypes.c_uint32(int(pd_seed) & 0xFFFFFFFF), ctypes.c_int64(i), _ptr(tgt), _ptr(ws), self.stream)
                continue
            self.lib.call("gt_predict", ctypes.byref(cfg), _ptr(self.params), _ptr(self.pe), _ptr(x[i:i + m]), _ptr(out[i:i + m]),
                          ctypes.c_float(thres), int(use_thres), _ptr(tgt), _ptr(ws), self.stream)
        return out

    def _chunk_ws(self, m, chunk):
        """(cfg, workspace, tgt scratch) of a predict call over m sequences, cached in _predict_ws: the full chunk + one remainder size at most"""
        d = self.dims
        if self._predict_epoch != self.lib.cdll.gt_layout_epoch():      # (a layout switch changed: see slot())
            self._predict_ws.clear()
            self._predict_epoch = self.lib.cdll.gt_layout_epoch()
        if m not in self._predict_ws:
            if len(self._predict_ws) >= 2:
                self._predict_ws.pop(next(k for k in self._predict_ws if k != chunk), None)
            cfg = _lib.make_config(m, d["embedding_size_src"], d["d_model"], d["n_heads"], d["dim_feedforward"],
                                   d["num_encoder_layers"], d["num_decoder_layers"], d["dropout"], d["precision"], self.cfg_flags)
            ws = torch.empty(self.lib.workspace_floats(cfg), dtype=torch.float32, device=self.device)
            self.lib.call("gt_workspace_init", ctypes.byref(cfg), _ptr(ws), self.stream)
            tgt = torch.empty(m, 32, 27, dtype=torch.float32, device=self.device) if not self.encoder_only else None
            self._predict_ws[m] = (cfg, ws, tgt)
        return self._predict_ws[m]

    def _chunk_prob(self, m):
        """the (m,32,9) probability buffer kept beside the workspace of chunk size m"""
        self._predict_prob = {k: v for k, v in self._predict_prob.items() if k in self._predict_ws}
        if m not in self._predict_prob:
            self._predict_prob[m] = torch.empty(m, 32, 9, dtype=torch.float32, device=self.device)
        return self._predict_prob[m]

    def _calibrated(self, voice_thresholds):
        """voice_thresholds="calibrated": the nine thresholds calibrate_thresholds stored on this engine"""
        if isinstance(voice_thresholds, str):
            if voice_thresholds != "calibrated":
                raise ValueError("voice_thresholds must be 9 values or \"calibrated\", got %r" % (voice_thresholds,))
            if self.voice_thresholds is None:
                raise ValueError("voice_thresholds=\"calibrated\" needs thresholds: run calibrate_thresholds first (or load a checkpoint that carries them)")
            return list(self.voice_thresholds)
        return voice_thresholds

    DEFAULT_CURVE_GRID = tuple(float(np.float32(k) / np.float32(100)) for k in range(1, 100))

    def hit_curve(self, x, gt_hvo, grid=None, temperature=1.0, voice_thresholds=None, chunk=None, counts=None):
        """Per-voice threshold curves of a whole set on the device (gt_hit_curve; include/groove_hip.h): for each voice and class (the ground
        truth is a hit / is not), how many predicted probabilities fall into each bin of `grid` (K ascending thresholds in [0,1]; default
        float32(k) / float32(100), k = 1..99) -> device int64 tensor (9, 2, K + 1).  The set is walked in predict's chunks over predict's
        cached workspaces; nothing is copied to the host per chunk.  counts: an earlier result over the same grid to continue (it is
        added to in place; counts of disjoint shards add, which is all a data-parallel evaluation needs).
        Encoder-only at temperature 1: gt_predict(use_thres = 0) per chunk, its hit columns read in place; otherwise gt_predict_voices and
        its prob_out.  Encoder-decoder: the probabilities are those ALONG THE GREEDY DECODE at the starting thresholds (voice_thresholds,
        default 0.5) -- the decode feeds decided hits back, so another threshold would have met other probabilities from its first
        differing step on; the curve approximates what a changed threshold does."""
        x = torch.as_tensor(x, dtype=torch.float32).to(self.device).contiguous()
        gt = torch.as_tensor(gt_hvo, dtype=torch.float32).to(self.device).contiguous()
        n = x.shape[0]
        if n < 1 or gt.numel() != n * 32 * 27:
            raise ValueError("hit_curve needs x (N,32,S) and gt_hvo (N,32,27) with N >= 1, got %s / %s" % (tuple(x.shape), tuple(gt.shape)))
        grid = [float(np.float32(t)) for t in (self.DEFAULT_CURVE_GRID if grid is None else grid)]
        k = len(grid)
        if not 1 <= k <= _lib.CURVE_MAX_THRES or not all(0.0 <= t <= 1.0 for t in grid) or any(b <= a for a, b in zip(grid, grid[1:])):
            raise ValueError("grid: 1..%d strictly ascending thresholds in [0, 1], got %r" % (_lib.CURVE_MAX_THRES, grid))
        plain = self.encoder_only and float(temperature) == 1.0
        vs = None
        if not plain:
            th = self._calibrated(voice_thresholds)
            vs = self.voice_sampling(True, 0.5, None, [0.5] * 9 if th is None else th, None, temperature, False)
        if counts is None:
            counts = torch.zeros(9, 2, k + 1, dtype=torch.int64, device=self.device)
        elif tuple(counts.shape) != (9, 2, k + 1) or counts.dtype != torch.int64 or not counts.is_contiguous() or counts.device != x.device:
            raise ValueError("counts must be a contiguous int64 tensor (9, 2, %d) on %s" % (k + 1, self.device))
        if chunk is None:
            chunk = self.predict_chunk(n)
        cgrid = (ctypes.c_float * k)(*grid)
        before = counts.clone()

        def walk():
            for i in range(0, n, chunk):
                m = min(chunk, n - i)
                cfg, ws, tgt = self._chunk_ws(m, chunk)
                if m not in self._curve_buf:
                    self._curve_buf = {q: v for q, v in self._curve_buf.items() if q in self._predict_ws}
                    words = int(self.lib.cdll.gt_hit_curve_scratch_words(ctypes.c_int64(m * 32), _lib.CURVE_MAX_THRES))
                    self._curve_buf[m] = (torch.empty(m, 32, 27, dtype=torch.float32, device=self.device),
                                          torch.empty(words, dtype=torch.int32, device=self.device))
                hvo, scratch = self._curve_buf[m]
                if plain:
                    self.lib.call("gt_predict", ctypes.byref(cfg), _ptr(self.params), _ptr(self.pe), _ptr(x[i:i + m]), _ptr(hvo),
                                  ctypes.c_float(0.5), 0, _ptr(tgt), _ptr(ws), self.stream)
                    prob, stride = hvo, 27
                else:
                    prob, stride = self._chunk_prob(m), 9
                    self.lib.call("gt_predict_voices", ctypes.byref(cfg), _ptr(self.params), _ptr(self.pe), _ptr(x[i:i + m]), _ptr(hvo),
                                  ctypes.byref(vs), ctypes.c_uint32(0), ctypes.c_int64(i), _ptr(prob), _ptr(tgt), _ptr(ws), self.stream)
                self.lib.call("gt_hit_curve", _ptr(prob), stride, _ptr(gt[i:i + m]), ctypes.c_int64(m * 32), cgrid, k, _ptr(counts),
                              _ptr(scratch), self.stream)

        walk()
        # a timed-out exchange inside the walk: as in predict, noticed when the walk ends; the counts go back to what they were and the
        # walk is repeated on the exchange-free schedule
        bad = [(cfg, ws) for cfg, ws, _ in self._predict_ws.values()
               if self._xchg_word(ws, cfg) is not None and int(self._xchg_word(ws, cfg)[0].item()) != 0]
        if bad:
            for cfg, ws in bad:
                self.lib.call("gt_workspace_init", ctypes.byref(cfg), _ptr(ws), self.stream)

            def again():
                counts.copy_(before)
                walk()
            self._local_retry(None, None, "hit_curve", again)
        self._trim_predict_ws()
        self._curve_buf = {q: v for q, v in self._curve_buf.items() if q in self._predict_ws}
        return counts

    def group_metrics(self, hvo_pred, hvo_gt, groups=None, n_groups=None, cells=None, removed=None, acc=None, seq_counts=False, chunk=None):
        """Per-group evaluation counts of predictions against ground truth, both (N,32,27) HVO tensors (gt_group_metrics;
        include/groove_hip.h) -> device int64 tensor of GT_GM_ACC_WORDS(n_groups) words; with seq_counts=True also the (N,4) int32 counts
        (counted cells, TP, FP, FN per sequence).  groups: N integer tags (None: every sequence in group 0); a tag outside 0..n_groups - 1
        skips its sequence.  n_groups: default the largest tag + 1 (one host read), 1 without groups.  The mask of the cells that count --
        at most one of: cells, the (N,9) int32 / uint32 bit words of gather_events or an (N,32,9) bool tensor; removed, the (N,) int32
        voice bitmasks of gather (each removed voice counts whole).  acc: an earlier result over the same n_groups to continue (it is
        added to in place; counts of disjoint shards add).  chunk: sequences per call (default: all, below the call's 2^26)."""
        from . import infill
        p = torch.as_tensor(hvo_pred, dtype=torch.float32).to(self.device).contiguous()
        g = torch.as_tensor(hvo_gt, dtype=torch.float32).to(self.device).contiguous()
        if p.shape != g.shape or p.shape[-1] != 27 or p.numel() % (32 * 27) or p.numel() == 0:
            raise ValueError("group_metrics needs two (N,32,27) HVO tensors with N >= 1, got %s / %s" % (tuple(p.shape), tuple(g.shape)))
        n = p.numel() // (32 * 27)
        if cells is not None and removed is not None:
            raise ValueError("group_metrics takes cells (a mask per cell) or removed (a bitmask of voices per sequence), not both")
        if removed is not None:
            removed = torch.as_tensor(removed).to(self.device, torch.int32).reshape(-1)
            if removed.numel() != n:
                raise ValueError("removed needs one bitmask per sequence (%d), got %d" % (n, removed.numel()))
            bit = (removed.view(n, 1) >> torch.arange(_lib.GT_VOICES, device=self.device, dtype=torch.int32).view(1, -1)) & 1
            cells = (-bit).to(torch.int32).contiguous()                      # a removed voice: the all-ones word
        elif cells is not None:
            cells = infill.cell_words(cells, n, self.device)
        if groups is not None:
            groups = torch.as_tensor(groups).to(self.device, torch.int32).reshape(-1).contiguous()
            if groups.numel() != n:
                raise ValueError("groups needs one tag per sequence (%d), got %d" % (n, groups.numel()))
        if n_groups is None:
            n_groups = 1 if groups is None else max(1, int(groups.max().item()) + 1)
        n_groups = int(n_groups)
        if not 1 <= n_groups <= _lib.GM_MAX_GROUPS:
            raise ValueError("n_groups must lie in 1..%d, got %d" % (_lib.GM_MAX_GROUPS, n_groups))
        words = _lib.gm_acc_words(n_groups)
        if acc is None:
            acc = torch.zeros(words, dtype=torch.int64, device=self.device)
        elif tuple(acc.shape) != (words,) or acc.dtype != torch.int64 or not acc.is_contiguous() or acc.device != p.device:
            raise ValueError("acc must be a contiguous int64 tensor (%d,) on %s" % (words, self.device))
        seq = torch.empty(n, 4, dtype=torch.int32, device=self.device) if seq_counts else None
        chunk = min(n, (1 << 26) - 1) if chunk is None else max(1, min(int(chunk), (1 << 26) - 1))
        scratch = torch.empty(int(self.lib.cdll.gt_group_metrics_scratch_words(ctypes.c_int64(min(chunk, n)), n_groups)), dtype=torch.int64,
                              device=self.device)
        p, g = p.view(n, 32, 27), g.view(n, 32, 27)
        for i in range(0, n, chunk):
            m = min(chunk, n - i)                                            # (a shorter tail needs no more scratch: the size grows with m)
            self.lib.call("gt_group_metrics", _ptr(p[i:i + m]), _ptr(g[i:i + m]), _ptr(groups[i:i + m]) if groups is not None else None,
                          _ptr(cells[i:i + m]) if cells is not None else None, ctypes.c_int64(m), n_groups, _ptr(acc),
                          _ptr(seq[i:i + m]) if seq is not None else None, _ptr(scratch), self.stream)
        return (acc, seq) if seq_counts else acc

    def groove_features(self, hvo_a, hvo_b=None, feat_b=True, pair=True, chunk=None):
        """Groove descriptors and rhythmic distances per sequence (gt_groove_features; include/groove_hip.h): the integer record of every
        sequence of hvo_a (N,32,27) -> device int64 tensor (N,32).  With hvo_b (the same shape): also its records (N,32) (feat_b=True) and
        the words that compare a with b, (N,8) (pair=True) -- returned as a tuple in that order, each only where asked for (a ground
        truth whose record is already known: feat_b=False).  Every word is stored by the call: nothing to zero, no scratch.
        chunk: sequences per call (default: all, below the call's 2^26)."""
        a = torch.as_tensor(hvo_a, dtype=torch.float32).to(self.device).contiguous()
        if a.shape[-1] != 27 or a.numel() % (32 * 27) or a.numel() == 0:
            raise ValueError("groove_features needs an (N,32,27) HVO tensor with N >= 1, got %s" % (tuple(a.shape),))
        n = a.numel() // (32 * 27)
        a = a.view(n, 32, 27)
        b = None
        if hvo_b is not None:
            b = torch.as_tensor(hvo_b, dtype=torch.float32).to(self.device).contiguous()
            if b.numel() != a.numel() or b.shape[-1] != 27:
                raise ValueError("groove_features needs two HVO tensors of one shape, got %s / %s" % (tuple(a.shape), tuple(b.shape)))
            b = b.view(n, 32, 27)
        want_fb, want_pair = b is not None and bool(feat_b), b is not None and bool(pair)
        fa = torch.empty(n, _lib.GF_WORDS, dtype=torch.int64, device=self.device)
        fb = torch.empty(n, _lib.GF_WORDS, dtype=torch.int64, device=self.device) if want_fb else None
        pw = torch.empty(n, _lib.GF_PAIR_WORDS, dtype=torch.int64, device=self.device) if want_pair else None
        chunk = min(n, (1 << 26) - 1) if chunk is None else max(1, min(int(chunk), (1 << 26) - 1))
        for i in range(0, n, chunk):
            m = min(chunk, n - i)
            self.lib.call("gt_groove_features", _ptr(a[i:i + m]), _ptr(b[i:i + m]) if (want_fb or want_pair) else None, ctypes.c_int64(m),
                          _ptr(fa[i:i + m]), _ptr(fb[i:i + m]) if want_fb else None, _ptr(pw[i:i + m]) if want_pair else None, self.stream)
        out = (fa,) + ((fb,) if want_fb else ()) + ((pw,) if want_pair else ())
        return out[0] if len(out) == 1 else out

    def _trim_predict_ws(self):
        for m in [k for k, (_, ws, _) in self._predict_ws.items() if 4 * ws.numel() > PREDICT_WS_KEEP]:
            del self._predict_ws[m]               # (stream-ordered free: the caching allocator keeps the block until the launches ran)

    # ---- in-launch exchanges (QUAD pair exchange, LayerNorm row exchange): what happens when partner workgroups were not co-resident ------
    # The exchanges poll with a bound (csrc/gt_seq.h seq_xchg_get, csrc/gt_gemm64.h g64_collect); a workgroup that gives its partner up raises
    # the error word at the head of the slot's exchange region and goes on with garbage.  Device side, every update that knows the workspace
    # refuses to apply anything while the word is set (parameters, moments and Adam's t untouched, gradients cleared, the skip COUNTED in word 1
    # of the region's header) -- and, data-parallel, while the all-reduced guard element is non-zero, so every rank skips together.
    # Host side, single process: the two words are read (a) asynchronously from the first train step of a slot on and then every
    # XCHG_POLL_EVERY-th (poll_exchange: an 8-byte copy into pinned memory, looked at one poll later -- no synchronisation on the step path),
    # (b) wherever the host synchronises anyway: mean_stats (the logging path), eval forwards, predict.  On a set word the engine zeroes the
    # region, falls back to the exchange-free schedules for the rest of ITS life (gt_config.flags of its own configurations: same numbers, no
    # in-launch exchange -- other engines of the process are not touched), drops its captured graphs and warns -- or raises, with
    # GT_XCHG_STRICT=1.  The steps in between were skipped, never applied; exchange_timeouts / skipped_updates say how many.
    # Multi-rank: a recovery changes the launch sequence and re-captures graphs -- the one-hipGraph recipe's capture runs a real warm-up step
    # with collectives -- so it must happen on the SAME step on every rank: it is decided only from values every rank holds identically (the
    # all-reduced guard element, read on the same step count and waited for; the flag inside mean_stats' / check_exchange's all-reduce).
    # Rank-local observations (an evaluation forward or predict on one rank) repeat their own call on borrowed flags and change nothing else.
    FALLBACK_FLAGS = _lib.CFG_NO_QUAD | _lib.CFG_NO_LN_XCHG

    def _xchg_word(self, s_or_ws, cfg=None):
        """2-element int32 view [error word, skipped updates] of a slot (or of a (cfg, workspace) pair), None when the shape has no
        exchange region."""
        if cfg is None:
            s = s_or_ws
            if s.xchg_off is None:
                try:
                    s.xchg_off = self.lib.ws_find(s.cfg, "xchg_err")[0]
                except Exception:
                    s.xchg_off = -1
            return s.ws[s.xchg_off:s.xchg_off + 2].view(torch.int32) if s.xchg_off >= 0 else None
        try:
            off = self.lib.ws_find(cfg, "xchg_err")[0]
        except Exception:
            return None
        return s_or_ws[off:off + 2].view(torch.int32) if off >= 0 else None

    def _guard_fn(self, s):
        """Data-parallel: before the gradient all-reduce every rank writes its error flag into the guard element (the last float of the
        gradient buffer: padding behind the 27-float output bias); the update kernel of EVERY rank skips when the sum is non-zero."""
        if self._xchg_word(s) is None:
            return lambda: None
        return lambda: self.lib.call("gt_dp_guard", ctypes.byref(s.cfg), _ptr(self.grads), _ptr(s.ws), self.stream)      # (one 1-thread launch)

    def _timeout_message(self, what):
        return ("an in-launch exchange (four-workgroups-per-sequence pair exchange / LayerNorm row exchange) timed out during %s (partner "
                "workgroups not co-resident: another stream / process holds CUs?)" % what)

    def _local_retry(self, ws, cfg, what, again):
        """A rank-local time-out in a call without side effects (evaluation forward, predict): zero the region, repeat the call on the
        exchange-free schedule.  Single process: that schedule stays (a full recovery).  Multi-rank: the flags are borrowed for the repeat
        alone -- the training schedule, its graphs and the other ranks are not touched."""
        self.exchange_timeouts += 1
        if self.xchg_strict:
            raise RuntimeError(self._timeout_message(what) + "; GT_XCHG_STRICT=1")
        if self.world_size == 1:
            self.exchange_timeouts -= 1            # (counted by _recover_exchange)
            self._recover_exchange(ws, cfg, what)
            again()
            return
        warnings.warn(self._timeout_message(what) + " -- repeated on the exchange-free schedule (this call only)", RuntimeWarning)
        if ws is not None:
            self.lib.call("gt_workspace_init", ctypes.byref(cfg), _ptr(ws), self.stream)
        keep = (self._flags_fallback, [(t, dict(t.graphs), dict(t.keep), t.use_graph) for t in self._slots.values()])
        self._flags_fallback = self.FALLBACK_FLAGS
        try:
            self._apply_flags()
            again()
        finally:
            self._flags_fallback = keep[0]
            self._apply_flags()
            for t, g, k, u in keep[1]:             # (the training graphs were recorded under the flags now back in force)
                t.graphs, t.keep, t.use_graph = g, k, u

    def _recover_exchange(self, ws, cfg, what):
        """Fall back to the exchange-free schedules for the rest of this engine's life.  Multi-rank: call it on EVERY rank on the same step."""
        self.exchange_timeouts += 1
        if self.xchg_strict:
            raise RuntimeError(self._timeout_message(what) + "; GT_XCHG_STRICT=1")
        for t in self._slots.values():             # the device's own count, before the regions are zeroed
            w = self._xchg_word(t)
            if w is not None:
                self.skipped_updates += int(w[1].item()) - t.xchg_skipped_seen
                t.xchg_skipped_seen = 0
        warnings.warn(self._timeout_message(what) + " -- the affected updates were skipped on the device (%d so far); falling back to the "
                      "exchange-free schedules for the rest of this engine's life" % self.skipped_updates, RuntimeWarning)
        self._flags_fallback = self.FALLBACK_FLAGS
        self._apply_flags()                        # (drops the captured graphs: they hold the exchanging launches)
        if ws is not None:
            self.lib.call("gt_workspace_init", ctypes.byref(cfg), _ptr(ws), self.stream)      # (zeroes the region: stale granules, the words)
        for t in self._slots.values():
            t.graphs.clear(); t.keep.clear(); t.use_graph = None
            t.xchg_host = None
            if t.ws is not ws and self._xchg_word(t) is not None:
                self.lib.call("gt_workspace_init", ctypes.byref(t.cfg), _ptr(t.ws), self.stream)
        self.grads[self.total - 1:].zero_()

    def poll_exchange(self, s):
        """Step path, no host-side wait in a single process: the slot's first call and then every XCHG_POLL_EVERY-th look at the PREVIOUS
        asynchronous copy of [error word, skipped updates] (complete by now, or left for the next poll) and start the next one.
        Multi-rank: the copy is of the ALL-REDUCED guard element (identical on every rank) and the look WAITS for it, so every rank decides
        on the same step from the same value (the copy is XCHG_POLL_EVERY steps old: the wait only bounds how far the host runs ahead)."""
        s.xchg_count += 1
        if s.xchg_count != 1 and s.xchg_count % XCHG_POLL_EVERY:
            return
        w = self._xchg_word(s)
        if w is None:
            return
        multi = self.world_size > 1
        if self.on_host:                            # (host emulator: no streams -- read in place; multi-rank tests over gloo)
            flag = float(self.grads[self.total - 1]) != 0.0 if multi else int(w[0]) != 0
            if flag:
                self._recover_exchange(s.ws, s.cfg, "a train step")
            return
        src = self.grads[self.total - 1:].view(torch.int32) if multi else w
        if s.xchg_host is None:
            s.xchg_host = torch.zeros(src.numel(), dtype=torch.int32).pin_memory()
            s.xchg_event = torch.cuda.Event()
        else:
            if multi:
                s.xchg_event.synchronize()
            elif not s.xchg_event.query():
                return                              # (the last copy is still in flight: look again next time)
            if int(s.xchg_host[0]) != 0:
                s.xchg_host.zero_()
                self._recover_exchange(s.ws, s.cfg, "a train step")
                return
            if not multi:
                seen = int(s.xchg_host[1])
                self.skipped_updates += seen - s.xchg_skipped_seen
                s.xchg_skipped_seen = seen
        s.xchg_host.copy_(src, non_blocking=True)
        s.xchg_event.record(torch.cuda.current_stream(self.device))

    def check_exchange(self, s, what="a train step"):
        """Synchronising read of slot s's error word (call where the host waits for the device anyway).  -> True when a time-out was found
        (and recovered from: the numbers of the launches since the last check are garbage, their updates were skipped).  Multi-rank: a
        COLLECTIVE -- every rank must call it at the same point (the flag is all-reduced, every rank recovers or none does)."""
        w = self._xchg_word(s)
        if self.world_size > 1:
            import torch.distributed as dist
            flag = torch.zeros(1, dtype=torch.float32, device=s.stats.device) if w is None else (w[:1] != 0).to(torch.float32)
            dist.all_reduce(flag)
            if float(flag) == 0.0:
                return False
            self._recover_exchange(s.ws, s.cfg, what + " (some rank)")
            return True
        if w is None or int(w[0].item()) == 0:
            return False
        self._recover_exchange(s.ws, s.cfg, what)
        return True

    def exchange_report(self, s=None):
        """{"exchange_timeouts", "skipped_updates"} up to now (synchronising: adds what the device counted since the last look)."""
        n = self.skipped_updates
        for t in ([s] if s is not None else list(self._slots.values())):
            w = self._xchg_word(t)
            if w is not None:
                n += int(w[1].item()) - t.xchg_skipped_seen
        return {"exchange_timeouts": self.exchange_timeouts, "skipped_updates": n}

    def mean_stats(self, s):
        """The slot's 8-float stats averaged over the data-parallel ranks (one tiny all-reduce; every rank must call it).
        Single process: the stats tensor itself.  Also the synchronising check of the exchanges: stats of a step whose exchange timed
        out come back as NaN (data-parallel: on every rank -- the flag travels with the stats all-reduce, so all ranks fall back together)."""
        if self.world_size == 1 or not self.reduce_stats:
            if self.world_size == 1 and self.check_exchange(s):
                return torch.full_like(s.stats, float("nan"))
            return s.stats
        import torch.distributed as dist
        w = self._xchg_word(s)
        flag = torch.zeros(1, dtype=torch.float32, device=s.stats.device) if w is None else (w[:1] != 0).to(torch.float32)
        t = torch.cat([s.stats, flag])
        dist.all_reduce(t)
        if float(t[8]) != 0.0:
            self._recover_exchange(s.ws, s.cfg, "a train step (some rank)")     # (ranks whose own word is clean fall back too: one schedule everywhere)
            return torch.full_like(s.stats, float("nan"))
        return t[:8] / self.world_size

    def mean_voice_stats(self, s):
        """The slot's 36 per-voice statistics of the last step with loss options (gt_loss_opts: [0..9) bce, [9..18) mse_v, [18..27) mse_o
        shares, [27..36) hit accuracy per voice), averaged over the data-parallel ranks like mean_stats (every rank must call it)."""
        if s.voice_stats is None:                  # (no step with options ran on this slot yet)
            self._loss_ready(s, self.loss_opts or self.make_loss_opts())
        if self.world_size == 1 or not self.reduce_stats:
            return s.voice_stats
        import torch.distributed as dist
        t = s.voice_stats.clone()
        dist.all_reduce(t)
        return t / self.world_size

    def profile(self, steps):
        """Eager (no graph) pass of `steps` train steps with HIP events around every launch.
        -> {kernel class: (launches, total_ms, total_flops, total_bytes)}.  Measurement aid for bench.py."""
        if self.on_host:
            return {}
        s = self.slot(self.B)
        snap = (self.params.clone(), self.state.clone(), None if self.m is None else (self.m.clone(), self.v.clone()))
        torch.cuda.synchronize(self.device)
        self.lib.cdll.gt_profile_enable(1)
        try:
            for _ in range(steps):
                self._enqueue_step(s, 0)
            buf = ctypes.create_string_buffer(1 << 16)
            self.lib.cdll.gt_profile_report(buf, len(buf), 256)
        finally:
            self.lib.cdll.gt_profile_enable(0)
        self.params.copy_(snap[0]); self.state.copy_(snap[1]); self.grads.zero_()
        if snap[2] is not None:
            self.m.copy_(snap[2][0]); self.v.copy_(snap[2][1])
        out = {}
        for line in buf.value.decode().splitlines():
            lab, cnt, ms, fl, by = line.split()
            out[lab] = (int(cnt), float(ms), float(fl), float(by))
        return out
