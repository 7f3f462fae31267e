"""initialize_model / calculate_loss / train_loop: the three names the reference imports from its
un-vendored submodule (ref:train.py:12), with the call signatures the reference uses
(ref:train.py:149,195-215; ref:tutorial.py:62-68,98-105), running on the HIP hot path.

Checkpoints keep the reference's layout: ``{epoch, model_state_dict, optimizer_state_dict, loss}`` in a file
``transformer_run_{run}_Epoch_{epoch}.Model`` (ckpt keys; pattern ref:tutorial.py:65), and
``params["load_model"]`` = ``{location: local|wandb, dir, file_pattern, epoch, run}`` resumes from one.
"""
import glob
import math
import os
import re

import torch

from . import _lib
from .model import GrooveTransformer, GrooveTransformerEncoder, _GrooveBase, engine_of

try:                                    # Weights & Biases is optional here (ref:train.py:106-113,150,252)
    import wandb
except Exception:                       # pragma: no cover - not installed in the build container
    wandb = None


def _wandb_active():
    return wandb is not None and getattr(wandb, "run", None) is not None


# ------------------------------------------------------------------------------------------------ optimizers
class _FusedMixin:
    """torch.optim-compatible front of the fused flat update (one kernel over all tensors).  Keeps torch's
    state_dict format: SGD -> per-param {'momentum_buffer': None | tensor} (ckpt); Adam / AdamW -> step/exp_avg/exp_avg_sq.

    Hyper-parameters: param_groups[0] is the source of truth (one group: the flat buffers have one set).  lr, momentum, nesterov and
    weight_decay are pushed to the engine by every step() and at the head of train_loop's fast path, so editing param_groups between
    steps takes effect.  dampening != 0, amsgrad and maximize have no kernel and raise ValueError.

    ONE deviation from torch: momentum, Nesterov and weight decay run as a pass over the gradient buffer in front of the update, so after
    step() the .grad views hold the TRANSFORMED gradient (weight decay added, the momentum step) until zero_grad(); torch leaves .grad as
    backward wrote it.  (AdamW decays the parameters and leaves the gradients alone.)"""

    def _bind(self, engine, algo, decoupled=False):
        self.engine = engine
        self._algo, self._decoupled = algo, decoupled
        engine.algo, engine.decoupled = algo, decoupled
        engine._fused_opt = True           # (the update kernel honours the exchange error word: engine.backward need not zero gradients)
        self._lr_on_device = None
        self._push_lr()

    def zero_grad(self, set_to_none=False):
        self.engine.grads.zero_()

    def _push_lr(self):
        """lr into the device step state (when it changed) and the other hyper-parameters of param_groups[0] into the engine"""
        g = self.param_groups[0]
        for k in ("dampening", "amsgrad", "maximize"):
            if g.get(k):
                raise ValueError("%s: %s=%r is not supported by the fused update" % (type(self).__name__, k, g[k]))
        lr = float(g["lr"])
        if lr != self._lr_on_device:
            self.engine.set_state(lr=lr)
            self._lr_on_device = lr
        eng = self.engine
        eng.algo, eng.decoupled = self._algo, self._decoupled
        eng.weight_decay, eng.momentum, eng.nesterov = float(g.get("weight_decay", 0.0)), float(g.get("momentum", 0.0)), bool(g.get("nesterov", False))
        eng._opt_extras()                  # (validates; allocates the momentum buffers when momentum is first non-zero)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self._push_lr()
        self.engine.enqueue_update(zero_grads=False)
        return loss


class GrooveSGD(_FusedMixin, torch.optim.SGD):
    """torch.optim.SGD(lr, momentum, nesterov, weight_decay) semantics with dampening 0 (ckpt: optimizer param_groups; the reference's
    momentum=0 is the default) on the fused kernels.  state[p]["momentum_buffer"] is a view into the engine's flat momentum buffer while
    momentum is non-zero (zeros before the first step: torch's buf = grad), else None as in the demo checkpoint.  See _FusedMixin for the one
    deviation from torch (.grad after step())."""

    def __init__(self, params, lr, engine, momentum=0, nesterov=False, weight_decay=0, dampening=0, maximize=False):
        if dampening != 0 or maximize:
            raise ValueError("GrooveSGD: dampening and maximize are not supported by the fused update")
        torch.optim.SGD.__init__(self, params, lr=lr, momentum=momentum, nesterov=nesterov, weight_decay=weight_decay)
        self._bind(engine, 0)

    def _push_lr(self):
        _FusedMixin._push_lr(self)
        eng = self.engine
        ps = self.param_groups[0]["params"]
        cur = self.state[ps[0]].get("momentum_buffer", False)       # (False: not set yet)
        if eng.momentum == 0.0:
            if cur is not None:
                for p in ps:
                    self.state[p]["momentum_buffer"] = None
        elif cur is None or cur is False:
            mb = eng.views(eng.mbuf)
            by_ptr = {t.data_ptr(): n for n, t in eng.views().items()}
            for p in ps:
                self.state[p]["momentum_buffer"] = mb[by_ptr[p.data_ptr()]]

    def load_state_dict(self, sd):
        """lr from the checkpoint; momentum / nesterov / weight_decay stay this run's.  Stored momentum buffers are copied into the engine's
        flat buffer; None (a momentum-free run's or a reference-written checkpoint) resumes a momentum run from zeros."""
        self.param_groups[0]["lr"] = sd["param_groups"][0]["lr"]
        self._push_lr()
        for i, p in enumerate(self.param_groups[0]["params"]):
            buf = (sd["state"].get(i) or {}).get("momentum_buffer")
            mine = self.state[p]["momentum_buffer"]
            if mine is not None:
                mine.zero_() if buf is None else mine.copy_(buf)


class GrooveAdam(_FusedMixin, torch.optim.Adam):
    """torch.optim.Adam(lr, weight_decay) (L2: the decay is added to the gradient); exp_avg / exp_avg_sq are views into the engine's flat
    moment buffers.  See _FusedMixin for the one deviation from torch (.grad after step())."""
    _base, _decoupled_decay = torch.optim.Adam, False

    def __init__(self, params, lr, engine, weight_decay=None, amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise ValueError("%s: amsgrad and maximize are not supported by the fused update" % type(self).__name__)
        kw = {} if weight_decay is None else {"weight_decay": weight_decay}          # (None: torch's default -- 0 for Adam, 1e-2 for AdamW)
        self._base.__init__(self, params, lr=lr, **kw)
        engine.ensure_adam()
        self._bind(engine, 1, self._decoupled_decay)
        m, v = engine.views(engine.m), engine.views(engine.v)
        by_ptr = {t.data_ptr(): n for n, t in engine.views().items()}
        for p in self.param_groups[0]["params"]:
            n = by_ptr[p.data_ptr()]
            self.state[p] = {"step": torch.tensor(0.0), "exp_avg": m[n], "exp_avg_sq": v[n]}

    @torch.no_grad()
    def step(self, closure=None):
        out = _FusedMixin.step(self, closure)
        for st in self.state.values():
            st["step"] += 1
        return out

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        self.param_groups[0]["lr"] = groups[0]["lr"]
        params = self.param_groups[0]["params"]
        steps = 0
        for i, p in enumerate(params):
            st = sd["state"].get(i)
            if st:
                self.state[p]["exp_avg"].copy_(st["exp_avg"])
                self.state[p]["exp_avg_sq"].copy_(st["exp_avg_sq"])
                self.state[p]["step"] = torch.as_tensor(float(st["step"]))
                steps = int(st["step"])
        self.engine.set_state(opt_step=steps)


class GrooveAdamW(GrooveAdam, torch.optim.AdamW):
    """torch.optim.AdamW(lr, weight_decay=1e-2): the parameters are decayed by 1 - lr * weight_decay in front of the Adam update."""
    _base, _decoupled_decay = torch.optim.AdamW, True


# ------------------------------------------------------------------------------------------------ checkpoints
FILE_PATTERN = "transformer_run_{}_Epoch_{}.Model"


def save_checkpoint(path, epoch, model, optimizer, loss):
    """Exactly the reference's four keys (ckpt).  The position of this replica's dropout stream rides in
    ``optimizer_state_dict["param_groups"][0]["dropout_step"]`` (torch optimizers keep unknown group keys), so a resumed
    run continues with fresh masks instead of replaying the ones of step 0."""
    osd = optimizer.state_dict()
    eng = getattr(model, "engine", None)
    if eng is not None and osd.get("param_groups"):
        osd["param_groups"][0]["dropout_step"] = max(int(eng.state_struct().step), int(getattr(model, "_train_forwards", 0)))
        # calibrated hit thresholds (model.calibrate_thresholds) ride beside it; a model without them writes no such key
        if getattr(model, "voice_thresholds", None) is not None:
            osd["param_groups"][0]["voice_thresholds"] = [float(t) for t in model.voice_thresholds]
    torch.save({"epoch": epoch, "model_state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()},
                "optimizer_state_dict": osd, "loss": float(loss)}, path)
    return path


def find_checkpoint(load_model):
    """load_model = {location, dir, file_pattern, [epoch], [run]} (ref:tutorial.py:62-66,98-104).
    Without 'epoch' the last stored epoch is used (ref:tutorial.py:36)."""
    loc = load_model.get("location", "local")
    if loc == "wandb":
        if wandb is None:
            raise RuntimeError("load_model.location == 'wandb' needs the wandb package")
        ep = load_model["epoch"]
        f = wandb.restore(load_model["file_pattern"].format(load_model["run"], ep), run_path=load_model["dir"])
        return f.name
    d, pat = load_model["dir"], load_model["file_pattern"]
    if load_model.get("epoch") is not None:
        cands = glob.glob(os.path.join(d, pat.format(load_model.get("run", "*"), load_model["epoch"])))
        if not cands:
            raise FileNotFoundError("no checkpoint for epoch %s in %s" % (load_model["epoch"], d))
        return sorted(cands)[-1]
    rx = re.compile(re.escape(pat).replace(r"\{\}", "(.+)", 1).replace(r"\{\}", r"(\d+)", 1) + "$")
    best = None
    for f in glob.glob(os.path.join(d, pat.format(load_model.get("run", "*"), "*"))):
        m = rx.match(os.path.basename(f))
        if m and (best is None or int(m.group(2)) > best[0]):
            best = (int(m.group(2)), f)
    if best is None:
        raise FileNotFoundError("no checkpoint matching %s in %s" % (pat, d))
    return best[1]


# ------------------------------------------------------------------------------------------------ initialize_model
def initialize_model(params):
    """params = {"model": {...}, "training": {...}, "load_model": None | {...}} (ref:train.py:115-143).
    -> (model, optimizer, initial_epoch)."""
    mp, tp = params["model"], params["training"]
    common = dict(d_model=mp["d_model"], nhead=mp["n_heads"], dim_feedforward=mp["dim_feedforward"],
                  dropout=mp["dropout"], embedding_size_src=mp["embedding_size_src"],
                  embedding_size_tgt=mp["embedding_size_tgt"], max_len=mp["max_len"], device=mp.get("device", "cuda"),
                  seed=int(params.get("seed", tp.get("seed", 0)) or 0),      # dropout stream (train.py --seed); rank mixed in by the model
                  precision=mp.get("precision", "fp32"))                     # "bf16": GEMM operands in bf16 (BASELINE configs[4]); "autocast": ... and bf16 storage of the Linear outputs (precision 2)
    if mp["encoder_only"]:
        model = GrooveTransformerEncoder(num_encoder_layers=mp["num_encoder_layers"], **common)
    else:
        model = GrooveTransformer(num_encoder_layers=mp["num_encoder_layers"],
                                  num_decoder_layers=mp["num_decoder_layers"], **common)
    lr = tp["learning_rate"]
    algo = str(mp.get("optimizer", "sgd")).lower()
    # not in the reference (its YAMLs lack the keys: plain SGD / Adam, as there): training.momentum / nesterov / weight_decay, and "adamw"
    wd, mom, nest = tp.get("weight_decay"), tp.get("momentum") or 0, bool(tp.get("nesterov") or False)
    if algo in ("adam", "adamw"):
        if mom or nest:
            raise ValueError("momentum / nesterov belong to optimizer_algorithm 'sgd', got %r with %r" % (algo, {"momentum": mom, "nesterov": nest}))
        optimizer = (GrooveAdamW if algo == "adamw" else GrooveAdam)(model.parameters(), lr, model.engine, weight_decay=wd)
    elif algo == "sgd":
        optimizer = GrooveSGD(model.parameters(), lr, model.engine, momentum=mom, nesterov=nest, weight_decay=wd or 0)
    else:
        raise ValueError("optimizer_algorithm must be 'sgd', 'adam' (ref:train.py:40-42) or 'adamw', got %r" % algo)
    _bind_engine(model)
    model.engine.set_state(lr=float(lr))
    model.engine.penalty = float(tp.get("hit_loss_penalty", 1.0))
    initial_epoch = 0
    if params.get("load_model"):
        ck = torch.load(find_checkpoint(params["load_model"]), map_location="cpu", weights_only=True)
        model.load_state_dict(ck["model_state_dict"], strict=True)
        optimizer.load_state_dict(ck["optimizer_state_dict"])
        optimizer._lr_on_device = None
        initial_epoch = int(ck["epoch"]) + 1          # resume after the stored epoch (payload, not file name: SURVEY 5)
        # continue the dropout stream where the stored run stopped (a reference-written checkpoint has no position: start
        # far from the masks of the first epochs)
        groups = ck["optimizer_state_dict"].get("param_groups") or [{}]
        step = int(groups[0].get("dropout_step", initial_epoch << 20)) & 0x7FFFFFFF
        model.engine.set_state(step=step)
        model._train_forwards = step
        if groups[0].get("voice_thresholds") is not None:
            model.voice_thresholds = groups[0]["voice_thresholds"]
    return model, optimizer, initial_epoch


# ------------------------------------------------------------------------------------------------ calculate_loss
class _LossFn(torch.autograd.Function):
    """gt_loss: BCE(hits)*pen + MSE(vel)*pen + MSE(off)*pen, voices summed, (B,T) averaged; grad = gt_loss's d_hvo."""

    @staticmethod
    def forward(ctx, hvo, y, penalty, engine, opts=None):
        s = engine.loss_slot(hvo.shape[0])
        s.hvo.copy_(hvo)
        stats, d_hvo = engine.loss(s, y, penalty, want_grad=True, opts=opts)
        ctx.save_for_backward(d_hvo)
        ctx.stats = stats.clone()
        return ctx.stats[0].clone()

    @staticmethod
    def backward(ctx, g):
        return ctx.saved_tensors[0] * g, None, None, None, None


def _loss_opts_of(engine, bce_fn=None, hit_loss_penalty=None, voice_weight=None, focal_gamma=None, vo_penalty=None, term_weights=None):
    """The StepEngine.loss_opts tuple for a bce_fn (its pos_weight: 1 or 9 elements) and calculate_loss's keyword options, or None when
    none of them is set (the loss then runs exactly as before).  ValueError for a pos_weight of any other shape or a value out of range."""
    pw = getattr(bce_fn, "pos_weight", None)
    if pw is None and voice_weight is None and focal_gamma is None and vo_penalty is None and term_weights is None:
        return None
    if pw is not None:
        pw = torch.as_tensor(pw).detach().float().cpu()
        if pw.numel() not in (1, 9) or pw.dim() > 1:
            raise ValueError("bce_fn.pos_weight must hold 1 or 9 elements (one per voice), got shape %s" % (tuple(pw.shape),))
        pw = pw.reshape(-1).tolist()
    return engine.make_loss_opts(vo_penalty=vo_penalty, pos_weight=1.0 if pw is None else pw, voice_weight=1.0 if voice_weight is None else voice_weight,
                                 focal_gamma=0.0 if focal_gamma is None else focal_gamma,
                                 term_weights=(1.0, 1.0, 1.0) if term_weights is None else term_weights, hit_penalty=hit_loss_penalty)


def calculate_loss(prediction, y, bce_fn, mse_fn, hit_loss_penalty, *, voice_weight=None, focal_gamma=None, vo_penalty=None, term_weights=None):
    """loss_fn of train_loop (ref:train.py:201-203,213).  bce_fn / mse_fn must be the reference's
    BCEWithLogitsLoss / MSELoss(reduction='none') (ref:train.py:176-179): the fused kernel implements exactly
    those.  Returns (loss tensor, hit_accuracy, hit_perplexity, bce_hits, mse_velocities, mse_offsets).
    Not in the reference: bce_fn.pos_weight (1 or 9 elements) is honoured as torch does; voice_weight (9) multiplies a voice's three terms,
    focal_gamma modulates the hit term by (1 - p_t)^gamma, vo_penalty is the penalty of the velocity / offset terms (default:
    hit_loss_penalty), term_weights = (h, v, o) weights of the three terms in the loss (gt_loss_opts, include/groove_hip.h).  With any of
    them the engine's `last_voice_stats` holds the 36 per-voice statistics of this call."""
    for fn, kind in ((bce_fn, torch.nn.BCEWithLogitsLoss), (mse_fn, torch.nn.MSELoss)):
        if fn is not None and (not isinstance(fn, kind) or fn.reduction != "none"):
            raise ValueError("calculate_loss expects %s(reduction='none') as in ref:train.py:176-179" % kind.__name__)
    h, v, o = prediction
    if not h.is_cuda:
        raise RuntimeError("calculate_loss runs on the GPU path only (predictions must be CUDA tensors)")
    # the engine that produced these predictions (model._run registers its output); predictions built elsewhere fall back to
    # the engine of the last initialised model
    engine = engine_of(h) or calculate_loss._engine
    if engine is None:
        raise RuntimeError("no model initialised: call initialize_model() (or bind calculate_loss._engine) first")
    hvo = torch.cat([h, v, o], dim=-1).contiguous()
    y = y.to(hvo.device, torch.float32)
    opts = _loss_opts_of(engine, bce_fn, float(hit_loss_penalty), voice_weight, focal_gamma, vo_penalty, term_weights)
    loss = _LossFn.apply(hvo, y, float(hit_loss_penalty), engine, opts)
    if opts is not None:
        engine.last_voice_stats = engine.loss_slot(hvo.shape[0]).voice_stats.clone()
    st = engine.loss_slot(hvo.shape[0]).stats.tolist()       # ONE D2H of the stats struct (no 5-6 .item() syncs)
    return loss, st[1], math.exp(st[3]), st[3], st[4], st[5]


calculate_loss._engine = None


def _bind_engine(model):
    if isinstance(model, _GrooveBase):
        calculate_loss._engine = model.engine


def save_schedule(total_epochs, initial_epochs_lim=10, initial_step=1, secondary_step_partial=10, secondary_step_all=20,
                  only_final=False):
    """Which epochs store a checkpoint / full evaluation: every epoch for the first `initial_epochs_lim`, then every
    10 (partial) / 20 (all), plus the last one -- the schedule ref:train.py:182-190 builds with ref:utils.py:230-264."""
    if only_final:
        return {total_epochs - 1}, set()
    part = set(range(0, min(initial_epochs_lim, total_epochs), initial_step))
    full = set(part)
    if initial_epochs_lim < total_epochs:
        part |= set(range(initial_epochs_lim, total_epochs, secondary_step_partial)) | {total_epochs - 1}
        full |= set(range(initial_epochs_lim, total_epochs, secondary_step_all)) | {total_epochs - 1}
    return part, full


# ------------------------------------------------------------------------------------------------ train_loop
def shift_right(y):
    """decoder teacher-forcing input: y delayed by one step, first row zeros."""
    return torch.cat([torch.zeros_like(y[:, :1]), y[:, :-1]], dim=1)


def _metrics_dict(prefix, st, clipped=False, voice=None):
    d = {prefix + "loss": st[0], prefix + "hit_accuracy": st[1], prefix + "hit_perplexity": math.exp(st[3]),
         prefix + "bce_h": st[3], prefix + "mse_v": st[4], prefix + "mse_o": st[5]}
    if clipped:                                # a clipped step's gradient norm before clipping and the coefficient applied
        d[prefix + "grad_norm"], d[prefix + "clip_coef"] = st[6], st[7]
    if voice is not None:                      # loss options on: each voice's share of bce_h and its hit accuracy (gt_loss_opts voice_stats)
        for c in range(9):
            d[prefix + "bce_h_voice%d" % c], d[prefix + "hit_accuracy_voice%d" % c] = voice[c], voice[27 + c]
    return d


# ------------------------------------------------------------------------------------------------ gradient clipping
def _engine_owning(params):
    """The StepEngine whose WHOLE parameter set `params` is (each one its Parameter view, each .grad its gradient view), else None."""
    from .engine import _ENGINES
    for eng in list(_ENGINES):
        views, gviews = eng.views(), eng.views(eng.grads)
        if len(params) != len(views):
            continue
        name_of = {v.data_ptr(): n for n, v in views.items()}
        names = [name_of.get(p.data_ptr()) for p in params]
        if None in names or len(set(names)) != len(names):
            continue
        if all(p.shape == views[n].shape and p.grad is not None and p.grad.data_ptr() == gviews[n].data_ptr()
               and p.grad.shape == gviews[n].shape for p, n in zip(params, names)):
            return eng
    return None


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """Drop-in for torch.nn.utils.clip_grad_norm_.  When `parameters` are exactly one model's parameters (model.parameters()), the
    norm type is 2 and error_if_nonfinite is off, the norm and the scaling run as two launches over the engine's flat gradient buffer
    (StepEngine.clip_grad_norm_: no synchronisation; returns a 0-dim device tensor).  Anything else -- a subset, another norm type,
    error_if_nonfinite, a max_norm <= 0 -- is torch's own function on the .grad tensors: slower, never different.  Data-parallel with
    the package's optimizers: call it on the all-reduced gradients (train_loop does); it clips the averaged gradient, as with DDP."""
    params = [parameters] if torch.is_tensor(parameters) else list(parameters)
    eng = None
    if float(norm_type) == 2.0 and not error_if_nonfinite and float(max_norm) > 0.0:
        eng = _engine_owning(params)
        if eng is not None and eng.world_size > 1 and not eng._fused_opt:
            eng = None                         # (a foreign optimizer has averaged the sums itself: grad_scale does not apply)
    if eng is not None:
        return eng.clip_grad_norm_(max_norm)
    return torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite, foreach=foreach)


def train_loop(dataloader, groove_transformer, encoder_only, opt, epoch, loss_fn, bce_fn, mse_fn, device,
               test_inputs=None, test_gt=None, validation_inputs=None, validation_gt=None, hit_loss_penalty=1,
               save=False, save_dir=None, run_id=None, log_every=50, on_log=None, max_grad_norm=None, loss_options=None):
    """One epoch (ref:train.py:195-215).  For every (x, y, idx) batch: forward, calculate_loss, backward, update.
    When model, loss_fn and optimizer are this package's, the whole batch body is ONE captured hipGraph replay
    (gt_train_step) and metrics leave the GPU as one 8-float copy every `log_every` batches; any other
    combination takes the generic autograd path.  Returns the metrics of the last logged batch.
    max_grad_norm (not in the reference): clip the gradients to this global 2-norm between backward and update
    (torch.nn.utils.clip_grad_norm_; inf = only measure); the logged records then carry train/grad_norm and train/clip_coef.
    loss_options (not in the reference): calculate_loss's keyword options {voice_weight, focal_gamma, vo_penalty, term_weights}; with them,
    or with a bce_fn that carries a pos_weight, every step computes the loss with options (StepEngine.loss_opts; the generic path and the
    test / validation leg pass the same options to loss_fn) and the logged records carry train/bce_h_voice{0..8} and
    train/hit_accuracy_voice{0..8}."""
    model = groove_transformer
    lopts = dict(loss_options or {})
    _bind_engine(model)
    model.train()
    eng = getattr(model, "engine", None)
    fast = (isinstance(model, _GrooveBase) and loss_fn is calculate_loss and isinstance(opt, _FusedMixin)
            and opt.engine is eng)
    world = 1
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        world = torch.distributed.get_world_size()
    fused_opt = isinstance(opt, _FusedMixin) and opt.engine is eng
    if eng is not None and eng.world_size != world:
        eng.world_size = world
    if fused_opt:                              # the fused update averages by grad_scale on the device: keep it = 1/world on BOTH paths
        eng.set_state(grad_scale=1.0 / world)
    if fast:
        eng.grads.zero_()                      # gt_train_step precondition; every fused update re-zeroes them
        eng.penalty = float(hit_loss_penalty)
        eng.algo = opt._algo
        opt._push_lr()
    clipped = max_grad_norm is not None
    if clipped:
        max_grad_norm = float(max_grad_norm)
    clip_keep = eng.max_grad_norm if fast else None
    if fast and clipped:
        eng.max_grad_norm = max_grad_norm      # the engine's clipped step (restored when the epoch ends)
    lo_keep = eng.loss_opts if fast else None
    lo_on = False                              # the fast path's loss runs with options
    if fast:
        lo = _loss_opts_of(eng, bce_fn, float(hit_loss_penalty), **lopts)
        lo_on = lo is not None
        if lo_on:
            eng.loss_opts = lo                 # (restored when the epoch ends)
    voice_of = lambda s_: eng.mean_voice_stats(s_).tolist() if lo_on else None
    last, stats = None, None
    n_batches = 0
    # a dataset resident in HBM hands over INDICES: the gather is the first launch of the step's graph
    indexed = fast and hasattr(dataloader, "index_batches") and getattr(dataloader, "x", None) is not None \
        and dataloader.x.device == eng.device
    batches = ((None, None, i) for i in dataloader.index_batches()) if indexed else dataloader
    # ... or ONE resident tensor of full grooves: the gather draws the voices to remove (gt_gather_infill) with the loader's options
    infilling = indexed and getattr(dataloader, "infill_opts", None) is not None
    # (event options: individual hits instead, gt_gather_infill_events)
    events = infilling and isinstance(dataloader.infill_opts, _lib.GtInfillEventOpts)
    if events:
        eng.infill_event_opts = _lib.infill_event_opts_tuple(dataloader.infill_opts)
    elif infilling:
        eng.infill_opts = _lib.infill_opts_tuple(dataloader.infill_opts)
    # wandb.watch(model, log_freq=1000) (ref:train.py:150) hooks the Parameters' gradients; the fused step never materialises a .grad
    # autograd could hook (it consumes and re-zeroes the flat gradient buffer inside its last launch).  Equivalent: every
    # model.watch_log_freq batches (0 = never) the step runs split -- backward, gradients visible, update -- and their histograms
    # are logged under the names wandb.watch uses ("gradients/<parameter>").
    watch = int(getattr(model, "watch_log_freq", 0) or 0) if fast else 0

    def watch_cb():
        rec = {}
        for n, g in eng.views(eng.grads).items():
            a = g.detach().float().cpu().numpy()
            rec["gradients/" + n] = wandb.Histogram(a) if (_wandb_active() and hasattr(wandb, "Histogram")) else a
        model.last_watch = rec
        if _wandb_active():
            wandb.log(rec, commit=False)

    try:
        for batch, (X, y, _idx) in enumerate(batches):
            n_batches += 1
            model._watch_step = getattr(model, "_watch_step", 0) + 1
            on_grads = watch_cb if (watch and model._watch_step % watch == 0) else None
            if events:
                stats = eng.train_step_indexed_infill_events(dataloader.x, _idx, on_grads=on_grads)
            elif infilling:
                stats = eng.train_step_indexed_infill(dataloader.x, _idx, on_grads=on_grads)
            elif indexed:
                stats = eng.train_step_indexed(dataloader.x, dataloader.y, _idx, on_grads=on_grads)
            if indexed:
                X = _idx                           # (only its length is used below)
                if (batch + 1) % log_every == 0:
                    last = _metrics_dict("train/", eng.mean_stats(eng.slot(X.shape[0])).tolist(), clipped, voice_of(eng.slot(X.shape[0])))
                if last is not None and (batch + 1) % log_every == 0:
                    rec = dict(last, epoch=epoch, batch=batch)
                    if _wandb_active():
                        wandb.log(rec, commit=True)
                    if on_log:
                        on_log(rec)
                continue
            X = X.to(device, torch.float32, non_blocking=True)
            y = y.to(device, torch.float32, non_blocking=True)
            if fast:
                stats = eng.train_step(X, y, on_grads=on_grads)
                if (batch + 1) % log_every == 0:
                    last = _metrics_dict("train/", eng.mean_stats(eng.slot(X.shape[0])).tolist(), clipped, voice_of(eng.slot(X.shape[0])))
            else:
                opt.zero_grad()
                pred = model(X) if encoder_only else model(X, shift_right(y))
                if eng is not None:
                    eng.last_voice_stats = None    # (calculate_loss leaves the per-voice statistics here when it ran with options)
                out = loss_fn(pred, y, bce_fn, mse_fn, hit_loss_penalty, **lopts)
                out[0].backward()
                if world > 1:
                    if eng is not None:            # every .grad is a view of ONE flat buffer: one collective, not one per tensor
                        torch.distributed.all_reduce(eng.grads)
                        if not fused_opt:          # a foreign optimizer knows nothing of grad_scale: average here
                            eng.grads /= world
                    else:
                        for p in model.parameters():
                            torch.distributed.all_reduce(p.grad)
                            p.grad /= world
                if clipped:
                    norm = clip_grad_norm_(model.parameters(), max_grad_norm)
                opt.step()
                last = {"train/loss": float(out[0]), "train/hit_accuracy": out[1], "train/hit_perplexity": out[2],
                        "train/bce_h": out[3], "train/mse_v": out[4], "train/mse_o": out[5]}
                if eng is not None and eng.last_voice_stats is not None:
                    vs = eng.last_voice_stats.tolist()
                    for c in range(9):
                        last["train/bce_h_voice%d" % c], last["train/hit_accuracy_voice%d" % c] = vs[c], vs[27 + c]
                if clipped:
                    n32 = torch.tensor(float(norm), dtype=torch.float32)
                    coef = torch.clamp(max_grad_norm / (n32 + 1e-6), max=1.0) if max_grad_norm != float("inf") else torch.tensor(1.0)
                    last["train/grad_norm"], last["train/clip_coef"] = float(n32), float(coef)
            if last is not None and ((batch + 1) % log_every == 0 or not fast):      # reference logs per batch; fast path every log_every
                rec = dict(last, epoch=epoch, batch=batch)
                if _wandb_active():
                    wandb.log(rec, commit=True)
                if on_log:
                    on_log(rec)
    finally:
        if fast:
            eng.max_grad_norm = clip_keep
            eng.loss_opts = lo_keep
    if fast and stats is not None:
        last = _metrics_dict("train/", eng.mean_stats(eng.slot(X.shape[0])).tolist(), clipped, voice_of(eng.slot(X.shape[0])))
    if isinstance(opt, GrooveAdam) and fast:
        for st in opt.state.values():
            st["step"] += n_batches
    if save:
        d = save_dir or (wandb.run.dir if _wandb_active() else ".")
        rid = run_id or (wandb.run.id if _wandb_active() else "local")
        save_checkpoint(os.path.join(d, FILE_PATTERN.format(rid, epoch)), epoch, model, opt,
                        last["train/loss"] if last else float("nan"))
    for name, xin, gt in (("test/", test_inputs, test_gt), ("validation/", validation_inputs, validation_gt)):
        if xin is None or gt is None:
            continue
        model.eval()
        with torch.no_grad():
            xin, gt = xin.to(device, torch.float32), gt.to(device, torch.float32)
            pred = model(xin) if encoder_only else model(xin, shift_right(gt))
            out = loss_fn(pred, gt, bce_fn, mse_fn, hit_loss_penalty, **lopts)
        rec = {name + "loss": float(out[0]), name + "hit_accuracy": out[1], name + "hit_perplexity": out[2],
               name + "bce_h": out[3], name + "mse_v": out[4], name + "mse_o": out[5], "epoch": epoch}
        if _wandb_active():
            wandb.log(rec, commit=False)
        if on_log:
            on_log(rec)
        model.train()
    return last
