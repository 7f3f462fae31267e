"""GrooveTransformerEncoder / GrooveTransformer: the reference's model interface over the HIP hot path.

Mirrors what the reference imports from its un-vendored submodule (ref:train.py:12,149; ref:evaluator.py:173):
``forward(src[, tgt]) -> (h_logits, v, o)`` and ``predict(src, use_thres=True, thres=0.5) -> (h, v, o)``,
an ``nn.Module`` whose ``state_dict()`` carries exactly the checkpoint's key names (so
ref:demo/transformer_run_171tyqit_Epoch_1.Model strict-loads) including the ``pe`` buffer.

Every parameter is a VIEW into the engine's flat HBM buffer (and ``.grad`` a view into the flat gradient
buffer), so the fused kernels, the single RCCL all-reduce and ``wandb.watch``/``state_dict`` all see the same
memory.  There is no CPU implementation: constructing a model without a ROCm GPU raises.
"""
import collections
import math
import os
import weakref

import torch
from torch import nn

from . import _lib, layout
from .engine import StepEngine


class _Node(nn.Module):
    """Name-only container so that parameter paths equal the reference's state-dict keys."""


def _attach(root, dotted, tensor, buffer=False):
    parts = dotted.split(".")
    m = root
    for p in parts[:-1]:
        if p not in m._modules:
            m.add_module(p, _Node())
        m = m._modules[p]
    if buffer:
        m.register_buffer(parts[-1], tensor)
    else:
        m.register_parameter(parts[-1], nn.Parameter(tensor))
    return m


# predictions -> the engine (and slot stamp) that produced them, keyed by the storage of the (B,32,27) tensor forward returned
# (h, v, o are views of it): calculate_loss finds ITS model's engine from the prediction, so two models in one process
# (train + a second evaluator model) never compute each other's loss.  Bounded; entries are overwritten per forward.
_PRODUCERS = collections.OrderedDict()


def _register_producer(hvo, engine):
    key = hvo.untyped_storage().data_ptr()
    _PRODUCERS.pop(key, None)
    _PRODUCERS[key] = weakref.ref(engine)
    while len(_PRODUCERS) > 64:
        _PRODUCERS.popitem(last=False)


def engine_of(tensor):
    """The StepEngine whose forward produced `tensor` (any view of its output), or None."""
    ref = _PRODUCERS.get(tensor.untyped_storage().data_ptr())
    return ref() if ref is not None else None


def default_seed_hi():
    """Data-parallel ranks must draw DIFFERENT dropout masks: the high seed word is the rank."""
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank()
    return int(os.environ.get("RANK", "0"))


class _GrooveFn(torch.autograd.Function):
    """autograd bridge: forward = gt_forward, backward = gt_backward accumulating into the flat .grad buffer."""

    @staticmethod
    def forward(ctx, hook, model, src, tgt):
        eng = model.engine
        train = model.training
        if train:
            model._train_forwards += 1
            eng.set_step_async(model._train_forwards)      # fresh dropout masks per training forward
        from .engine import PREDICT_CHUNK
        if not train and src.shape[0] > PREDICT_CHUNK:
            # evaluation sets come in one call (ref:train.py:195-215 test / validation inputs): chunked, nothing saved
            ctx.slot = None
            return eng.forward_eval_chunked(src, tgt)
        hvo = eng.forward(src, tgt, train)
        ctx.model, ctx.slot, ctx.train = model, eng.slot(src.shape[0]), train
        ctx.fwd_id = ctx.slot.fwd_id
        return hvo.clone()

    @staticmethod
    def backward(ctx, d_hvo):
        if ctx.slot is None:
            raise RuntimeError("backward through a chunked evaluation forward (more than %d sequences in eval mode): "
                               "no activations were saved" % d_hvo.shape[0])
        if ctx.slot.fwd_id != ctx.fwd_id:
            # the saved activations live in the per-batch-size workspace; a later forward / predict / train_step at the same
            # batch size has overwritten them -- gradients from them would be silently wrong
            raise RuntimeError("backward() after another forward at the same batch size (%d): the activations saved by this "
                               "forward were overwritten; call backward before the next forward of that size" % ctx.slot.B)
        ctx.model.engine.backward(ctx.slot, d_hvo.contiguous(), ctx.train, accumulate=True)
        return None, None, None, None


class _GrooveBase(nn.Module):
    def __init__(self, d_model, nhead, num_encoder_layers, num_decoder_layers, dim_feedforward, dropout,
                 embedding_size_src, embedding_size_tgt, max_len, device, seed=0, precision="fp32"):
        super().__init__()
        if max_len != 32 or embedding_size_tgt != 27:
            raise ValueError("the HIP path is built for max_len=32 / embedding_size_tgt=27 (ref:train.py:128,132)")
        self.d_model, self.nhead, self.dim_feedforward, self.dropout = d_model, nhead, dim_feedforward, dropout
        self.num_encoder_layers, self.num_decoder_layers = num_encoder_layers, num_decoder_layers
        self.embedding_size_src, self.embedding_size_tgt, self.max_len = embedding_size_src, embedding_size_tgt, max_len
        self.device = device if device is not None else "cuda"
        # dropout stream: low word = the run's seed, high word = the data-parallel rank (ranks must not share masks)
        self.engine = StepEngine(d_model, nhead, dim_feedforward, num_encoder_layers, num_decoder_layers, dropout,
                                 embedding_size_src, device=self.device,
                                 seed=(int(seed) & 0xFFFFFFFF) | (default_seed_hi() << 32), precision=precision)
        eng = self.engine
        grads = eng.views(eng.grads)
        for name, view in eng.views().items():
            _attach(self, name, view)
        for name, p in self.named_parameters():
            p.grad = grads[name]
        pe = eng.pe.view(1, max_len, d_model)
        _attach(self, "InputLayerEncoder.PositionalEncoding.pe", pe, buffer=True)
        if num_decoder_layers:
            _attach(self, "InputLayerDecoder.PositionalEncoding.pe", pe, buffer=True)
        self._hook = torch.zeros(1, device=eng.device, requires_grad=True)   # ties outputs into autograd
        self._train_forwards = 0
        self.reset_parameters()

    def reset_parameters(self):
        """torch defaults for the Transformer stack (xavier-uniform packed in-proj, zero attention biases,
        kaiming-uniform(a=sqrt 5) linears, LayerNorm 1/0); IO layers U(-0.1, 0.1) with zero bias
        (ckpt: InputLayer weight range +-0.0995)."""
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.endswith("in_proj_weight"):
                    nn.init.xavier_uniform_(p)
                elif name.endswith(("in_proj_bias", "out_proj.bias")):
                    p.zero_()
                elif name.startswith(("InputLayer", "OutputLayer")):
                    p.uniform_(-0.1, 0.1) if name.endswith("weight") else p.zero_()
                elif "norm" in name:
                    p.fill_(1.0) if name.endswith("weight") else p.zero_()
                elif name.endswith("weight"):
                    nn.init.kaiming_uniform_(p, a=math.sqrt(5))
                else:
                    fan_in = self.d_model if "linear1" in name else self.dim_feedforward
                    p.uniform_(-1.0 / math.sqrt(fan_in), 1.0 / math.sqrt(fan_in))

    def zero_grad(self, set_to_none=False):
        self.engine.grads.zero_()        # grads stay views of the flat buffer; never set to None

    def _run(self, src, tgt):
        src = src.to(self.engine.device, torch.float32)
        if src.dim() != 3 or src.shape[1] != self.max_len or src.shape[2] != self.embedding_size_src:
            raise ValueError("src must be (B, %d, %d), got %s" % (self.max_len, self.embedding_size_src, tuple(src.shape)))
        if tgt is not None:
            tgt = tgt.to(self.engine.device, torch.float32)
        hvo = _GrooveFn.apply(self._hook, self, src, tgt)
        _register_producer(hvo, self.engine)                   # calculate_loss(prediction, ...) runs on the engine that made it
        n = self.embedding_size_tgt // 3
        return hvo[..., :n], hvo[..., n:2 * n], hvo[..., 2 * n:]

    def predict(self, src, use_thres=True, thres=0.5, use_pd=False, pd_seed=None, voice_thresholds=None, voice_max_count=None,
                temperature=1.0, mask_vo=False):
        """eval-mode, no-grad inference (ref:evaluator.py:173): h thresholded to {0,1} (or probabilities).
        use_pd: hits SAMPLED from the predicted probabilities on the device (gt_predict_pd: h = 1 iff p > u, one u per (sequence, step,
        voice) from a counter hash of pd_seed -- drawn from torch's generator when not given); the encoder-decoder feeds the sampled
        hits back through its greedy decode.
        Per-voice controls (gt_predict_voices): voice_thresholds -- 9 values in [0,1] that override thres (with use_pd: a floor under the
        sampled hits, 0 when not given); voice_max_count -- 9 caps in 0..32 on a voice's hits per sequence, the most probable stay and of
        equal probabilities the earlier step; temperature -- p = sigmoid(logit / temperature); mask_vo -- velocity and offset are 0
        wherever the final hit is 0.  They need decided hits: with use_thres=False (and no use_pd) they raise ValueError.
        voice_thresholds="calibrated": the thresholds calibrate_thresholds stored (ValueError before any calibration)."""
        self.eval()
        n = self.embedding_size_tgt // 3
        voices = dict(voice_thresholds=voice_thresholds, voice_max_count=voice_max_count, temperature=temperature, mask_vo=mask_vo)
        if use_pd:
            if pd_seed is None:
                pd_seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
            with torch.no_grad():
                hvo = self.engine.predict(src, pd_seed=pd_seed, **voices)
            return hvo[..., :n], hvo[..., n:2 * n], hvo[..., 2 * n:]
        with torch.no_grad():
            hvo = self.engine.predict(src, use_thres=use_thres, thres=thres, **voices)
        return hvo[..., :n], hvo[..., n:2 * n], hvo[..., 2 * n:]

    def predict_hvo(self, src, use_thres=True, thres=0.5, voice_thresholds=None, voice_max_count=None, temperature=1.0, mask_vo=False):
        """Same, but returns the concatenated (N,32,27) HVO tensor (one D2H for the evaluator)."""
        self.eval()
        with torch.no_grad():
            return self.engine.predict(src, use_thres=use_thres, thres=thres, voice_thresholds=voice_thresholds,
                                       voice_max_count=voice_max_count, temperature=temperature, mask_vo=mask_vo)

    # the nine thresholds of the last calibration live on the engine (engine.predict(voice_thresholds="calibrated") reads them there)
    voice_thresholds = property(lambda self: self.engine.voice_thresholds,
                                lambda self, v: setattr(self.engine, "voice_thresholds", None if v is None else [float(t) for t in v]))

    def calibrate_thresholds(self, src, gt_hvo, criterion="f_beta", beta=1.0, grid=None, temperature=1.0, fallback=0.5, rounds=1):
        """Pick a hit threshold per voice from the threshold curves of an evaluation set: the curves are counted on the device
        (engine.hit_curve), ONE copy of the (9, 2, K + 1) counts comes to the host, gt_hit_thresholds chooses.  criterion "f_beta": the
        threshold of the best F-beta; "density": the threshold at which the voice places as many hits as the ground truth has.  A voice the
        rule cannot decide (no true hit; F-beta 0 everywhere) gets `fallback`.  The nine thresholds are stored as model.voice_thresholds:
        predict(voice_thresholds="calibrated") uses them, checkpoints carry them.
        Encoder-decoder: the curve holds the probabilities met along the greedy decode at the starting thresholds (0.5), which feeds decided
        hits back -- an approximation of what other thresholds would meet; rounds=2 repeats the calibration from the thresholds of round 1.
        -> {"thresholds": [9], "index": [9], "precision" | "recall" | "f_beta" | "density_ratio": {voice: float}, "counts": numpy (9, 2, K + 1)}"""
        from .metrics import VOICES
        if criterion not in _lib.CRITERIA:
            raise ValueError("criterion must be one of %s, got %r" % (sorted(_lib.CRITERIA), criterion))
        if int(rounds) < 1:
            raise ValueError("rounds must be >= 1, got %r" % (rounds,))
        eng = self.engine
        grid = [float(t) for t in (eng.DEFAULT_CURVE_GRID if grid is None else grid)]
        self.eval()
        start = None
        for _ in range(int(rounds)):
            with torch.no_grad():
                counts = eng.hit_curve(src, gt_hvo, grid=grid, temperature=temperature, voice_thresholds=start).cpu().numpy()
            th, idx, sc = eng.lib.hit_thresholds(counts, grid, _lib.CRITERIA[criterion], beta, fallback)
            start = th
        self.voice_thresholds = th
        out = {"thresholds": list(self.voice_thresholds), "index": idx, "counts": counts}
        for j, name in enumerate(("precision", "recall", "f_beta", "density_ratio")):
            out[name] = {v: sc[c][j] for c, v in enumerate(VOICES)}
        return out

    def infill(self, hvo_in, removed=None, mode=1, cells=None, **predict_kwargs):
        """The finished groove on the device: predict on the symbolic input hvo_in (N,32,27) -- a groove with voices removed --, then put
        the prediction back into it (gt_infill_merge; ref:evaluator.py:364-372 add_removed_part_to_hvo).  removed: one bitmask per sequence
        (what gt_gather_infill reported), or None -- the model may then fill any voice; mode 1: where the input has a hit its (h, v, o) win
        whole; mode 0: the reference's arithmetic (velocities and offsets are summed).  cells (instead of removed): the mask per cell
        (gt_infill_merge_cells) -- (N,9) bit words as gt_gather_infill_events reported them, or (N,32,9) bool: the prediction is confined to
        those cells.  predict_kwargs: predict_hvo's.  -> (N,32,27)"""
        from . import infill
        if removed is not None and cells is not None:
            raise ValueError("infill takes removed (a bitmask of voices per sequence) or cells (a mask per cell), not both")
        if self.embedding_size_src != self.embedding_size_tgt:
            raise ValueError("infill needs a symbolic model (embedding_size_src 27: the input is an HVO groove), got %d" % self.embedding_size_src)
        hvo_in = torch.as_tensor(hvo_in, dtype=torch.float32).to(self.engine.device).contiguous()
        pred = self.predict_hvo(hvo_in, **predict_kwargs)
        return infill.merge(pred, hvo_in, removed, mode, lib=self.engine.lib, out=pred, cells=cells)


class GrooveTransformerEncoder(_GrooveBase):
    """encoder_only = 1 (every shipped YAML: ref:configs/*_training.yaml:11)."""

    def __init__(self, d_model=512, nhead=8, num_encoder_layers=6, dim_feedforward=2048, dropout=0.1,
                 embedding_size_src=16, embedding_size_tgt=27, max_len=32, device=None, seed=0, precision="fp32"):
        super().__init__(d_model, nhead, num_encoder_layers, 0, dim_feedforward, dropout, embedding_size_src,
                         embedding_size_tgt, max_len, device, seed, precision)

    def forward(self, src):
        return self._run(src, None)


class GrooveTransformer(_GrooveBase):
    """encoder-decoder (encoder_only = 0, ref:train.py:125-127); tgt = y shifted right by one step."""

    def __init__(self, d_model=512, nhead=8, num_encoder_layers=6, num_decoder_layers=6, dim_feedforward=2048,
                 dropout=0.1, embedding_size_src=16, embedding_size_tgt=27, max_len=32, device=None, seed=0, precision="fp32"):
        super().__init__(d_model, nhead, num_encoder_layers, num_decoder_layers, dim_feedforward, dropout,
                         embedding_size_src, embedding_size_tgt, max_len, device, seed, precision)

    def forward(self, src, tgt):
        return self._run(src, tgt)


def parameter_names(model):
    return [n for n, _ in layout.param_names(model.d_model, model.dim_feedforward, model.embedding_size_src,
                                             model.num_encoder_layers, model.num_decoder_layers)]
