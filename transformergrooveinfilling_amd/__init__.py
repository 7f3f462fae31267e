"""MI355X-native hot path for the GrooveTransformer that pelinski/TransformerGrooveInfilling's
train.py drives: hand-written HIP kernels (csrc/) behind a C ABI (include/groove_hip.h), and the
Python mirror of the reference's model / loss / train-loop interface on top of it."""
from . import _lib, layout  # noqa: F401

__all__ = ["_lib", "layout", "clip_grad_norm_"]


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """Drop-in for torch.nn.utils.clip_grad_norm_ (training.clip_grad_norm_): a model's whole parameter set is clipped by two
    launches over its flat gradient buffer; anything else is handed to torch."""
    from .training import clip_grad_norm_ as clip
    return clip(parameters, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite, foreach=foreach)
