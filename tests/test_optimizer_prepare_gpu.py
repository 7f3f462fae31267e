"""The optimizer's extras (SGD momentum / Nesterov / weight decay, Adam's L2 weight decay, AdamW) on the GPU: gt_optimizer_prepare's kernel
against the fp64 restatement, StepEngine's steps -- watched and as one captured graph -- against torch.optim on the shapes of every
schedule, the everything-off step, the exchanges' fail-safe, train_loop's fast path against the generic loop, and train.py's flags."""
import os
import subprocess
import sys

import pytest
import torch

from test_clip_grad_norm import KERNEL_SHAPES, _engine
from test_optimizer_prepare import ENGINE_VARIANTS, _batch, check_engine_against_torch, check_kernel
from transformergrooveinfilling_amd import _lib, layout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", list(KERNEL_SHAPES))
def test_kernel_against_fp64_restatement_hip(shape):
    check_kernel(_lib.get_lib(), "cuda", KERNEL_SHAPES[shape])


ENGINE_CASES = {
    # name: (dims, batch): the shapes that exercise each schedule
    "headline_d128_bs64": (dict(d_model=128, n_heads=4, dim_feedforward=512, num_encoder_layers=3), 64),       # QUAD forward + rider wgrads
    "closedhh_d32_h16_bs16": (dict(d_model=32, n_heads=16, dim_feedforward=512, num_encoder_layers=6), 16),
    "op_d512_l1_bs64": (dict(d_model=512, n_heads=8, dim_feedforward=512, num_encoder_layers=1), 64),
    "encdec_d32_l2_2_bs8": (dict(d_model=32, n_heads=4, dim_feedforward=64, num_encoder_layers=2, num_decoder_layers=2), 8),
}


def _make(case, optimizer, **kw):
    dims, B = ENGINE_CASES[case]
    return _engine(dims, B, optimizer, lib=_lib.get_lib(), device="cuda", use_graph=True, **kw)


def _check_case(case, variant, max_norm=None):
    optimizer, kw = ENGINE_VARIANTS[variant]
    B = ENGINE_CASES[case][1]
    extra = {} if max_norm is None else {"max_grad_norm": max_norm}
    eng, twin = _make(case, optimizer, **kw, **extra), _make(case, optimizer, **kw, **extra)
    check_engine_against_torch(eng, optimizer, kw, *_batch(B, "cuda"), max_norm=max_norm, twin=twin)
    # the twin's steps ran as ONE captured graph whose key carries the hyper-parameter tuple
    keys = list(twin.slot(B).graphs)
    assert len(keys) == 1 and keys[0][0] == ("fused_prep" if max_norm is None else "fused_clip"), keys
    assert keys[0][-4:] == twin._opt_extras(), keys


@pytest.mark.parametrize("variant", list(ENGINE_VARIANTS))
def test_headline_step_matches_torch_optim_hip(variant):
    _check_case("headline_d128_bs64", variant)


@pytest.mark.parametrize("variant", ["sgd_nesterov_wd", "adamw"])
@pytest.mark.parametrize("case", [c for c in ENGINE_CASES if c != "headline_d128_bs64"])
def test_engine_step_matches_torch_optim_hip(case, variant):
    _check_case(case, variant)


def test_clip_first_then_transform_hip():
    case = "headline_d128_bs64"
    probe = _make(case, "sgd", max_grad_norm=float("inf"))
    first = float(probe.train_step(*_batch(ENGINE_CASES[case][1], "cuda"))[6])
    _check_case(case, "sgd_nesterov_wd", max_norm=0.3 * first)


def test_everything_off_is_bitwise_unchanged_hip():
    case = "headline_d128_bs64"
    B = ENGINE_CASES[case][1]
    x, y = _batch(B, "cuda")
    for optimizer in ("sgd", "adam"):
        a = _make(case, optimizer)
        b = _make(case, optimizer, weight_decay=0.0, momentum=0.0, nesterov=False)
        for _ in range(3):
            sa, sb = a.train_step(x, y).clone(), b.train_step(x, y).clone()
            assert torch.equal(sa, sb) and torch.equal(a.params, b.params)
        assert b.mbuf is None
        assert list(b.slot(B).graphs) == list(a.slot(B).graphs) == [("fused", b.algo, b.penalty)]       # no new graph key


@pytest.mark.parametrize("optimizer,kw", [("sgd", dict(momentum=0.9, weight_decay=5e-2)), ("adamw", dict(weight_decay=5e-2))])
def test_extras_keep_the_exchange_fail_safe_hip(optimizer, kw):
    dims = dict(d_model=128, n_heads=4, dim_feedforward=32, num_encoder_layers=1)
    eng = _engine(dims, 2, optimizer, dropout=0.0, lib=_lib.get_lib(), device="cuda", use_graph=True, **kw)
    x, y = _batch(2, "cuda")
    s = eng.slot(2)
    assert eng._xchg_word(s) is not None            # (d_model 128 at batch 2: the four-workgroups-per-sequence forward and its exchange region)
    eng.train_step(x, y)
    keep = {k: getattr(eng, k).clone() for k in ("params", "mbuf", "m", "v") if getattr(eng, k) is not None}
    t0 = eng.state_struct().opt_step
    eng._xchg_word(s)[0] = 1                        # the error word, raised by hand
    eng.train_step(x, y)
    torch.cuda.synchronize()
    for k, t in keep.items():
        assert torch.equal(getattr(eng, k), t), k
    assert eng.state_struct().opt_step == t0 and float(eng.grads.abs().max()) == 0.0


def _params(algo="sgd", **training):
    return {"model": {"experiment": "InfillingClosedHH", "encoder_only": 1, "optimizer": algo, "d_model": 64, "n_heads": 4,
                      "dim_feedforward": 64, "dropout": 0.0, "num_encoder_layers": 2, "num_decoder_layers": 0,
                      "max_len": 32, "embedding_size_src": 16, "embedding_size_tgt": 27, "device": "cuda"},
            "training": dict({"learning_rate": 0.05, "batch_size": 8, "hit_loss_penalty": 0.38}, **training), "load_model": None}


def test_train_loop_fast_path_matches_the_generic_loop():
    from transformergrooveinfilling_amd.training import GrooveSGD, calculate_loss, initialize_model, train_loop
    x, y = layout.synthetic_batch(32, 16, seed=3)
    x, y = torch.from_numpy(x), torch.from_numpy(y)
    batches = [(x[i:i + 8], y[i:i + 8], torch.arange(i, i + 8)) for i in range(0, 32, 8)]
    bce, mse = torch.nn.BCEWithLogitsLoss(reduction="none"), torch.nn.MSELoss(reduction="none")
    P = layout.init_params(dict(d_model=64, n_heads=4, dim_feedforward=64, num_encoder_layers=2, num_decoder_layers=0, dropout=0.0,
                                embedding_size_src=16), seed=5)
    extras = dict(momentum=0.9, nesterov=True, weight_decay=5e-4)
    fast_model, fast_opt, _ = initialize_model(_params(**extras))
    assert isinstance(fast_opt, GrooveSGD) and {k: fast_opt.param_groups[0][k] for k in extras} == extras
    fast_model.engine.load_named(P)
    # the generic loop through the module API: forward, calculate_loss, backward, opt.step()
    ref_model, ref_opt, _ = initialize_model(_params(**extras))
    ref_model.engine.load_named(P)
    ref_model.train()
    for xb, yb, _ in batches:
        ref_opt.zero_grad()
        calculate_loss(ref_model(xb.cuda()), yb.cuda(), bce, mse, 0.38)[0].backward()
        ref_opt.step()
    train_loop(dataloader=batches, groove_transformer=fast_model, encoder_only=1, opt=fast_opt, epoch=0, loss_fn=calculate_loss,
               bce_fn=bce, mse_fn=mse, device="cuda", hit_loss_penalty=0.38, log_every=1)
    torch.cuda.synchronize()
    fe, re_ = fast_model.engine, ref_model.engine
    assert float(fe.mbuf.abs().max()) > 0
    assert float((fe.params - re_.params).abs().max()) <= 1e-5          # (fused step vs module kernels: fp32 rounding)
    assert float((fe.mbuf - re_.mbuf).abs().max()) <= 1e-5
    # the momentum buffers ride in the checkpoint format torch uses
    sd = fast_opt.state_dict()
    assert torch.equal(sd["state"][0]["momentum_buffer"], next(iter(fe.views(fe.mbuf).values())))


def test_train_cli_with_adamw(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--experiment", "InfillingClosedHH", "--synthetic", "256", "--epochs", "1",
                        "--optimizer_algorithm", "adamw", "--weight_decay", "0.01", "--wandb", "False", "--save-dir", str(tmp_path),
                        "--eval-size", "64"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
