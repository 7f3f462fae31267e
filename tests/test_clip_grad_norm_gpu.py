"""Global-norm gradient clipping on the GPU: gt_clip_grad_norm's kernels against numpy, StepEngine's clipped step (captured graph) against
backward / torch's clip / update on the shapes of every schedule, the device's clipped gradients against the fp64 oracle's, train_loop's
fast path against the generic loop, and train.py --max_grad_norm."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from harness import Runner, cfg_dict
from oracle import numpy_groove as ng
from parity import GRAD_TOL, adopt_device_kinks, kink_bound
from test_clip_grad_norm import KERNEL_SHAPES, _engine, check_engine_against_manual, check_kernels
from transformergrooveinfilling_amd import _lib, layout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", list(KERNEL_SHAPES))
def test_kernels_against_numpy_hip(shape):
    check_kernels(_lib.get_lib(), "cuda", KERNEL_SHAPES[shape])


ENGINE_CASES = {
    # name: (dims, batch, extra engine keywords)
    "headline_d128_bs64": (dict(d_model=128, n_heads=4, dim_feedforward=512, num_encoder_layers=3), 64, {}),    # QUAD forward + rider wgrads
    "closedhh_d32_h16_bs16": (dict(d_model=32, n_heads=16, dim_feedforward=512, num_encoder_layers=6), 16, {}),
    "cli_d64_h16_l7_bs16": (dict(d_model=64, n_heads=16, dim_feedforward=256, num_encoder_layers=7), 16, {}),
    "op_d512_l1_bs64": (dict(d_model=512, n_heads=8, dim_feedforward=512, num_encoder_layers=1), 64, {}),
    "op_d512_bf16_bs64": (dict(d_model=512, n_heads=8, dim_feedforward=512, num_encoder_layers=1), 64, {"precision": "bf16"}),
    "encdec_d32_l2_2_bs8": (dict(d_model=32, n_heads=4, dim_feedforward=64, num_encoder_layers=2, num_decoder_layers=2), 8, {}),
}


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_engine_clipped_step_matches_manual_sequence_hip(case, optimizer):
    dims, B, kw = ENGINE_CASES[case]
    make = lambda **k: _engine(dims, B, optimizer, lib=_lib.get_lib(), device="cuda", use_graph=True, **kw, **k)
    probe = make(max_grad_norm=float("inf"))
    x, y = layout.synthetic_batch(B, 16, seed=9)
    first = float(probe.train_step(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())[6])
    adam = optimizer == "adam"
    clipped, _, _ = check_engine_against_manual(make, B, 0.3 * first, sgd_lr=None if adam else 0.05, shared_grads=adam)
    if adam:                                        # (the comparison above stepped through the split sequence: now the graph)
        st = clipped.train_step(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()).cpu()
        assert 0 < float(st[7]) < 1 and torch.isfinite(clipped.params).all()
    s = clipped.slot(B)
    assert any(k[0] == "fused_clip" for k in s.graphs)                       # the clipped step ran as one captured graph
    assert float(clipped._clip_scratch.abs().max()) == 0.0


def test_clipped_step_auto_graph_decision_and_unclipped_engine_unchanged():
    dims, B, _ = ENGINE_CASES["headline_d128_bs64"]
    a = _engine(dims, B, lib=_lib.get_lib(), device="cuda", dropout=0.24)
    b = _engine(dims, B, lib=_lib.get_lib(), device="cuda", dropout=0.24, max_grad_norm=None)
    x, y = layout.synthetic_batch(B, 16, seed=9)
    x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for _ in range(3):
        sa, sb = a.train_step(x, y).clone(), b.train_step(x, y).clone()
        assert torch.equal(sa, sb) and torch.equal(a.params, b.params)
    n = a.lib.cdll.gt_step_launches(ctypes.byref(a.slot(B).cfg))
    assert a._graph_for_clip(a.slot(B)) == (not (0 < n and n + 3 <= 24))


def test_clipped_gradients_against_the_oracle_hip():
    """the device's gradients after backward (skip_update = 1) and gt_clip_grad_norm == the fp64 oracle's gradients clipped here"""
    cfg = dict(cfg_dict(128, 4, 64, 2), dropout=0.1)
    B = 4
    P = ng.init_params(cfg, seed=9, perturb=0.05)
    x, y = ng.synthetic_batch(B, 16, seed=4)
    r = Runner(cfg, B, "hip", rng=(77, 5, 0), lr=0.05)
    r.set_params(P)
    r.train_step(x, y, 0.38, skip_update=1)
    (h, v, o), C = ng.forward({k: a.astype(np.float64) for k, a in P.items()}, cfg, x, rng=(77, 5, 0), dtype=np.float64)
    _, dpred = ng.calculate_loss((h, v, o), y.astype(np.float64), 0.38)
    assert adopt_device_kinks(r, C, cfg) <= kink_bound(r, cfg)
    G = ng.backward(P, cfg, C, dpred, dtype=np.float64)
    total = float(np.sqrt(sum(np.sum(g ** 2) for g in G.values())))
    mn = 0.25 * total
    coef = min(1.0, mn / (total + 1e-6))
    n_scr = int(r.lib.cdll.gt_clip_grad_norm_scratch_floats(ctypes.byref(r.c)))
    scratch = torch.zeros(n_scr, dtype=torch.float32, device="cuda")
    out = torch.zeros(2, dtype=torch.float32, device="cuda")
    r.lib.call("gt_clip_grad_norm", ctypes.byref(r.c), r.grads.ptr, r.state.ptr, ctypes.c_float(mn), ctypes.c_void_p(out.data_ptr()),
               ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    got = r.unflatten(r.grads.numpy())
    o = out.cpu().numpy()
    assert abs(float(o[0]) - total) <= GRAD_TOL * total and abs(float(o[1]) - coef) <= GRAD_TOL * coef
    for k in G:
        want = G[k] * coef
        err = float(np.abs(got[k] - want).max() / max(np.abs(want).max(), 1e-5 * coef))
        assert err < GRAD_TOL, (k, err)


def _params(d=64, H=4, F=64, L=2, lr=0.05, algo="sgd"):
    return {"model": {"experiment": "InfillingClosedHH", "encoder_only": 1, "optimizer": algo, "d_model": d, "n_heads": H,
                      "dim_feedforward": F, "dropout": 0.0, "num_encoder_layers": L, "num_decoder_layers": 0,
                      "max_len": 32, "embedding_size_src": 16, "embedding_size_tgt": 27, "device": "cuda"},
            "training": {"learning_rate": lr, "batch_size": 8, "hit_loss_penalty": 0.38}, "load_model": None}


def test_train_loop_fast_path_clips_like_the_generic_loop():
    from transformergrooveinfilling_amd.training import calculate_loss, initialize_model, train_loop
    x, y = layout.synthetic_batch(32, 16, seed=3)
    x, y = torch.from_numpy(x), torch.from_numpy(y)
    batches = [(x[i:i + 8], y[i:i + 8], torch.arange(i, i + 8)) for i in range(0, 32, 8)]
    bce, mse = torch.nn.BCEWithLogitsLoss(reduction="none"), torch.nn.MSELoss(reduction="none")
    P = layout.init_params(dict(d_model=64, n_heads=4, dim_feedforward=64, num_encoder_layers=2, num_decoder_layers=0, dropout=0.0,
                                embedding_size_src=16), seed=5)
    fast_model, fast_opt, _ = initialize_model(_params())
    fast_model.engine.load_named(P)
    logs = []
    # the generic loop: module forward, calculate_loss, backward, torch's clip, the optimizer
    ref_model, ref_opt, _ = initialize_model(_params())
    ref_model.engine.load_named(P)
    ref_model.train()
    norms = []
    for xb, yb, _ in batches:
        ref_opt.zero_grad()
        out = calculate_loss(ref_model(xb.cuda()), yb.cuda(), bce, mse, 0.38)
        out[0].backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(ref_model.parameters()), 0.2)))
        ref_opt.step()
    assert min(norms) > 0.2                                                   # (clipping active on every batch)
    m = train_loop(dataloader=batches, groove_transformer=fast_model, encoder_only=1, opt=fast_opt, epoch=0, loss_fn=calculate_loss,
                   bce_fn=bce, mse_fn=mse, device="cuda", hit_loss_penalty=0.38, log_every=1, on_log=logs.append, max_grad_norm=0.2)
    torch.cuda.synchronize()
    assert fast_model.engine.max_grad_norm is None                             # (the keyword binds this epoch only)
    assert float((fast_model.engine.params - ref_model.engine.params).abs().max()) <= 1e-5      # (fused step vs module kernels: fp32 rounding)
    got = [r["train/grad_norm"] for r in logs if "train/grad_norm" in r]
    assert len(got) == 4 and all(abs(a - b) <= 1e-5 * b for a, b in zip(got, norms)), (got, norms)
    assert all(0 < r["train/clip_coef"] < 1 for r in logs if "train/clip_coef" in r)
    assert "train/grad_norm" in m


def test_drop_in_on_model_parameters_takes_the_fused_path(monkeypatch):
    import transformergrooveinfilling_amd as pkg
    from transformergrooveinfilling_amd.training import calculate_loss, initialize_model
    model, opt, _ = initialize_model(_params())
    x, y = layout.synthetic_batch(8, 16, seed=3)
    bce, mse = torch.nn.BCEWithLogitsLoss(reduction="none"), torch.nn.MSELoss(reduction="none")
    model.train()
    opt.zero_grad()
    calculate_loss(model(torch.from_numpy(x).cuda()), torch.from_numpy(y).cuda(), bce, mse, 0.38)[0].backward()
    ref = [p.grad.detach().clone() for p in model.parameters()]
    copies = []
    for g in ref:
        c = torch.nn.Parameter(torch.empty_like(g))
        c.grad = g
        copies.append(c)
    want = float(torch.nn.utils.clip_grad_norm_(copies, 0.05))

    def refuse(*a, **k):
        raise AssertionError("the fused path must not call torch's clip_grad_norm_")
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", refuse)
    norm = pkg.clip_grad_norm_(model.parameters(), 0.05)
    assert norm.is_cuda and norm.dim() == 0 and abs(float(norm) - want) <= 1e-6 * want
    for p, c in zip(model.parameters(), copies):
        assert float((p.grad - c.grad).abs().max()) <= 1e-6 * float(c.grad.abs().max() + 1e-30)


def test_train_cli_with_max_grad_norm(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--experiment", "InfillingClosedHH", "--synthetic", "256", "--epochs", "1",
                        "--max_grad_norm", "0.5", "--wandb", "False", "--save-dir", str(tmp_path), "--eval-size", "64"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
