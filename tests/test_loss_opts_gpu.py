"""The loss options of the train step on the GPU: the checks of tests/test_loss_opts.py through the HIP library -- gt_loss_ex's kernel against
the fp64 restatement, gt_train_step_loss on the shapes that reach every schedule (tests/test_optimizer_prepare_gpu.py ENGINE_CASES) against
forward / restated loss / backward, against the oracle's model and against gt_train_step, StepEngine.loss_opts with captured graphs,
calculate_loss against stock torch, train_loop's fast path against its generic path, and train.py's flags."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import loss_opts_ref as ref
import test_loss_opts as T
from harness import cfg_dict
from test_clip_grad_norm import _engine
from test_optimizer_prepare import ENGINE_VARIANTS, check_engine_against_torch
from test_optimizer_prepare_gpu import ENGINE_CASES
from transformergrooveinfilling_amd import _lib, layout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(name):
    dims, B = ENGINE_CASES[name]
    return cfg_dict(dims["d_model"], dims["n_heads"], dims["dim_feedforward"], dims["num_encoder_layers"], dims.get("num_decoder_layers", 0)), B, True


@pytest.mark.parametrize("wrt_logits", [0, 1])
@pytest.mark.parametrize("variant", list(T.VARIANTS))
@pytest.mark.parametrize("B", T.BATCHES)
def test_kernel_against_fp64_restatement_hip(B, variant, wrt_logits):
    T.check_kernel(_lib.get_lib(), "cuda", B, variant, wrt_logits)


@pytest.mark.parametrize("wrt_logits", [0, 1])
def test_kernel_against_fp64_restatement_saturated_hip(wrt_logits):
    T.check_kernel_saturated(_lib.get_lib(), "cuda", 3, wrt_logits)


@pytest.mark.parametrize("B", T.BATCHES)
def test_defaults_are_gt_loss_hip(B):
    T.check_defaults_match_gt_loss(_lib.get_lib(), "cuda", B)


def test_rejected_arguments_launch_nothing_hip():
    T.check_rejected(_lib.get_lib(), "cuda")


@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_step_teacher_forced_hip(case):
    T.check_step_teacher_forced("hip", *_case(case))


@pytest.mark.parametrize("case", ["headline_d128_bs64", "encdec_d32_l2_2_bs8"])
def test_step_against_oracle_model_hip(case):
    T.check_step_against_oracle("hip", *_case(case))


@pytest.mark.parametrize("case", [c for c in ENGINE_CASES if not c.startswith("encdec")])
def test_default_options_track_gt_train_step_hip(case):
    T.check_default_options_track_gt_train_step("hip", *_case(case))


# ---- StepEngine -----------------------------------------------------------------------------------------------------------------------
def _make(case, optimizer="sgd", **kw):
    dims, B = ENGINE_CASES[case]
    return _engine(dims, B, optimizer, lib=_lib.get_lib(), device="cuda", use_graph=True, **kw)


def test_engine_without_options_is_bitwise_unchanged_hip():
    case = "headline_d128_bs64"
    B = ENGINE_CASES[case][1]
    b = T.check_engine_off_is_bitwise_unchanged(lambda opt, **kw: _make(case, opt, **kw), B, "cuda")
    assert list(b.slot(B).graphs) == [("fused", b.algo, b.penalty)]                # today's graph key, nothing added


@pytest.mark.parametrize("case", list(ENGINE_CASES))
def test_engine_step_with_options_is_one_graph_hip(case):
    B = ENGINE_CASES[case][1]
    t = T.engine_opts_tuple()
    eng, twin = _make(case, loss_opts=t), _make(case)
    T.check_engine_step_against_module_sequence(eng, twin, B, "cuda")
    assert list(eng.slot(B).graphs) == [("fused", eng.algo, eng.penalty, t)]       # one captured graph, its key carries the tuple
    assert float(eng.slot(B).loss_scratch.abs().max()) == 0.0


@pytest.mark.parametrize("variant,clip", [("sgd_nesterov_wd", False), ("adamw", False), ("sgd_nesterov_wd", True)])
def test_clipped_and_extras_recipes_still_match_torch_hip(variant, clip):
    case = "headline_d128_bs64"
    B = ENGINE_CASES[case][1]
    optimizer, kw = ENGINE_VARIANTS[variant]
    t = T.engine_opts_tuple()
    x, y = T._batch(B, "cuda")
    extra = {}
    if clip:
        probe = _make(case, optimizer, loss_opts=t, max_grad_norm=float("inf"))
        extra = dict(max_grad_norm=0.3 * float(probe.train_step(x, y)[6]))
    eng, twin = (_make(case, optimizer, loss_opts=t, **kw, **extra) for _ in range(2))
    check_engine_against_torch(eng, optimizer, kw, x, y, max_norm=extra.get("max_grad_norm"), twin=twin)
    keys = list(twin.slot(B).graphs)
    assert len(keys) == 1 and keys[0][0] == ("fused_clip" if clip else "fused_prep") and keys[0][3] == t, keys


# ---- calculate_loss / train_loop / train.py ---------------------------------------------------------------------------------------------
def _params(**training):
    return {"model": {"experiment": "InfillingClosedHH", "encoder_only": 1, "optimizer": "sgd", "d_model": 64, "n_heads": 4,
                      "dim_feedforward": 64, "dropout": 0.0, "num_encoder_layers": 2, "num_decoder_layers": 0,
                      "max_len": 32, "embedding_size_src": 16, "embedding_size_tgt": 27, "device": "cuda"},
            "training": dict({"learning_rate": 0.05, "batch_size": 8, "hit_loss_penalty": 0.38}, **training), "load_model": None}


@pytest.mark.parametrize("pw", [T.PW, [3.0]])
def test_calculate_loss_honours_pos_weight_like_stock_torch(pw):
    """a bce_fn that carries a pos_weight: loss, terms and gradient are those of the stock torch modules (oracle.torch_groove's
    calculate_loss applies bce_fn itself), in fp64 on the CPU"""
    from oracle import torch_groove as tg
    from transformergrooveinfilling_amd.training import calculate_loss, initialize_model
    initialize_model(_params())
    hvo, y = ref.make_inputs(3, seed=2)
    hvo, y = hvo.reshape(3, 32, 27), y.reshape(3, 32, 27)
    pred = [torch.from_numpy(hvo[..., i * 9:(i + 1) * 9].copy()).cuda().requires_grad_(True) for i in range(3)]
    mse = torch.nn.MSELoss(reduction="none")
    out = calculate_loss(pred, torch.from_numpy(y).cuda(), torch.nn.BCEWithLogitsLoss(reduction="none", pos_weight=torch.tensor(pw).cuda()), mse, 0.38)
    out[0].backward()
    pred64 = [torch.from_numpy(hvo[..., i * 9:(i + 1) * 9].astype(np.float64)).requires_grad_(True) for i in range(3)]
    want = tg.calculate_loss(pred64, torch.from_numpy(y.astype(np.float64)),
                             torch.nn.BCEWithLogitsLoss(reduction="none", pos_weight=torch.tensor(pw, dtype=torch.float64)), mse, 0.38)
    want[0].backward()
    got, ref0 = float(out[0].detach()), float(want[0].detach())
    assert abs(got - ref0) <= T.STAT_TOL * max(1.0, abs(ref0))
    for i in (1, 3, 4, 5):
        assert abs(out[i] - want[i]) <= T.STAT_TOL * max(1.0, abs(want[i])), (i, out[i], want[i])
    for a, b in zip(pred, pred64):
        assert float((a.grad.cpu().double() - b.grad).abs().max()) < T.GRAD_TOL * float(max(p.grad.abs().max() for p in pred64))
    with pytest.raises(ValueError, match="pos_weight"):
        calculate_loss(pred, torch.from_numpy(y).cuda(), torch.nn.BCEWithLogitsLoss(reduction="none", pos_weight=torch.ones(3).cuda()), mse, 0.38)


def test_train_loop_fast_path_matches_its_generic_path():
    from transformergrooveinfilling_amd.training import calculate_loss, initialize_model, train_loop
    x, y = layout.synthetic_batch(32, 16, seed=3)
    x, y = torch.from_numpy(x), torch.from_numpy(y)
    batches = [(x[i:i + 8], y[i:i + 8], torch.arange(i, i + 8)) for i in range(0, 32, 8)]
    bce = torch.nn.BCEWithLogitsLoss(reduction="none", pos_weight=torch.tensor(T.PW).cuda())
    mse = torch.nn.MSELoss(reduction="none")
    opts = dict(voice_weight=T.VW, focal_gamma=2.0, vo_penalty=0.05, term_weights=(0.7, 2.0, 0.4))
    P = layout.init_params(dict(d_model=64, n_heads=4, dim_feedforward=64, num_encoder_layers=2, num_decoder_layers=0, dropout=0.0,
                                embedding_size_src=16), seed=5)
    runs = {}
    for name, loss_fn in (("fast", calculate_loss), ("generic", lambda *a, **k: calculate_loss(*a, **k))):
        model, opt, _ = initialize_model(_params())
        model.engine.load_named(P)
        log = []
        last = train_loop(dataloader=batches, groove_transformer=model, encoder_only=1, opt=opt, epoch=0, loss_fn=loss_fn, bce_fn=bce,
                          mse_fn=mse, device="cuda", hit_loss_penalty=0.38, log_every=1, on_log=log.append, loss_options=opts,
                          test_inputs=x[:8], test_gt=y[:8])
        torch.cuda.synchronize()
        assert model.engine.loss_opts is None                                      # restored when the epoch ends
        runs[name] = (model.engine.params.clone(), last, log)
    assert float((runs["fast"][0] - runs["generic"][0]).abs().max()) <= 1e-5      # (fused step vs module kernels: fp32 rounding)
    for k in ["train/loss", "train/bce_h"] + ["train/bce_h_voice%d" % c for c in range(9)] + ["train/hit_accuracy_voice%d" % c for c in range(9)]:
        assert abs(runs["fast"][1][k] - runs["generic"][1][k]) <= 2e-5 * max(1.0, abs(runs["generic"][1][k])), k
    assert abs(sum(runs["fast"][1]["train/bce_h_voice%d" % c] for c in range(9)) - runs["fast"][1]["train/bce_h"]) <= 1e-5
    tf, tg_ = (next(r for r in runs[n][2] if "test/loss" in r) for n in ("fast", "generic"))
    assert abs(tf["test/loss"] - tg_["test/loss"]) <= 2e-5 * max(1.0, abs(tg_["test/loss"]))
    # without options the records keep today's keys
    model, opt, _ = initialize_model(_params())
    last = train_loop(dataloader=batches[:1], groove_transformer=model, encoder_only=1, opt=opt, epoch=0, loss_fn=calculate_loss,
                      bce_fn=torch.nn.BCEWithLogitsLoss(reduction="none"), mse_fn=mse, device="cuda", hit_loss_penalty=0.38, log_every=1)
    assert not any("voice" in k for k in last)


def test_train_cli_with_loss_flags(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--experiment", "InfillingClosedHH", "--synthetic", "256", "--epochs", "1",
                        "--pos_weight", ",".join(str(v) for v in T.PW), "--focal_gamma", "2", "--vo_penalty", "0", "--loss_weights", "1,2,0.5",
                        "--wandb", "False", "--save-dir", str(tmp_path), "--eval-size", "64"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
