"""Per-voice generation controls on the GPU: the checks of tests/test_predict_voices.py on the HIP library (gt_voice_select against numpy,
gt_predict_voices against the fp64 oracle on the sequence-resident, the one-kernel-per-op and the greedy-decode path, the reduction to
gt_predict / gt_predict_pd_at, the argument checks), and the Python interface: model.predict / engine.predict with the new keywords."""
import numpy as np
import pytest
import torch

from harness import Runner, cfg_dict
from test_predict_voices import (CAPS, ENC, ENCDEC, REDUCTIONS, REJECTED, THRES, check_encoder_decoder, check_encoder_only, check_reduction,
                                 check_rejected, check_select, runner)
from transformergrooveinfilling_amd import layout

pytestmark = pytest.mark.gpu

OP = (cfg_dict(256, 4, 64, 1), 2)                   # one kernel per op


@pytest.mark.parametrize("mask_vo", [False, True])
@pytest.mark.parametrize("n_seq", [1, 3, 67])
def test_voice_select_against_numpy_hip(n_seq, mask_vo):
    r = runner("hip", ENC)
    check_select(r.lib, r.Buf, n_seq, mask_vo)


@pytest.mark.parametrize("temperature", [1.0, 0.5])
@pytest.mark.parametrize("shape", [ENC, OP], ids=["seq_d32", "op_d256"])
def test_encoder_only_against_oracle_hip(shape, temperature):
    check_encoder_only("hip", shape, temperature)


@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_encoder_decoder_against_oracle_hip(temperature):
    check_encoder_decoder("hip", ENCDEC, temperature)


@pytest.mark.parametrize("which", REDUCTIONS)
@pytest.mark.parametrize("shape", [ENC, ENCDEC], ids=["enc", "encdec"])
def test_reduces_to_predict_and_predict_pd_at_hip(shape, which):
    check_reduction("hip", shape, which)


@pytest.mark.parametrize("case", list(REJECTED))
def test_rejected_before_any_launch_hip(case):
    check_rejected("hip", case)


# ---- the Python interface ----------------------------------------------------------------------------------------------------------------
DIMS = dict(d_model=64, n_heads=4, dim_feedforward=64, num_encoder_layers=2, num_decoder_layers=0, dropout=0.0, embedding_size_src=16)


@pytest.fixture(scope="module")
def model():
    from transformergrooveinfilling_amd.training import initialize_model
    m, _, _ = initialize_model({"model": dict(DIMS, experiment="InfillingClosedHH", encoder_only=1, optimizer="sgd", max_len=32,
                                              embedding_size_tgt=27, device="cuda"),
                                "training": {"learning_rate": 0.05, "batch_size": 8, "hit_loss_penalty": 0.38}, "load_model": None})
    m.engine.load_named(layout.init_params(DIMS, seed=5))
    return m


def _x(n):
    return torch.from_numpy(layout.synthetic_batch(n, 16, seed=3)[0]).cuda()


def test_model_predict_with_voice_keywords(model):
    x = _x(5)
    kw = dict(voice_thresholds=THRES, voice_max_count=CAPS, temperature=0.5, mask_vo=True)
    h, v, o = model.predict(x, **kw)
    assert h.shape == v.shape == o.shape == (5, 32, 9)
    assert int(h.sum()) > 0 and set(h.unique().tolist()) <= {0.0, 1.0}
    assert (h.sum(1).cpu() <= torch.tensor(CAPS)[None, :]).all()               # per (sequence, voice): hit count <= cap
    assert (v[h == 0] == 0).all() and (o[h == 0] == 0).all()
    hvo = model.engine.predict(x, **kw)
    assert torch.equal(torch.cat([h, v, o], -1), hvo) and torch.equal(model.predict_hvo(x, **kw), hvo)
    uncapped = model.engine.predict(x, voice_thresholds=THRES, temperature=0.5)
    assert (uncapped[..., :9].sum(1).cpu() > torch.tensor(CAPS)[None, :]).any()     # (the caps had something to prune)


def test_sampled_mode_does_not_depend_on_the_chunking(model):
    x = _x(5)
    kw = dict(pd_seed=99, voice_thresholds=[0.3] * 9, voice_max_count=CAPS, temperature=0.8)
    a = model.engine.predict(x, chunk=2, **kw).clone()
    b = model.engine.predict(x, chunk=5, **kw)
    assert torch.equal(a, b)
    assert 0.02 < float(model.engine.predict(x, pd_seed=99, temperature=0.8)[..., :9].mean()) < 0.98
    h, _, _ = model.predict(x, use_pd=True, pd_seed=99, voice_thresholds=[0.3] * 9, voice_max_count=CAPS, temperature=0.8)
    assert torch.equal(h, b[..., :9])


def test_default_arguments_take_the_existing_calls(model, monkeypatch):
    """predict with default arguments: gt_predict / gt_predict_pd_at as before, bit for bit"""
    x = _x(5)
    r = Runner(DIMS, 5, "hip")
    r.set_params({k: v.detach().cpu().numpy() for k, v in model.engine.views().items()})
    want = r.predict(x.cpu().numpy(), thres=0.4)
    called = []
    call = model.engine.lib.call
    monkeypatch.setattr(model.engine.lib, "call", lambda name, *a: (called.append(name), call(name, *a))[1])
    h, v, o = model.predict(x, thres=0.4)
    got = torch.cat([h, v, o], -1).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    model.predict(x, use_pd=True, pd_seed=3)
    assert "gt_predict_voices" not in called and {"gt_predict", "gt_predict_pd_at"} <= set(called)
    model.predict(x, temperature=0.9)
    assert "gt_predict_voices" in called


@pytest.mark.parametrize("kw", [dict(voice_thresholds=[0.5] * 8), dict(voice_thresholds=[0.5] * 8 + [1.2]), dict(voice_max_count=[4] * 10),
                                dict(voice_max_count=[4] * 8 + [33]), dict(voice_max_count=[-1] * 9), dict(temperature=0.0),
                                dict(temperature=float("inf")), dict(temperature=float("nan")), dict(use_thres=False, mask_vo=True),
                                dict(use_thres=False, voice_max_count=CAPS)])
def test_bad_keywords_raise_before_the_library_is_called(model, monkeypatch, kw):
    def refuse(name, *a):
        raise AssertionError("library called: " + name)
    monkeypatch.setattr(model.engine.lib, "call", refuse)
    with pytest.raises(ValueError):
        model.predict(_x(2), **kw)
