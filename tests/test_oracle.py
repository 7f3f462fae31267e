"""The oracle against its pins: the reference's demo checkpoint (a copy under golden/reference_demo/) and the golden vectors that stock
torch modules produced (oracle/make_golden.py).  CPU only."""
import glob
import os

import numpy as np
import pytest

from oracle import numpy_groove as ng

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_g2(path):
    z = np.load(path)
    cfg = {k: (float(v) if k == "dropout" else int(v)) for k, v in zip(z["cfg_keys"], z["cfg_vals"])}
    return z, cfg


def test_demo_checkpoint_forward():
    z = np.load(os.path.join(GOLD, "demo_ckpt.npz"))
    P = {k[3:]: z[k] for k in z.files if k.startswith("sd/")}
    pe = P.pop("InputLayerEncoder.PositionalEncoding.pe")
    assert pe.shape == (1, 32, 32)
    assert np.abs(pe[0] - ng.positional_encoding(32)).max() < 1e-6          # buffer == recomputed sinusoid
    assert float(z["sgd_lr"]) == pytest.approx(0.094) and int(z["epoch"]) == 0
    for H in (4, 16):
        cfg = dict(d_model=32, n_heads=H, dim_feedforward=16, num_encoder_layers=6, num_decoder_layers=0,
                   embedding_size_src=16)
        assert [n for n, _ in ng.param_names(cfg)] == list(P.keys())          # state-dict order
        (h, v, o), _ = ng.forward(P, cfg, z["x"])
        for a, k in ((h, "h"), (v, "v"), (o, "o")):
            assert np.abs(a - z["%s_H%d" % (k, H)]).max() < 2e-5


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "g2_*.npz"))))
def test_numpy_oracle_vs_torch_golden(path):
    z, cfg = load_g2(path)
    P = ng.init_params(cfg, seed=int(z["seed"]), perturb=0.05)
    if "param/OutputLayer.Linear.bias" in z.files:                             # seeded init is reproducible
        for k in P:
            assert np.array_equal(P[k], z["param/" + k])
    x, y = z["x"], z["y"]
    enc_only = cfg["num_decoder_layers"] == 0
    tgt = None if enc_only else np.concatenate([np.zeros_like(y[:, :1]), y[:, :-1]], 1)
    (h, v, o), C = ng.forward(P, cfg, x, tgt=tgt)
    for a, k in ((h, "h"), (v, "v"), (o, "o")):
        assert np.abs(a - z[k]).max() < 2e-5
    for pen in (1.0, 0.47, 0.0):
        st, dpred = ng.calculate_loss((h, v, o), y, pen)
        ref = z["stats_pen%g" % pen]
        assert np.allclose(np.array(st, np.float64), ref, rtol=2e-5, atol=1e-6)
    st, dpred = ng.calculate_loss((h, v, o), y, 0.47)
    G = ng.backward(P, cfg, C, dpred)
    for k in P:
        if "grad/" + k in z.files:
            ref = z["grad/" + k]
            assert np.abs(G[k] - ref).max() <= 2e-4 * np.abs(ref).max() + 1e-7, k
        else:
            idx, val = z["gidx/" + k], z["gval/" + k]
            assert np.abs(G[k].reshape(-1)[idx] - val).max() <= 2e-4 * np.abs(val).max() + 1e-7, k
            assert np.sqrt((G[k].astype(np.float64) ** 2).sum()) == pytest.approx(float(z["gnorm/" + k]), rel=1e-4)
    if "sgd/OutputLayer.Linear.bias" in z.files:
        Ps = ng.sgd_step(P, G, 0.094)
        Pa, _, _ = ng.adam_step(P, G, {k: 0 * P[k] for k in P}, {k: 0 * P[k] for k in P}, 1, 1e-3)
        for k in P:
            assert np.abs(Ps[k] - z["sgd/" + k]).max() < 1e-5, k
            live = np.abs(G[k]) > 1e-6        # Adam divides by |g|: a ~0 gradient (softmax-invariant key bias) is all noise
            assert np.abs(Pa[k] - z["adam/" + k])[live].max(initial=0) < 2e-5, k
    if "pred_h" not in z.files:                                                # full-size goldens (make_golden.py G2_FULL) carry no predict()
        return
    (ph, pv, po), margin = ng.predict(P, cfg, x)
    sure = margin > 1e-4
    assert np.array_equal(ph[sure], z["pred_h"][sure])                          # hit mask bit-exact
    if enc_only:                                                                # (greedy decode can diverge after a flipped hit)
        assert np.abs(pv - z["pred_v"]).max() < 2e-5 and np.abs(po - z["pred_o"]).max() < 2e-5


def test_reference_checkpoint_strict_loads_into_torch_restatement():
    import torch
    from oracle import torch_groove as tg
    ck = torch.load(os.path.join(GOLD, "reference_demo", "transformer_run_171tyqit_Epoch_1.Model"), weights_only=True, map_location="cpu")
    m = tg.build(dict(d_model=32, n_heads=4, dim_feedforward=16, num_encoder_layers=6, num_decoder_layers=0))
    res = m.load_state_dict(ck["model_state_dict"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert len(list(m.parameters())) == len(ck["optimizer_state_dict"]["param_groups"][0]["params"]) == 78
    z = np.load(os.path.join(GOLD, "demo_ckpt.npz"))                          # the weights demo_ckpt.npz was dumped from
    assert sorted(k[3:] for k in z.files if k.startswith("sd/")) == sorted(ck["model_state_dict"])
    for k, t in ck["model_state_dict"].items():
        assert np.array_equal(t.numpy(), z["sd/" + k]), k


def test_dropout_hash_statistics():
    m = ng.keep_mask((1234, 99, 3), ng.layer_site(2, ng.S_FFN), 200000, 0.24)
    keep = (m > 0).mean()
    assert abs(keep - 0.76) < 0.005
    assert np.allclose(m[m > 0], 1 / (1 - float(np.float32(0.24))))
    m2 = ng.keep_mask((1234, 99, 4), ng.layer_site(2, ng.S_FFN), 200000, 0.24)
    assert abs(((m > 0) == (m2 > 0)).mean() - (0.76 ** 2 + 0.24 ** 2)) < 0.01   # steps are independent


def _synthetic_update(seed=0, lr=0.05):
    """Parameters (a weight matrix, LayerNorm gains near 1, a bias) and fp64 gradients whose magnitudes spread over decades, the largest
    update 3e-3 (150 times the old 2e-5 bar), like a real first step's"""
    rnd = np.random.default_rng(seed)
    P = {"w": (0.1 * rnd.standard_normal((64, 32))).astype(np.float32),
         "norm.weight": (1 + 0.01 * rnd.standard_normal(32)).astype(np.float32),
         "b": (0.05 * rnd.standard_normal(96)).astype(np.float32)}
    G = {k: rnd.standard_normal(v.shape) * np.exp(rnd.standard_normal(v.shape)) for k, v in P.items()}
    G = {k: g * 3e-3 / (lr * np.abs(g).max()) for k, g in G.items()}
    return P, G, np.float32(lr)


def _sgd(P, G, lr, which=None, fn=None):
    """w - lr g in fp32 on the fp32-rounded gradient, as the device runs it; which = (tensor, flat index): that element computed by fn"""
    out = {k: (P[k] - lr * G[k].astype(np.float32)).astype(np.float32) for k in P}
    if which is not None:
        k, i = which
        out[k].reshape(-1)[i] = fn(P[k].reshape(-1)[i], G[k].reshape(-1), i)
    return out


def _old_bar_accepts(P, after, G, lr):
    """check_train_step's free-running parameter bar before the per-step check existed: |p_dev - p_ref| < 2e-5 max(1, max |p|)"""
    return all(np.abs(after[k] - (P[k].astype(np.float64) - float(lr) * G[k])).max() < 2e-5 * max(1.0, np.abs(P[k]).max()) for k in P)


def test_update_check_catches_subtly_wrong_sgd_updates():
    import parity
    P, G, lr = _synthetic_update()
    assert parity.check_update(P, _sgd(P, G, lr), G, lr) < 0.1               # the exact update passes with room
    assert _old_bar_accepts(P, _sgd(P, G, lr), G, lr)
    d = np.abs(float(lr) * G["w"]).reshape(-1)
    # an element left where it was although its update (below the old bar) is not negligible
    small = int(np.flatnonzero((d > 2e-6) & (d < 2e-5))[0])
    frozen = _sgd(P, G, lr, ("w", small), lambda w, g, i: w)
    # an element updated with its neighbour's gradient; the pair chosen so that the two updates differ by less than the old bar
    dd = np.abs(np.diff(float(lr) * G["w"].reshape(-1)))
    nb = int(np.flatnonzero((dd > 2e-6) & (dd < 2e-5))[0])
    swapped = _sgd(P, G, lr, ("w", nb), lambda w, g, i: np.float32(w - lr * np.float32(g[i + 1])))
    for bad in (frozen, swapped):
        assert _old_bar_accepts(P, bad, G, lr)                                   # the gap the per-step check closes
        with pytest.raises(AssertionError, match="w element"):
            parity.check_update(P, bad, G, lr)
    with pytest.raises(AssertionError):
        parity.check_update(P, _sgd(P, G, np.float32(lr * 0.995)), G, lr)


def _adam(P, G, m0, v0, t, lr):
    """Adam in fp32 as the device runs it (seq_upd_elem / adam_kernel), on the fp32-rounded gradient"""
    f = np.float32
    b1, b2, eps = f(0.9), f(0.999), f(1e-8)
    step_size, inv_sqrt_bc2 = f(lr) / (f(1) - b1 ** f(t)), f(1) / np.sqrt(f(1) - b2 ** f(t))
    out, m1, v1 = {}, {}, {}
    for k in P:
        g = G[k].astype(f)
        m1[k] = (b1 * m0[k] + (f(1) - b1) * g).astype(f)
        v1[k] = (b2 * v0[k] + (f(1) - b2) * g * g).astype(f)
        out[k] = (P[k] - step_size * m1[k] / (np.sqrt(v1[k]) * inv_sqrt_bc2 + eps)).astype(f)
    return out, m1, v1


def test_update_check_catches_adam_with_the_wrong_step():
    import parity
    P, G, lr = _synthetic_update(seed=1)
    rnd = np.random.default_rng(2)
    m0 = {k: (0.3 * g * rnd.random(g.shape)).astype(np.float32) for k, g in G.items()}          # mid-training moments
    v0 = {k: (0.01 * g * g * rnd.random(g.shape)).astype(np.float32) for k, g in G.items()}
    after, m1, v1 = _adam(P, G, m0, v0, 3, lr)
    assert parity.check_update(P, after, G, lr, adam=dict(m0=m0, v0=v0, m1=m1, v1=v1, t=3)) < 0.1
    after2, m2, v2 = _adam(P, G, m0, v0, 2, lr)                                                 # bias correction of step 2 at step 3
    with pytest.raises(AssertionError, match="live elements"):
        parity.check_update(P, after2, G, lr, adam=dict(m0=m0, v0=v0, m1=m2, v1=v2, t=3))
    with pytest.raises(AssertionError, match="first moment"):                                   # moments from stale state
        parity.check_update(P, after, G, lr, adam=dict(m0=m0, v0=v0, m1={k: 0.9 * m0[k] for k in m0}, v1=v1, t=3))
