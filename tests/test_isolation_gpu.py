"""tests/isolation.py on the MI355X at the smallest shape on each side of each host dispatch rule (DESIGN.md 4a, table "rule -> boundary
batch -> test"): no result depends on the bytes a workspace or an output buffer held, on the calls the buffers served before, or on what
lies beside them, and nothing is written there.  No oracle runs, so a case costs what its launches cost.  Every case asserts the path it
exists for from the GT_TRACE_DISPATCH lines of its default-mode pass, with the helpers of tests/test_dispatch_edges_gpu.py (the
deterministic pass has no split over the tokens, hence no chunk tails).  The engine twin runs StepEngine with every torch.empty /
empty_like it makes filled with NaNs.

GT_ISOLATION_REPORT=<file>: append one line per case (dispatch families seen, wall time); profiles/isolation.txt is written from it."""
import os
import time

import numpy as np
import pytest

import isolation as iso
from harness import cfg_dict, dispatched
from test_dispatch_edges_gpu import (C4_1, EPI_MASK_NZ, EPI_RELU_DROP, EPI_RES_LN, EPI_RES_LNBWD, EPI_STORE, FALLBACK, GEMMS, KS_1, LM_1, RING,
                                     _cus, _d128_boundaries, _no_ln_exchange, _schedule, _traced, _wgrad_tail)

pytestmark = pytest.mark.gpu

P = 0.2
D128 = cfg_dict(128, 4, 64, 1)                     # (the table's shape with one layer)
D64_H16 = cfg_dict(64, 16, 256, 1)
D96 = cfg_dict(96, 2, 2048, 1)
PRED_D512 = cfg_dict(512, 8, 2048, 1, 1)
ENCDEC_D32 = cfg_dict(32, 4, 64, 1, 1)
PREDICT_FORMS = ("eval", "predict", "predict_pd")   # the predict edges: the decode GEMMs are what the batch size moves


def _report(request, trace, err, t0):
    path = os.environ.get("GT_ISOLATION_REPORT")
    if path:
        fams = sorted({fam for fam, _ in trace} | {" ".join(ln.split()[:2]) for ln in err.splitlines() if ln.startswith("[gemm64] ")})
        with open(path, "a") as f:
            f.write("%s | %s | %.1f s\n" % (request.node.name, " ".join(fams), time.time() - t0))


# ---- the paths: (trace, stderr, batch) -> assertions, one per rule of the table ----------------------------------------------------------
def _generic(cfg, bm, **kw):
    def path(tr, err, B):
        M = 32 * B
        assert dispatched(tr, "gemm_cfg", BM=bm, BN=bm, M=M, edge=1, **kw), dispatched(tr, "gemm_cfg", M=M)[:4]
    return path


def _ffn_generic(bm, cls):
    def path(tr, err, B):
        M = 32 * B
        assert dispatched(tr, "gemm_cfg", BM=bm, BN=bm, M=M, N=2048, K=256, form="NT", epi=EPI_RELU_DROP, edge=1)
        assert dispatched(tr, "gemm_cfg", BM=bm, BN=bm, M=M, N=2048, K=256, form="NN", epi=EPI_MASK_NZ, edge=1)
        assert not dispatched(tr, RING, M=M, N=2048)
        if cls is not None:
            _wgrad_tail(tr, cls)
    return path


def _ring64(tr, err, B):
    ring = dispatched(tr, ("gemm64", "gemm64h"), M=32 * B)
    assert ring
    if B == 64:                                      # the whole grid resident: LayerNorm through the row exchange, FFN keep bits
        assert dispatched(tr, "gemm64", M=2048, N=512, epi=EPI_RES_LN, rowx=1) and dispatched(tr, "gemm64", M=2048, N=512, epi=EPI_RES_LNBWD, rowx=1)
        assert any(ln.startswith("[gemm64] kbits write") for ln in err.splitlines())


def _off_ring64(tr, err, B):
    assert not dispatched(tr, RING, M=32 * B)
    assert dispatched(tr, "gemm_cfg", M=32 * B, N=1536, edge=1)
    _wgrad_tail(tr, 2)


def _row_tile_513(tr, err, B):
    assert dispatched(tr, "gemm_cfg", BM=64, BN=256, M=16416, N=256, row=1, epi=EPI_RES_LN, edge=1)
    assert dispatched(tr, "gemm_cfg", BM=64, BN=256, M=16416, N=256, row=1, epi=EPI_RES_LNBWD, form="NN", edge=1)
    assert not dispatched(tr, RING, M=16416)
    _wgrad_tail(tr, 2)


def _fallback_d256(tr, err, B):
    _no_ln_exchange([t for t in tr if t[1].get("M") == 32 * B], "")
    assert dispatched(tr, "gemm32row", BM=32, M=32 * B, N=256, epi=EPI_RES_LN, form="NT")
    assert dispatched(tr, "gemm32row", BM=32, M=32 * B, N=256, epi=EPI_RES_LNBWD, form="NN")


def _fallback_d512(tr, err, B):
    _no_ln_exchange([t for t in tr if t[1].get("M") == 32 * B], "")
    assert dispatched(tr, "gemm64", M=2048, N=512, K=512, form="NT", epi=EPI_STORE)
    assert dispatched(tr, "ln_fwd", M=2048, d=512) and dispatched(tr, "ln_bwd", M=2048, d=512)


def _sched(want):
    def path(tr, err, B):
        mine = [t for t in tr if t[0] in ("seq_fwd", "seq_bwd") and t[1]["B"] == B]
        got = _schedule(mine)
        assert got == want, (B, got, want)
    return path


def _narrow_whole(tr, err, B):
    mine = [t for t in tr if t[0] in ("seq_fwd", "seq_bwd") and t[1]["B"] == B]
    assert _schedule(mine)[0] == 0


def _wgrad_class_1(tr, err, B):
    q = _wgrad_tail(tr, 1)
    assert any(d["M"] == 2048 and d["N"] == 96 and d["K"] == 2016 and d["k_chunk"] == 256 for d in q), q
    assert dispatched(tr, "attn_fwd", kernel="generic") and dispatched(tr, "attn_bwd", kernel="generic")


def _decode_edges(tr, err, B):
    dec = dispatched(tr, RING + ("gemm_cfg",), M=B)
    assert dec and all(d["edge"] == 1 for d in dec if "edge" in d) and not dispatched(tr, RING, M=B), dec[:3]


def _decode(tr, err, B):
    assert dispatched(tr, GEMMS, M=B)


def _bf16_wt(bm):
    def path(tr, err, B):
        M = 32 * B
        big = dispatched(tr, "gemm_cfg", M=M, prec=1, edge=1)
        assert any(d["BM"] == bm for d in big), big[:6]
        assert not dispatched(tr, ("gemm32h", "gemm64h"), M=M) and not dispatched(tr, GEMMS, M=M, prec=0)
    return path


def _bf16_shadows(tr, err, B):
    assert dispatched(tr, ("gemm32h", "gemm64h"), M=32 * B, prec=1)


def _op_path(tr, err, B):
    assert dispatched(tr, GEMMS, M=32 * B) and not [t for t in tr if t[0] == "seq_fwd" and t[1]["B"] == B]


def _b(edge):
    return lambda: _d128_boundaries()[edge][0]


def _want(edge):
    return lambda tr, err, B: _sched(_d128_boundaries()[edge][1])(tr, err, B)


# id -> (cfg, batch or a callable giving it, keywords of the checks, path)
CASES = {
    "d512-64": (C4_1, 64, {}, _ring64), "d512-65": (C4_1, 65, {}, _off_ring64), "d512-66": (C4_1, 66, {}, _ring64),
    "d256-F2048-33": (LM_1, 33, {}, _ffn_generic(64, None)), "d256-F2048-129": (LM_1, 129, {}, _ffn_generic(128, 2)),
    "d256-F2048-130": (LM_1, 130, {}, _ffn_generic(128, 3)), "d256-F2048-131": (LM_1, 131, {}, _ffn_generic(128, 2)),
    "d512-qkv-43": (C4_1, 43, {}, _generic(C4_1, 64, N=1536, K=512, form="NT", epi=EPI_STORE)),
    "d256-513": (KS_1, 513, {}, _row_tile_513),
    "fallback-d256-256": (KS_1, 256, dict(flags=FALLBACK), _fallback_d256), "fallback-d512-64": (C4_1, 64, dict(flags=FALLBACK), _fallback_d512),
    "d128-quad-last": (D128, _b("quad-last"), {}, _want("quad-last")),
    "d128-quad-first-without": (D128, _b("quad-first-without"), {}, _want("quad-first-without")),
    "d128-riders-last": (D128, _b("riders-last"), {}, _want("riders-last")),
    "d128-riders-first-without": (D128, _b("riders-first-without"), {}, _want("riders-first-without")),
    "d128-split-last": (D128, _b("split-last"), {}, _want("split-last")),
    "d128-split-first-without": (D128, _b("split-first-without"), {}, _want("split-first-without")),
    "d64-h16-past-split": (D64_H16, lambda: _cus() // 2 + 1, {}, _narrow_whole),
    "d96-F2048-63": (D96, 63, {}, _wgrad_class_1),
    "predict-d512-F2048-520": (PRED_D512, 520, dict(forms=PREDICT_FORMS), _decode_edges),
    "predict-d32-encdec-5": (ENCDEC_D32, 5, {}, _decode), "predict-d32-encdec-33": (ENCDEC_D32, 33, {}, _decode),
    "bf16-1-d256-F2048-129": (dict(LM_1, precision=1), 129, {}, _bf16_wt(128)), "bf16-2-d256-F2048-129": (dict(LM_1, precision=2), 129, {}, _bf16_wt(128)),
    "bf16-1-d512-64": (dict(C4_1, precision=1), 64, {}, _bf16_shadows), "bf16-2-d512-64": (dict(C4_1, precision=2), 64, {}, _bf16_shadows),
    "bf16-1-d512-65": (dict(C4_1, precision=1), 65, {}, _bf16_wt(64)), "bf16-2-d512-65": (dict(C4_1, precision=2), 65, {}, _bf16_wt(64)),
    "d12-S5-1": (cfg_dict(12, 3, 7, 1, embedding_size_src=5), 1, {}, _op_path), "d12-S5-7": (cfg_dict(12, 3, 7, 1, embedding_size_src=5), 7, {}, _op_path),
    "d36-S27-1": (cfg_dict(36, 3, 40, 1, embedding_size_src=27), 1, {}, _op_path), "d36-S27-7": (cfg_dict(36, 3, 40, 1, embedding_size_src=27), 7, {}, _op_path),
    "d72-S27-1": (cfg_dict(72, 2, 100, 1, embedding_size_src=27), 1, {}, _op_path), "d72-S5-7": (cfg_dict(72, 2, 100, 1, embedding_size_src=5), 7, {}, _op_path),
}


# a 2.4 GiB workspace: no other configuration of this library reaches it within a tested batch size
FILL_KW = {"predict-d512-F2048-520": dict(other=False)}


def _case(name):
    cfg, B, kw, path = CASES[name]
    return cfg, (B() if callable(B) else B), kw, path


@pytest.mark.parametrize("name", list(CASES))
def test_fill_independence(capfd, request, name):
    cfg, B, kw, path = _case(name)
    t0 = time.time()
    trace, err = _traced(capfd, request, lambda: iso.check_fill_independence("hip", cfg, B, P, fills=("qnan",), deterministic=False, other=False, **kw))
    path(trace, err, B)
    iso.check_fill_independence("hip", cfg, B, P, **dict(kw, **FILL_KW.get(name, {})))
    _report(request, trace, err, t0)


@pytest.mark.parametrize("name", list(CASES))
def test_redzones(capfd, request, name):
    cfg, B, kw, path = _case(name)
    t0 = time.time()
    trace, err = _traced(capfd, request, lambda: iso.check_redzones("hip", cfg, B, P, deterministic=False, **kw))
    path(trace, err, B)
    _report(request, trace, err, t0)


# ---- one history per path family -------------------------------------------------------------------------------------------------------
def _gemm64_line(prefix):
    return lambda tr, err, B: [ln for ln in err.splitlines() if ln.startswith("[gemm64] " + prefix)] or pytest.fail("no [gemm64] %s line" % prefix)


def _shadows_2(tr, err, B):
    from harness import Runner
    r = Runner(dict(C4_1, precision=2, dropout=P), B, "hip")
    assert r.precision_in_force() == 2 and r.lib.cdll.gt_operand_shadow_level(__import__("ctypes").byref(r.c)) == 2
    _bf16_shadows(tr, err, B)


HISTORIES = {
    "seq-whole": (D128, _b("split-first-without"), {}, _want("split-first-without")),
    "quad-fused-launch": (D128, _b("quad-last"), {}, lambda tr, err, B: (_want("quad-last")(tr, err, B),
                                                                       [d for d in dispatched(tr, "seq_fwd") if d["fuse_b0"] == 1] or pytest.fail("no fused launch"))),
    "split-riders": (D128, _b("riders-last"), {}, lambda tr, err, B: (_want("riders-last")(tr, err, B),
                                                                     [d for d in dispatched(tr, "seq_bwd") if d["riders"] > 0] or pytest.fail("no riders"))),
    "rowx-ln64": (C4_1, 64, {}, _ring64), "rowx-ln128": (C4_1, 256, {}, _gemm64_line("ln128")), "rowx-ln32": (KS_1, 32, {}, _gemm64_line("ln32")),
    "keep-bits": (C4_1, 64, dict(flags=FALLBACK), lambda tr, err, B: (_gemm64_line("kbits write")(tr, err, B), _gemm64_line("kbits read")(tr, err, B))),
    "bf16-2-shadows": (dict(C4_1, precision=2), 64, {}, _shadows_2),
    "encoder-decoder": (ENCDEC_D32, 33, {}, _decode),
}


@pytest.mark.parametrize("name", list(HISTORIES))
def test_history_independence(capfd, request, name):
    cfg, B, kw, path = HISTORIES[name]
    B = B() if callable(B) else B
    t0 = time.time()
    out = {}

    def default_mode():
        out["bit"] = iso.check_history_independence("hip", cfg, B, P, deterministic=False, seed=1, **kw)
    trace, err = _traced(capfd, request, default_mode)
    path(trace, err, B)
    assert out["bit"] >= 2
    iso.check_history_independence("hip", cfg, B, P, **kw)
    _report(request, trace, err, t0)


# ---- the engine twin: StepEngine's own torch.empty pattern ---------------------------------------------------------------------------------
class PoisonedTorch:
    """the torch module with empty / empty_like returning tensors that hold a bit pattern; everything else is torch's"""

    def __init__(self, torch, pattern):
        self._torch, self._word, self.poisoned = torch, int(np.uint32(pattern).astype(np.int32)), 0

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def _poison(self, t):
        if t.numel() and t.element_size() % 4 == 0 and t.is_contiguous():
            t.view(self._torch.int32).fill_(self._word)
            self.poisoned += 1
        return t

    def empty(self, *a, **kw):
        return self._poison(self._torch.empty(*a, **kw))

    def empty_like(self, *a, **kw):
        return self._poison(self._torch.empty_like(*a, **kw))


def _engines(monkeypatch, poison, make, run, at_least=0):
    """run(make()) with the host modules' torch replaced (or not); the engine is made AND used under the replacement, which must have
    filled at_least allocations"""
    import torch
    from transformergrooveinfilling_amd import engine, infill
    proxy = PoisonedTorch(torch, iso.QNAN)
    with monkeypatch.context() as m:
        if poison:
            for mod in (engine, infill):
                m.setattr(mod, "torch", proxy)
        out = run(make())
        torch.cuda.synchronize()
    assert proxy.poisoned >= at_least, proxy.poisoned
    return out


def _equal(a, b):
    import torch
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert torch.equal(a[k], b[k]) and not (a[k].is_floating_point() and bool(torch.isnan(a[k]).any())), "%s differs (or holds a NaN) under poisoned torch.empty" % k


TRAIN_DIMS = dict(d_model=128, n_heads=4, dim_feedforward=512, num_encoder_layers=3, num_decoder_layers=0, dropout=0.24, embedding_size_src=16)
ENGINE_DIMS = dict(d_model=32, n_heads=4, dim_feedforward=64, num_encoder_layers=2, num_decoder_layers=1, dropout=0.1, embedding_size_src=16)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_engine_train_on_poisoned_allocations(monkeypatch, request, use_graph):
    import torch
    import parity
    from oracle import numpy_groove as ng
    from transformergrooveinfilling_amd import _lib
    from transformergrooveinfilling_amd.engine import StepEngine
    t0 = time.time()
    B = 64
    Pm = ng.init_params(TRAIN_DIMS, seed=3, perturb=0.05)
    x, y = (torch.from_numpy(a) for a in ng.synthetic_batch(100, 16, seed=5))

    def make():
        eng = StepEngine(batch_size=B, optimizer="adam", learning_rate=0.01, hit_loss_penalty=0.47, seed=7, use_graph=use_graph, **TRAIN_DIMS)
        eng.load_named(Pm)
        return eng

    def run(eng):
        out = {}
        for i in range(3):
            out["step%d" % i] = eng.train_step(x[:B], y[:B]).clone()
        eng.max_grad_norm = 0.5
        out["clipped"] = eng.train_step(x[:B], y[:B]).clone()
        eng.max_grad_norm = None
        eng.loss_opts = eng.make_loss_opts(vo_penalty=0.7, pos_weight=2.0, focal_gamma=1.5, term_weights=(1.0, 0.5, 2.0))
        out["loss_opts"] = eng.train_step(x[:B], y[:B]).clone()
        out["voice_stats"] = eng.slot(B).voice_stats.clone()
        eng.loss_opts = None
        out["eval"] = eng.forward_eval_chunked(x.cuda(), chunk=B).clone()           # 64 (the train slot) + 36
        out["params"] = eng.params.clone()
        return out

    with parity._deterministic(_lib.get_lib(), True):
        _equal(_engines(monkeypatch, True, make, run, at_least=3), _engines(monkeypatch, False, make, run))      # two slots' workspaces, the output
    _report(request, [], "", t0)


def test_engine_predict_on_poisoned_allocations(monkeypatch, request):
    """600 sequences = a chunk of 512 and a remainder of 88, then 530: the remainder workspace is replaced"""
    import torch
    import parity
    from transformergrooveinfilling_amd.engine import StepEngine
    t0 = time.time()
    cfg, Pm, x = parity.predict_inputs(cfg_dict(32, 4, 64, 2, 1), 600)
    x = torch.from_numpy(x)
    gt = (torch.rand(600, 32, 27, generator=torch.Generator().manual_seed(3)) > 0.8).float()
    thres = [0.3, 0.5, 0.4, 0.6, 0.5, 0.45, 0.55, 0.5, 0.35]

    def make():
        eng = StepEngine(batch_size=4, seed=2, **dict(ENGINE_DIMS, dropout=cfg["dropout"]))
        eng.load_named(Pm)
        return eng

    def run(eng):
        out = {"thres": eng.predict(x, chunk=512, thres=0.5).clone(), "sampled": eng.predict(x, chunk=512, pd_seed=0x5EED).clone(),
               "voices": eng.predict(x, chunk=512, voice_thresholds=thres, voice_max_count=6, temperature=0.8, mask_vo=True).clone()}
        out["curve"] = eng.hit_curve(x, gt, chunk=512).clone()
        out["metrics"] = eng.voice_metrics(out["thres"], gt.cuda()).clone()
        out["second"] = eng.predict(x[:530], chunk=512, thres=0.5).clone()
        return out

    # three chunk workspaces with their tgt scratch, five outputs, probabilities, the curve's buffers
    _equal(_engines(monkeypatch, True, make, run, at_least=12), _engines(monkeypatch, False, make, run))
    _report(request, [], "", t0)
