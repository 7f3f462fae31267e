"""Oracle parity on the far side of the host dispatch rules (DESIGN.md "Dispatch trace", table "rule -> boundary batch -> test"):
the schedule an engine trains on after an exchange time-out (gt_config.flags = NO_QUAD | NO_LN_XCHG), batches whose token count 32 B is
no multiple of the large tiles (generic 64x64 / 128x128 tiles, 64-row row tiles and weight-gradient chunks with a partial last tile), and
the batches at which the sequence-resident schedule changes (QUAD / riders / SPLIT against the CU count).  Every case is one of the
project's parity checks with its bars unchanged, and asserts from the GT_TRACE_DISPATCH lines that the path it exists for really ran.

GT_DISPATCH_EDGES_REPORT=<file>: append one line per case (dispatch families seen, error / bar ratios, wall time)."""
import os
import time

import pytest

import harness
import parity
from harness import Runner, cfg_dict, dispatched, parse_dispatch
from transformergrooveinfilling_amd import _lib

pytestmark = pytest.mark.gpu

FALLBACK = _lib.CFG_NO_QUAD | _lib.CFG_NO_LN_XCHG           # engine.py FALLBACK_FLAGS
EPI_STORE, EPI_RELU_DROP, EPI_MASK_NZ, EPI_RES_LN, EPI_RES_LNBWD = 0, 3, 5, 7, 8
RING = ("gemm32", "gemm32h", "gemm32row", "gemm64", "gemm64h")
GEMMS = RING + ("gemm_cfg",)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _traced(capfd, request, *checks):
    """Run the checks (callables) with the dispatch trace (and the [gemm64] lines) on; returns (parsed [dispatch] lines, whole stderr).
    The environment and the process-wide schedule switches a Runner(seq=...) sets are put back whatever happens."""
    lib = _lib.get_lib()
    os.environ["GT_TRACE_DISPATCH"] = harness.TRACE_LEVEL
    os.environ["GT_TRACE_GEMM64"] = "1"
    figures = {}
    t0 = time.time()
    try:
        capfd.readouterr()
        for check in checks:
            parity.FIGURES.clear()
            check()
            for k, v in parity.FIGURES.items():
                figures[k] = max(figures.get(k, 0.0), v)
        err = capfd.readouterr().err
    finally:
        del os.environ["GT_TRACE_DISPATCH"]
        del os.environ["GT_TRACE_GEMM64"]
        lib.cdll.gt_set_seq(1)                      # (what every Runner sets for seq=True)
        lib.cdll.gt_set_seq_split(-1)
        lib.cdll.gt_set_seq_quad(-1)
        lib.cdll.gt_set_seq_ride(-1)
    trace = parse_dispatch(err)
    assert trace, "no [dispatch] line: the trace is off"
    report = os.environ.get("GT_DISPATCH_EDGES_REPORT")
    if report:
        with open(report, "a") as f:
            f.write("%s | %s | %s | %.1f s\n" % (request.node.name, " ".join(sorted({fam for fam, _ in trace})),
                                                " ".join("%s/bar %.3f" % kv for kv in sorted(figures.items())) or "-", time.time() - t0))
    return trace, err


def _no_ln_exchange(trace, err):
    """no LayerNorm-in-the-epilogue launch through the row exchange, on any tile (ln64 / ln128 / ln32)"""
    assert not dispatched(trace, GEMMS, rowx=1), dispatched(trace, GEMMS, rowx=1)[:3]
    assert not [ln for ln in err.splitlines() if ln.startswith("[gemm64] ln")]


# ================================================================================================ C1: the time-out fall-back schedule
C2_SHAPE = cfg_dict(128, 4, 512, 3)
C4_1 = cfg_dict(512, 8, 512, 1)
KS_1 = cfg_dict(256, 2, 512, 1)                    # the K&S / Random YAML shape, one layer


@pytest.mark.parametrize("how", ["flags", "split-noquad"])
@pytest.mark.parametrize("check", ["step", "train"])
def test_fallback_split_forward_d128(capfd, request, how, check):
    """d_model 128 after a time-out: the two-workgroups-per-sequence SPLIT forward, riders in the backward, no backward phase 0 behind the
    forward -- through the engine's flags, and through the process-wide switch the flags replace (each against the oracle on its own)."""
    kw = dict(flags=FALLBACK) if how == "flags" else dict(seq="split-noquad")
    fn = parity.check_step if check == "step" else parity.check_train_step
    trace, err = _traced(capfd, request, lambda: fn("hip", C2_SHAPE, 64, 0.24, **kw))
    fwd, bwd = dispatched(trace, "seq_fwd"), dispatched(trace, "seq_bwd")
    assert fwd and bwd
    assert all(d["split"] == 1 and d["quad"] == 0 and d["ride"] == 1 and d["fuse_b0"] == 0 for d in fwd), fwd[:4]
    assert all(d["quad"] == 0 and d["fuse_b0"] == 0 for d in bwd), bwd[:4]
    assert {d["phase"] for d in bwd} == {0, 1, 2, 3}                    # phase 0 is a backward launch of its own again
    assert any(d["riders"] > 0 for d in bwd)
    if check == "train":
        assert dispatched(trace, "update", kind="folded_pack")


@pytest.mark.parametrize("check", ["step", "train", "bf16-1", "bf16-2"])
def test_fallback_d512_gemm_then_row_pass(capfd, request, check):
    """d_model 512 at 2048 tokens after a time-out: the Linears on the 64x64 ring tiles (bf16: on their bf16-source forms), every LayerNorm
    and LayerNorm backward as a row pass of its own."""
    fn = {"step": lambda: parity.check_step("hip", C4_1, 64, 0.2, flags=FALLBACK),
          "train": lambda: parity.check_train_step("hip", C4_1, 64, 0.2, flags=FALLBACK),
          "bf16-1": lambda: parity.check_step_bf16("hip", C4_1, 64, 0.2, flags=FALLBACK),
          "bf16-2": lambda: parity.check_step_bf16("hip", C4_1, 64, 0.2, precision=2, flags=FALLBACK)}[check]
    trace, err = _traced(capfd, request, fn)
    _no_ln_exchange(trace, err)
    prec = 0 if check in ("step", "train") else 1
    # out-proj / linear2 (N = d_model, plain store) and their dgrads on a ring tile, then the norm
    assert dispatched(trace, RING, N=512, epi=EPI_STORE, prec=prec)
    if prec == 0:
        assert dispatched(trace, "gemm64", M=2048, N=512, K=512, form="NT", epi=EPI_STORE)
        assert dispatched(trace, "gemm64", M=2048, N=512, form="NN", epi=EPI_STORE)
    assert dispatched(trace, "ln_fwd", M=2048, d=512) and dispatched(trace, "ln_bwd", M=2048, d=512)
    assert not dispatched(trace, GEMMS, epi=EPI_RES_LN) and not dispatched(trace, GEMMS, epi=EPI_RES_LNBWD)


@pytest.mark.parametrize("B,bm", [(256, 32), (512, 64)])
def test_fallback_d256_row_owning_tiles(capfd, request, B, bm):
    """d_model 256 from GT_ROW_FUSE_MIN_M tokens after a time-out: the row-owning tiles on the ring body, 32 rows per workgroup below
    GT_ROW32_BM64_MIN_WG workgroups of 64 and 64 rows from there"""
    trace, err = _traced(capfd, request, lambda: parity.check_step("hip", KS_1, B, 0.2, flags=FALLBACK))
    _no_ln_exchange(trace, err)
    assert dispatched(trace, "gemm32row", BM=bm, M=32 * B, N=256, epi=EPI_RES_LN, form="NT")
    assert dispatched(trace, "gemm32row", BM=bm, M=32 * B, N=256, epi=EPI_RES_LNBWD, form="NN")
    assert not dispatched(trace, "gemm32row", BM=96 - bm)


@pytest.mark.parametrize("check", ["step", "train"])
def test_fallback_d256_yaml_batch(capfd, request, check):
    """the K&S YAML shape at its batch of 32 (1024 tokens) without the 32x32-tile row exchange: plain GEMM + row pass"""
    fn = parity.check_step if check == "step" else parity.check_train_step
    trace, err = _traced(capfd, request, lambda: fn("hip", KS_1, 32, 0.2, flags=FALLBACK))
    _no_ln_exchange(trace, err)
    assert dispatched(trace, "ln_fwd", M=1024, d=256) and dispatched(trace, "ln_bwd", M=1024, d=256)
    assert dispatched(trace, GEMMS, M=1024, N=256, epi=EPI_STORE)


def test_fallback_encoder_decoder(capfd, request):
    trace, err = _traced(capfd, request, lambda: parity.check_step("hip", cfg_dict(256, 2, 512, 1, 1), 64, 0.2, flags=FALLBACK))
    _no_ln_exchange(trace, err)
    assert len(dispatched(trace, "ln_fwd", M=2048, d=256)) >= 5          # 2 encoder + 3 decoder norms (the final ones ride along)
    assert dispatched(trace, "ln_bwd", variant="two_norms")


# ================================================================================================ C2: partial large tiles (flags = 0)
LM_1 = cfg_dict(256, 2, 2048, 1)                   # the lm YAML's dim_feedforward, one layer


def _wgrad_tail(trace, cls):
    q = dispatched(trace, "wgrad_queue", cls=cls, tail=1)
    assert q, [d for d in dispatched(trace, "wgrad_queue")][:8]
    assert dispatched(trace, "wgrad_flush", cls=cls)
    return q


def test_partial_64_tile_ffn(capfd, request):
    """M = 1056 (33 sequences): FFN1 and the FFN2 dgrad have 17 x 32 tiles of 64x64 -- past GT_T64_MIN, M % 64 = 32 keeps them off the ring
    tile -- the last row tile is half full"""
    trace, _ = _traced(capfd, request, lambda: parity.check_step("hip", LM_1, 33, 0.2))
    assert dispatched(trace, "gemm_cfg", BM=64, BN=64, M=1056, N=2048, K=256, form="NT", epi=EPI_RELU_DROP, edge=1)
    assert dispatched(trace, "gemm_cfg", BM=64, BN=64, M=1056, N=2048, K=256, form="NN", epi=EPI_MASK_NZ, edge=1)
    assert not dispatched(trace, RING, M=1056)


@pytest.mark.parametrize("B", [129, 130, 131])
def test_partial_128_tile_ffn(capfd, request, B):
    """M % 128 = 32, 64, 96 at 33 x 16 tiles of 128x128 (GT_T128_MIN reached): the generic 128x128 tile with a partial last row tile.
    B = 130 has M % 64 == 0 but 65 x 32 tiles of 64x64 exceed GT_T64R_MAX: neither ring tile.  The FFN weight gradients go to
    wgrad_group_kernel<4> (class 2) with a 32 / 96-token tail in the last 512-token chunk; at B = 130 the token count is a multiple of 64,
    which is all wgrad32_ok asks of it: the ring body (class 3) with a 64-token tail."""
    M = 32 * B
    trace, _ = _traced(capfd, request, lambda: parity.check_step("hip", LM_1, B, 0.2))
    assert dispatched(trace, "gemm_cfg", BM=128, BN=128, M=M, N=2048, K=256, form="NT", epi=EPI_RELU_DROP, edge=1)
    assert dispatched(trace, "gemm_cfg", BM=128, BN=128, M=M, N=2048, K=256, form="NN", epi=EPI_MASK_NZ, edge=1)
    assert not dispatched(trace, RING, M=M, N=2048)
    q = _wgrad_tail(trace, 3 if B == 130 else 2)
    assert any(d["K"] == M and d["M"] == 2048 and d["N"] == 256 and d["k_chunk"] == 512 for d in q), q


def test_partial_64_tile_qkv_d512(capfd, request):
    """d_model 512 at M = 1376 (43 sequences): the QKV projection has 22 x 24 tiles of 64x64 with a half row tile"""
    trace, _ = _traced(capfd, request, lambda: parity.check_step("hip", C4_1, 43, 0.2))
    assert dispatched(trace, "gemm_cfg", BM=64, BN=64, M=1376, N=1536, K=512, form="NT", epi=EPI_STORE, edge=1)
    assert not dispatched(trace, RING, M=1376)


@pytest.mark.parametrize("B", [65, 66])
def test_ring64_multiple_of_64_rule(capfd, request, B):
    """one batch either side of the 64x64 ring tile's M % 64 == 0 rule, inside its tile range (33 x 8 ... 33 x 24 tiles)"""
    trace, _ = _traced(capfd, request, lambda: parity.check_step("hip", C4_1, B, 0.2))
    ring = dispatched(trace, ("gemm64", "gemm64h"))
    if B == 66:
        assert ring and all(d["M"] == 2112 for d in ring)
    else:
        assert not ring and not dispatched(trace, RING)
        assert dispatched(trace, "gemm_cfg", M=2080, N=1536, edge=1)
        _wgrad_tail(trace, 2)


def test_partial_64_row_tile(capfd, request):
    """M = 16416 (513 sequences) at d_model 256: M % 64 = 32 takes the step off the row exchange and off the ring-body row tiles; the
    generic row-owning tiles are 64 rows high from GT_ROW_BM64_MIN tokens and the last one is half full (LayerNorm-backward partials:
    ceil(M / 64) rows)"""
    trace, _ = _traced(capfd, request, lambda: parity.check_step("hip", KS_1, 513, 0.2))
    assert dispatched(trace, "gemm_cfg", BM=64, BN=256, M=16416, N=256, row=1, epi=EPI_RES_LN, edge=1)
    assert dispatched(trace, "gemm_cfg", BM=64, BN=256, M=16416, N=256, row=1, epi=EPI_RES_LNBWD, form="NN", edge=1)
    assert not dispatched(trace, RING)
    _wgrad_tail(trace, 2)


def test_wgrad_class_1_tail(capfd, request):
    """wgrad_group_kernel<2> (class 1, 64x64 tiles) is reachable on the one-kernel-per-op path only where a gradient is under 128 wide and
    long: d_model 96 (two heads of 48: outside the sequence-resident class, and the generic attention kernels) with dim_feedforward 2048 at
    2016 tokens -- 32 x 2 tiles x 8 chunks of 256 tokens, the last chunk 224 long"""
    trace, _ = _traced(capfd, request, lambda: parity.check_step("hip", cfg_dict(96, 2, 2048, 1), 63, 0.2))
    q = _wgrad_tail(trace, 1)
    assert any(d["M"] == 2048 and d["N"] == 96 and d["K"] == 2016 and d["k_chunk"] == 256 for d in q), q
    assert dispatched(trace, "attn_fwd", kernel="generic") and dispatched(trace, "attn_bwd", kernel="generic")
    assert dispatched(trace, "gemm_cfg", BM=64, BN=64, M=2016, N=2048, edge=1)


@pytest.mark.parametrize("cfg,B", [(LM_1, 129), (C4_1, 65)])
def test_partial_tiles_bf16_operands(capfd, request, cfg, B):
    """precision 1 where M % 128 != 0 rules the operand shadows out: fp32 W^T copies (bf16_wt), every Linear on the generic kernel's bf16
    body with a partial row tile -- at thousands of tokens"""
    M = 32 * B
    trace, _ = _traced(capfd, request, lambda: parity.check_step_bf16("hip", cfg, B, 0.2))
    big = dispatched(trace, "gemm_cfg", M=M, prec=1, edge=1)
    assert any(d["BM"] == (128 if cfg is LM_1 else 64) for d in big), big[:6]
    assert not dispatched(trace, ("gemm32h", "gemm64h")) and not dispatched(trace, GEMMS, prec=0)
    # every dgrad of the encoder layer in the NT form over the transposed copy (the 27-wide output layer has none)
    assert not [d for d in dispatched(trace, "gemm_cfg", M=M, form="NN") if d["K"] != 27]
    assert not dispatched(trace, "wgrad_queue", cls=4) and not dispatched(trace, "wgrad_queue", cls=5)


def test_precision_2_falls_back_off_the_tile(capfd, request):
    out = {}

    def check():
        out["r"] = parity.check_step_bf16("hip", C4_1, 65, 0.2, precision=2)[0]
    trace, _ = _traced(capfd, request, check)
    assert out["r"].precision_in_force() == 1
    assert dispatched(trace, "gemm_cfg", M=2080, prec=1, edge=1) and not dispatched(trace, ("gemm32h", "gemm64h"))
    assert not dispatched(trace, ("attn_fwd", "attn_bwd"), kernel="lds64-bf16")


# ================================================================================================ C3: sequence-resident batch boundaries
D128 = cfg_dict(128, 4, 64, 2)


def _schedule(trace):
    fwd, bwd = dispatched(trace, "seq_fwd"), dispatched(trace, "seq_bwd")
    assert fwd and bwd
    sched = {(d["split"], d["quad"], d["ride"]) for d in fwd}
    assert len(sched) == 1, fwd
    split, quad, ride = sched.pop()
    assert all(d["split"] == split and d["ride"] == ride for d in bwd), bwd
    return split, quad, ride


def _d128_boundaries():
    cus = _cus()
    return {"quad-last": (cus // 4, (1, 1, 1)), "quad-first-without": (cus // 4 + 1, (1, 0, 1)),
            "riders-last": ((cus - 96) // 2, (1, 0, 1)), "riders-first-without": ((cus - 96) // 2 + 1, (1, 0, 0)),
            "split-last": (cus // 2, (1, 0, 0)), "split-first-without": (cus // 2 + 1, (0, 0, 0))}


@pytest.mark.parametrize("edge", ["quad-last", "quad-first-without", "riders-last", "riders-first-without", "split-last", "split-first-without"])
def test_seq_schedule_boundaries_d128(capfd, request, edge):
    """QUAD needs 4 B <= CUs, riders CUs - 2 B >= GT_SEQ_RIDE_MIN_IDLE (96), SPLIT 2 B <= CUs: the last batch on each schedule and the first
    past it, from the device's CU count"""
    B, want = _d128_boundaries()[edge]
    trace, _ = _traced(capfd, request, lambda: parity.check_step("hip", D128, B, 0.1))
    assert _schedule(trace) == want, (B, _schedule(trace), want)


def test_seq_schedule_boundary_d128_wide_input(capfd, request):
    B, want = _d128_boundaries()["quad-first-without"]
    trace, _ = _traced(capfd, request, lambda: parity.check_step("hip", dict(D128, embedding_size_src=27), B, 0.1))
    assert _schedule(trace) == want


@pytest.mark.parametrize("edge", ["quad-first-without", "split-first-without"])
def test_seq_schedule_boundaries_d128_train(capfd, request, edge):
    """three train steps right past the QUAD and the SPLIT boundary: the folded update's weight packs (check_train_step asserts them bit
    for bit) are what the next step's schedule reads"""
    B, want = _d128_boundaries()[edge]
    trace, _ = _traced(capfd, request, lambda: parity.check_train_step("hip", D128, B, 0.1))
    assert _schedule(trace) == want
    assert all(d["fuse_b0"] == 0 for d in dispatched(trace, "seq_fwd"))
    assert len(dispatched(trace, "update", kind="folded_pack")) == 3 and len(dispatched(trace, "seq_pack")) == 1


@pytest.mark.parametrize("cfg", [cfg_dict(32, 16, 64, 2), cfg_dict(64, 16, 256, 2)], ids=["d32", "d64"])
@pytest.mark.parametrize("past", [0, 1])
def test_seq_split_boundary_narrow(capfd, request, cfg, past):
    """the d_model 32 / 64 SPLIT families (16 heads) at the same 2 B <= CUs edge"""
    B = _cus() // 2 + past
    trace, _ = _traced(capfd, request, lambda: parity.check_step("hip", cfg, B, 0.1))
    assert _schedule(trace)[0] == 1 - past


def test_seq_bucketed_backward_past_quad(capfd, request):
    """the bucket cut of the data-parallel backward exists exactly where the weight gradients ride (grad_split): read, not assumed"""
    B = _cus() // 4 + 1
    r = Runner(dict(D128, dropout=0.1), B, "hip")
    nb = len(r.lib.grad_buckets(r.c))
    trace, _ = _traced(capfd, request, lambda: parity.check_bucketed_backward("hip", D128, B, 0.1, nb, exact=False))
    ride = _schedule(trace)[2]
    assert nb == (2 if ride else 1), (nb, ride)
    assert ride == 1 and dispatched(trace, "seq_tail", kind="out_early")


def test_step_handoffs_stay_inside_their_call(capfd):
    """the GPU twin of tests/test_emu_kernels.py::test_step_handoffs_stay_inside_their_call (same shape, same launch sequences)"""
    os.environ["GT_TRACE_DISPATCH"] = harness.TRACE_LEVEL
    try:
        parity.check_step_handoffs("hip", lambda: parse_dispatch(capfd.readouterr().err))
    finally:
        del os.environ["GT_TRACE_DISPATCH"]
