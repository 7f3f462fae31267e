"""Each sequence's share of the parameter gradients (parity.check_grad_probes) and accumulation onto a non-zero gradient buffer
(parity.check_accumulate) at the sizes where the token dimension of the weight gradients is really cut: rider tiles and the tail launch,
the grouped dispatch's token chunks with a partial last one, one workgroup per tile (deterministic mode), one and two workgroups per
sequence, the encoder-decoder, 128x128 tiles over 512-token chunks, LayerNorm-in-the-epilogue launches, the bf16 kernel's 32-token slabs,
the schedule after an exchange time-out.  Every case asserts from the GT_TRACE_DISPATCH lines that the path it exists for ran; probes sit
on the partition boundaries read from that trace (parity.chunk_rows) or restated from the host rules (parity.rider_rows).

GT_GRAD_PROBES_REPORT=<file>: append one line per case (dispatch families seen, probes, error / bar ratios, wall time)."""
import ctypes
import os
import time

import pytest

import parity
from harness import cfg_dict, dispatched, trace_dispatch
from transformergrooveinfilling_amd import _lib

pytestmark = pytest.mark.gpu

FALLBACK = _lib.CFG_NO_QUAD | _lib.CFG_NO_LN_XCHG           # engine.py FALLBACK_FLAGS
EPI_RES_LN, EPI_RES_LNBWD, EPI_RES_LN_X, EPI_RES_LNBWD_X = 7, 8, 9, 10
GEMMS = ("gemm32", "gemm32h", "gemm32row", "gemm64", "gemm64h", "gemm_cfg")
D128 = cfg_dict(128, 4, 512, 2)                    # the headline shape's class; two layers: the in-proj riders need a layer above layer 0
C4_1 = cfg_dict(512, 8, 512, 1)
KS_1 = cfg_dict(256, 2, 512, 1)
ENC, ENCDEC = cfg_dict(32, 4, 16, 2), cfg_dict(32, 4, 16, 2, 2)


@pytest.fixture(autouse=True)
def _switches_back():
    """the process-wide schedule switches a Runner(seq=...) sets are put back whatever happens"""
    yield
    lib = _lib.get_lib()
    lib.cdll.gt_set_seq(1)
    lib.cdll.gt_set_seq_split(-1)
    lib.cdll.gt_set_seq_quad(-1)
    lib.cdll.gt_set_seq_ride(-1)


def _from_chunks(split_rows=True, limit=parity.MAX_PROBES):
    return lambda trace, M: parity.probe_places(M // 32, parity.chunk_rows(trace, M), split_rows=split_rows, limit=limit)


BIG = _from_chunks(False, 6)                       # the big shapes take six: the SPLIT kernels' row halves do not exist there


def _from_riders(trace, M):
    return parity.probe_places(M // 32, parity.rider_rows(M))


def _riders(tr, pl, B):
    bwd = dispatched(tr, "seq_bwd")
    assert bwd and any(d["riders"] > 0 for d in bwd) and all(d["split"] == 1 and d["ride"] == 1 for d in bwd), bwd
    assert dispatched(tr, "seq_tail", kind="tail") and not dispatched(tr, "wgrad_queue")
    M = 32 * B
    assert ("row", M // 2 // 64 * 64 - 1) in pl and ("row", M // 2 // 64 * 64) in pl, pl


def _grouped(tr, pl, B):
    bwd = dispatched(tr, "seq_bwd")
    assert bwd and all(d["split"] == 1 and d["ride"] == 0 and d["riders"] == 0 for d in bwd), bwd
    q = [d for d in dispatched(tr, "wgrad_queue") if d["K"] == 32 * B and d["splitk"] > 1]
    assert q and dispatched(tr, "wgrad_flush") and not dispatched(tr, "seq_tail"), dispatched(tr, "wgrad_queue")
    assert len(pl) >= 7, pl                          # the five fixed places and the rows either side of a chunk boundary at least


def _deterministic(tr, pl, B):
    q = dispatched(tr, "wgrad_queue")
    assert q and all(d["splitk"] == 1 and d["k_chunk"] >= 32 * B for d in q), q


def _whole(tr, pl, B):
    bwd = dispatched(tr, "seq_bwd")
    assert bwd and all(d["split"] == 0 and d["phase"] == 0 for d in bwd), bwd
    assert dispatched(tr, "seq_fwd", split=0) and dispatched(tr, "wgrad_queue")


def _one_kernel_per_op(tr, pl, B):
    assert not dispatched(tr, ("seq_fwd", "seq_bwd", "seq_tail"))
    assert dispatched(tr, "wgrad_queue", K=32 * B, tail=1), dispatched(tr, "wgrad_queue")       # 160 tokens: a partial last chunk
    assert dispatched(tr, "attn_bwd") and ("row", 127) in pl and ("row", 128) in pl, pl


def _encoder_decoder(tr, pl, B):
    assert not dispatched(tr, ("seq_fwd", "seq_bwd", "seq_tail"))
    d = ENCDEC["d_model"]
    q = dispatched(tr, "wgrad_queue", K=32 * B)
    assert [x for x in q if x["M"] == 2 * d and x["N"] == d], q        # the cross-attention k / v in-proj weight gradient (memory as operand)
    assert dispatched(tr, "ln_bwd", variant="two_norms")


def _big_tiles(tail):
    def check(tr, pl, B):
        q = [d for d in dispatched(tr, "wgrad_queue") if d["K"] == 32 * B and d["M"] >= 512 and d["N"] >= 512]
        # 128x128 tiles (class 2, or 3: the same tiles on the prefetch-ring body where 32 B is a multiple of 64), 512-token chunks
        assert q and all(d["cls"] in (2, 3) and d["k_chunk"] == 512 and d["tail"] == tail for d in q), q
        assert ("row", 511) in pl and ("row", 512) in pl and ("row", (32 * B - 1) // 512 * 512) in pl and len(pl) == 6, pl
    return check


def _row_tiles(tr, pl, B):
    # LayerNorm and LayerNorm backward in the epilogue of the d_model-wide Linears / dgrads (on tiles that own their rows, or through the
    # row exchange: the _X forms), the parameter-gradient partials of the backward ones summed by the reduce
    ln = [d for d in dispatched(tr, GEMMS, M=32 * B, N=256) if d["epi"] in (EPI_RES_LN, EPI_RES_LN_X)]
    lnb = [d for d in dispatched(tr, GEMMS, M=32 * B, N=256) if d["epi"] in (EPI_RES_LNBWD, EPI_RES_LNBWD_X)]
    # (one layer: out-proj + norm1 forward, linear1 dgrad + norm1 backward; the layer's closing norm runs with the final norm as a row pass)
    assert ln and lnb, sorted({(d["N"], d["epi"]) for f, d in tr if f in GEMMS})
    assert dispatched(tr, "ln_param_reduce") and dispatched(tr, "wgrad_queue", K=32 * B)


def _bf16_slabs(tr, pl, B):
    q = [d for d in dispatched(tr, "wgrad_queue") if d["K"] == 32 * B and d["M"] >= 512 and d["N"] >= 512]
    assert q and all(d["cls"] in (4, 5) and d["prec"] == 1 for d in q), q      # staged from the operands' bf16 shadows
    assert not dispatched(tr, "wgrad_queue", prec=0)


def _fallback(tr, pl, B):
    fwd, bwd = dispatched(tr, "seq_fwd"), dispatched(tr, "seq_bwd")
    assert fwd and all(d["split"] == 1 and d["quad"] == 0 and d["fuse_b0"] == 0 for d in fwd), fwd
    assert {d["phase"] for d in bwd} == {0, 1, 2} and all(d["quad"] == 0 for d in bwd), bwd
    _riders(tr, pl, B)


#        name: (cfg, B, p, probes, keywords of check_grad_probes, accumulate too?, what the trace must show)
CASES = {
    # M 544: ride_last_k 256 on a sequence boundary, the tail's chunk boundary 272 inside sequence 8 (its rows 15 | 16)
    "riders": (D128, 17, 0.24, _from_riders, dict(), True, _riders),
    "riders-full": (D128, 64, 0.24, _from_riders, dict(), True, _riders),                  # ride_last_k = the tail's boundary = 1024
    "grouped-dispatch": (D128, 17, 0.24, _from_chunks(), dict(seq="split-noride"), True, _grouped),
    # one workgroup per gradient tile over all tokens -- on the paths that queue weight gradients (the riders do not consult the switch)
    "deterministic": (D128, 17, 0.1, _from_chunks(), dict(seq="split-noride", deterministic=True), False, _deterministic),
    "deterministic-op": (D128, 17, 0.1, _from_chunks(), dict(seq=False, deterministic=True), False, _deterministic),
    "whole-d32-h16": (cfg_dict(32, 16, 512, 2), 16, 0.2, _from_chunks(), dict(seq="whole"), True, _whole),          # head_dim 2
    "whole-d64-h16": (cfg_dict(64, 16, 256, 2), 16, 0.2, _from_chunks(), dict(seq="whole"), True, _whole),          # head_dim 4
    "one-kernel-per-op": (ENC, 5, 0.25, _from_chunks(), dict(seq=False), True, _one_kernel_per_op),
    "encoder-decoder": (ENCDEC, 3, 0.25, _from_chunks(), dict(), True, _encoder_decoder),
    "tiles-128-B64": (C4_1, 64, 0.15, BIG, dict(), False, _big_tiles(0)),
    "tiles-128-B72": (C4_1, 72, 0.15, BIG, dict(), False, _big_tiles(1)),      # M 2304: 4.5 chunks
    "row-tiles": (KS_1, 64, 0.3, BIG, dict(), False, _row_tiles),
    "bf16-slabs": (C4_1, 64, 0.24, BIG, dict(precision=1), False, _bf16_slabs),
    "fallback-schedule": (D128, 17, 0.24, _from_riders, dict(flags=FALLBACK), True, _fallback),
}


@pytest.mark.parametrize("case", list(CASES))
def test_grad_probes(case):
    cfg, B, p, probes, kw, acc, path = CASES[case]
    t0 = time.time()
    r, trace, places = parity.check_grad_probes("hip", cfg, B, p, probes, **kw)
    figures = dict(parity.FIGURES)
    path(trace, places, B)
    if case == "bf16-slabs":
        assert r.precision_in_force() == 1 and r.lib.cdll.gt_operand_shadow_level(ctypes.byref(r.c)) == 2
    if acc:
        akw = {k: v for k, v in kw.items() if k in ("seq", "flags")}
        _, atrace = trace_dispatch(lambda: parity.check_accumulate("hip", cfg, B, p, **akw))
        figures["accumulate"] = parity.FIGURES["accumulate"]
        path(atrace, places, B)                      # the accumulating backwards took the same path
    report = os.environ.get("GT_GRAD_PROBES_REPORT")
    if report:
        with open(report, "a") as f:
            f.write("%s | %s | %d probes | %s | %.1f s\n" % (case, " ".join(sorted({fam for fam, _ in trace})), len(places),
                                                          " ".join("%s/bar %.3f" % kv for kv in sorted(figures.items())), time.time() - t0))
