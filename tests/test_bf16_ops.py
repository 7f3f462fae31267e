"""The per-operation parity proof of the bf16 modes (parity.check_ops_bf16) proves its own closure, on the host emulator: the walk's ledger
leaves no gradient tensor uncompared and reads no device tensor that an earlier operation did not compare; the ledger itself raises when
a comparison is taken away; and the closed walk holds away from initialisation (tests/regimes.py: peaked softmax, shifted score rows,
LayerNorm variances at eps, saturated heads) under its fixed class bars.  tests/test_bf16_ops_gpu.py runs the same through the HIP library,
and the wide shapes only there (profiles/bf16_ops.txt: the ratios per bar class, the ledger's verdict on the walk before it was closed, the
mutation record)."""
import os
import subprocess

import pytest

import harness
import parity
from harness import cfg_dict

#        name: (cfg, B, dropout)
CASES = {
    "d32-h4": (cfg_dict(32, 4, 16, 2), 3, 0.1),                        # encoder-only: the output layer's dgrad feeds the two-norm row pass
    "encdec-d32-h4": (cfg_dict(32, 4, 16, 1, 1), 2, 0.1),              # causal and cross attention, three norms per decoder layer
}
P2_CASE = (cfg_dict(256, 4, 128, 1), 4, 0.1)     # precision 2 in force under the lowered-threshold emulator build of tests/test_emu_kernels.py
SEED = 5                         # of the parameters and the batch: picked on the CPU -- the fp64 oracle alone meets every regime's condition on every case
#                                  here and in tests/test_bf16_ops_gpu.py (3 and 4 miss shift at d_model 256: layer 0's row maxima stop at -83 / +61)
REGIMES = ("peaked", "shift", "flat")            # on every case; saturated (d loss / d logits) on the first
RUNS = [(c, g) for c in CASES for g in REGIMES] + [("d32-h4", "saturated")]


def run_walk(backend, cases, case, regime, precision=1):
    cfg, B, p = cases[case]
    try:
        r, _, _ = parity.check_step_bf16(backend, cfg, B, p, seed=SEED, precision=precision, regime=regime)
        assert r.precision_in_force() == precision
    finally:
        f, g = parity.FIGURES, parity.BF16_FIGURES
        print("%s %s %s precision %d: worst %.3f of its bar at %s; end to end %.3f (max-abs %.3f); widened %s"
              % (backend, case, regime, precision, f.get("bf16_op", -1), g.get("op_at"), f.get("bf16_e2e", -1), f.get("bf16_out_max", -1), g.get("widened", [])))
        for cls, (ratio, what) in sorted(g.get("ops", {}).items()):
            print("    %-78s %.4f  %s" % (cls, ratio, what))


# what the walk did not compare before it kept a ledger, per model kind: each must now be the compared output of some operation
HOLES = {
    "d32-h4": ["ctx[0]", "ctx[1]", "P[1]", "dlogits[0]", "dzA[1]", "dzAm[1]", "dzAm[0]", "dqkv[0]", "dqkv[1]", "rstd1[0]", "xhat2[0]", "rstd2[1]", "enc_xhat[0]",
               "enc_rstd[0]"],
    "encdec-d32-h4": ["ctx[0]", "ctx[1]", "P[1]", "Px[1]", "ctxx[1]", "dlogits[0]", "dzA[1]", "dzAm[1]", "dzBm[1]", "dzC[1]", "dzCm[1]", "dqkvx[1]", "dqkv[1]",
                      "dqkv[0]", "rstdx[1]", "enc_xhat[0]", "enc_rstd[0]"],
}


@pytest.mark.parametrize("case", list(CASES))
def test_walk_is_closed_and_complete(case):
    cfg, B, p = CASES[case]
    r, P, G = parity.check_step_bf16("emu", cfg, B, p)
    led = parity.BF16_FIGURES["ledger"]
    assert led.verdict() == ([], [])
    assert set(led.cover) == set(G) and all(c.all() for c in led.cover.values())
    assert led.consumed and all(how is not None and how.startswith("compared: ") for how in led.consumed.values()), led.consumed
    assert "d_hvo" not in led.consumed               # (the loss's: d loss / d logits is restated from hvo, y and the penalty)
    for t in HOLES[case]:
        assert t in led.compared, t
    # every region of the workspace the walk read is one gt_ws_find knows, at that layer
    for key in led.consumed:
        if key != "hvo":
            name, layer = key[:-1].split("[")
            r.lib.ws_find(r.c, name, int(layer))


@pytest.mark.parametrize("gone,names", [("ctx[0]", r"ctx\[0\]"), ("dlogits[0]", r"dlogits\[0\]"), ("dzAm[1]", r"dzAm\[1\]"),
                                        (("grad", "Encoder.Encoder.layers.0.norm2.weight"), r"layers\.0\.norm2\.weight"),
                                        (("grad", "Encoder.Encoder.layers.1.self_attn.in_proj_weight"), r"layers\.1\.self_attn\.in_proj_weight")])
def test_ledger_raises_when_a_comparison_is_removed(monkeypatch, gone, names):
    real = parity._ledger_compare

    def without(led, key, dev, ref, what, **kw):
        if key == gone or (isinstance(key, tuple) and key[:2] == gone):
            return                                   # this one comparison does not take place
        real(led, key, dev, ref, what, **kw)

    monkeypatch.setattr(parity, "_ledger_compare", without)
    cfg, B, p = CASES["d32-h4"]
    with pytest.raises(AssertionError, match="not closed.*" + names):
        parity.check_step_bf16("emu", cfg, B, p)


def test_ledger_names_a_slice_of_a_packed_gradient(monkeypatch):
    real = parity._ledger_compare
    key = "Decoder.Decoder.layers.0.multihead_attn.in_proj_weight"

    def without(led, k, dev, ref, what, **kw):
        if isinstance(k, tuple) and k[1] == key and k[2] == slice(32, 96):
            return                                   # the k / v rows of the cross-attention in-proj weight stay uncompared
        real(led, k, dev, ref, what, **kw)

    monkeypatch.setattr(parity, "_ledger_compare", without)
    cfg, B, p = CASES["encdec-d32-h4"]
    with pytest.raises(AssertionError, match=r"not closed.*multihead_attn\.in_proj_weight rows 32\.\.95"):
        parity.check_step_bf16("emu", cfg, B, p)


def test_probe_walks_assert_closure_too():
    """check_grad_probes(precision=1): the probes after the first skip the forward's comparisons (forward_checks=False) -- the ledger says so
    and the closure assertion runs all the same; d_hvo is the probe's own"""
    cfg, B, _ = CASES["d32-h4"]
    parity.check_grad_probes("emu", cfg, B, 0.1, [("seq", 0), ("row", 32 * B - 1)], precision=1)
    led = parity.BF16_FIGURES["ledger"]              # of the last probe
    assert led.forward_by_first_walk and led.verdict() == ([], [])
    assert led.consumed["d_hvo"] == "supplied by the test (probe)"
    assert led.compared["ctx[0]"].endswith("(by the first walk of this forward)") and "first walk" not in led.compared["dlogits[0]"]


@pytest.mark.parametrize("case,regime", RUNS)
def test_walk_in_regime(case, regime):
    run_walk("emu", CASES, case, regime)


def test_walk_in_regime_precision_2():
    """precision 2 in force: the emulator library built with the tile thresholds lowered (as tests/test_emu_kernels.py builds it), in a
    subprocess -- the harness's library handle is process-wide"""
    from test_emu_kernels import _emu_subprocess
    so = os.path.join(harness.ROOT, "tests", "emu", "libgroove_emu_big.so")
    subprocess.check_call([os.path.join(harness.ROOT, "tests", "emu", "build_emu.sh"), "-DGT_T128_BIG_MIN=1", "-DGT_T128H_MIN=1", "-DGT_WGRAD_T128_MIN=1",
                           "-DGT_ROW32_MIN_M=64", "-DGT_ROW_FUSE_MIN_M=64", "-DGT_ATTN_BWD_LDS_MIN=1"], env=dict(os.environ, GT_EMU_OUT=so),
                          stdout=subprocess.DEVNULL)
    out = _emu_subprocess("import test_bf16_ops as T\n"
                          "for regime in T.REGIMES:\n"
                          "    T.run_walk('emu', {'p2': T.P2_CASE}, 'p2', regime, precision=2)\n", dict(GT_EMU_LIB_PATH=so))
    print(out.stdout)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
