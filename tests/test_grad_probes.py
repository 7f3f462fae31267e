"""Each sequence's share of the parameter gradients, and accumulation onto a non-zero gradient (parity.check_grad_probes /
parity.check_accumulate), on the CPU: the check tested on the oracle alone, then both checks on the host emulator build of the kernels --
the one-kernel-per-op path, the encoder-decoder and the sequence-resident schedules the emulator reaches at up to four sequences.  The
GPU counterparts at real sizes: tests/test_grad_probes_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import parity
from harness import ROOT, cfg_dict
from oracle import numpy_groove as ng


def test_the_whole_batch_bar_accepts_a_sequence_counted_at_98_percent_and_the_probe_bar_does_not():
    """d32 / H4 / F16 / L1 at 256 sequences, oracle only.  G' = G - 0.02 G_seq128 (sequence 128's contribution counted at 98 %) passes
    check_step's bar -- max |G' - G| < GRAD_TOL max |G| per tensor; computed: 1.13e-4 in the worst tensor -- because one sequence's share
    of a tensor's largest entry is 3.3e-3 ... 5.6e-3 here.  The probe comparison for that sequence, fed 0.98 G_seq128 as the device's
    result, raises: its error is 2e-2 of the probe's own tensor.
    Should a change to the oracle move the first figure over the bar, this test fails and says so: the mutation then has to shrink (the
    share of one sequence grew), the old bar must not be widened."""
    cfg = dict(cfg_dict(32, 4, 16, 1), dropout=0.1)
    B, rng = 256, (1234, 99, 7)
    P = ng.init_params(cfg, seed=3, perturb=0.05)
    x, y = ng.synthetic_batch(B, 16, seed=5)
    (h, v, o), C = ng.forward(P, cfg, x, rng=rng, dtype=np.float64)
    _, dpred = ng.calculate_loss((h, v, o), y.astype(np.float64), 0.47)
    G = ng.backward(P, cfg, C, dpred, dtype=np.float64)
    only = [np.zeros_like(a) for a in dpred]
    for a, b in zip(only, dpred):
        a[128] = b[128]
    Gs = ng.backward(P, cfg, C, only, dtype=np.float64)
    mutated = {k: G[k] - 0.02 * Gs[k] for k in G}
    old = max(float(np.abs(mutated[k] - G[k]).max() / max(np.abs(G[k]).max(), 1e-5)) for k in G)
    share = [float(np.abs(Gs[k]).max() / np.abs(G[k]).max()) for k in G]
    print("old bar: worst error %.3g (bar %g); one sequence's share of max |G|: %.3g ... %.3g" % (old, parity.GRAD_TOL, min(share), max(share)))
    assert old < parity.GRAD_TOL, "the whole-batch bar no longer accepts the 2 %% mutation (error %.3g): the premise of this test moved" % old
    assert old > 0.25 * parity.GRAD_TOL                                    # ... and it is a mutation of substance, not rounding noise
    # (the loss's d_hvo carries the factor 1 / (32 B); a probe's is U(-1, 1): by linearity, the same gradients times 32 B)
    Gs = {k: 32 * B * g for k, g in Gs.items()}
    assert parity.probe_compare(Gs, Gs, ("seq", 128)) == 0.0
    with pytest.raises(AssertionError, match=r"probe \('seq', 128\): .* element "):
        parity.probe_compare({k: 0.98 * g for k, g in Gs.items()}, Gs, ("seq", 128))
    # a sequence counted at 99.9 %: still caught (1e-3 against the bar of 2e-4); a tensor the probe does not reach is an error, not a pass
    with pytest.raises(AssertionError):
        parity.probe_compare({k: 0.999 * g for k, g in Gs.items()}, Gs, ("seq", 128))
    with pytest.raises(ValueError, match="another probe seed"):
        parity.probe_compare(Gs, dict(Gs, **{"OutputLayer.Linear.bias": 1e-5 * Gs["OutputLayer.Linear.bias"]}), ("seq", 128))


def test_probe_placement():
    assert parity.probe_places(17) == [("seq", 0), ("seq", 16), ("row", 271), ("row", 272), ("row", 543)]
    assert parity.rider_rows(544) == [255, 256, 271, 272] and parity.rider_rows(2048) == [1023, 1024, 1023, 1024]
    pl = parity.probe_places(17, parity.rider_rows(544))                    # the tail's chunk boundary falls on rows 15 / 16 of sequence 8
    assert pl == [("seq", 0), ("seq", 16), ("row", 271), ("row", 272), ("row", 543), ("row", 255), ("row", 256)]
    assert len(parity.probe_places(64, parity.rider_rows(2048))) == 7
    assert parity.probe_places(64, [511, 512, 1536], split_rows=False) == [("seq", 0), ("seq", 63), ("row", 2047), ("row", 511), ("row", 512), ("row", 1536)]
    trace = [("wgrad_queue", dict(M=16, N=32, K=160, k_chunk=64)), ("wgrad_queue", dict(M=27, N=32, K=160, k_chunk=64)),
             ("wgrad_queue", dict(M=96, N=32, K=160, k_chunk=192)), ("wgrad_queue", dict(M=96, N=32, K=160, k_chunk=128))]
    assert parity.chunk_rows(trace, 160) == [127, 128, 128, 63, 64, 128]                       # the largest gradient's chunk length first
    assert parity.probe_places(64, [511, 512, 1536, 63, 64], split_rows=False, limit=6)[-1] == ("row", 1536)
    assert len(parity.probe_places(5, list(range(100)))) == parity.MAX_PROBES
    d = parity.probe_d_hvo(5, ("row", 100), 7)
    assert d.dtype == np.float32 and np.flatnonzero(np.abs(d).reshape(160, 27).max(1)).tolist() == [100] and np.abs(d).max() <= 1
    d = parity.probe_d_hvo(5, ("seq", 4), 7)
    assert np.flatnonzero(np.abs(d).reshape(5, -1).max(1)).tolist() == [4]


def _emu(code, env=None):
    head = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import parity, harness\nfrom harness import cfg_dict, dispatched\n"
            "def probes(rows=None):\n"
            "    return lambda trace, M: parity.probe_places(M // 32, parity.chunk_rows(trace, M) if rows is None else rows(M))\n"
            "import time\nT0 = [time.time()]\n"
            "def show(tag, trace):\n"
            "    print('CASE', tag, sorted({f for f, _ in trace}), 'probe/bar %%.3f' %% parity.FIGURES['probe'], '%%.1f s' %% (time.time() - T0[0]))\n"
            "    T0[0] = time.time()\n"
            "def accumulate(*a, **k):\n"
            "    parity.check_accumulate(*a, **k)\n"
            "    print('ACC accumulate/bar %%.3f' %% parity.FIGURES['accumulate'], '%%.1f s' %% (time.time() - T0[0]))\n"
            "    T0[0] = time.time()\n") % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", head + code + "print('ok')\n"], env=dict(os.environ, **(env or {})), capture_output=True, text=True,
                         timeout=1500)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("ok"), (out.stdout[-2000:], out.stderr[-4000:])
    print(out.stdout)
    return out


ENC, ENCDEC = cfg_dict(32, 4, 16, 2), cfg_dict(32, 4, 16, 2, 2)


def test_probes_and_accumulation_on_the_one_kernel_per_op_path():
    """d32 at 3 and 5 sequences (160 tokens: weight-gradient chunks of 128 with a partial last one) and the encoder-decoder (cross-attention q / kv
    weight gradients, the memory gradient summed over the decoder layers)"""
    out = _emu("r, tr, pl = parity.check_grad_probes('emu', %r, 3, 0.25, probes(), seq=False)\n"
               "assert dispatched(tr, 'wgrad_queue') and not dispatched(tr, ('seq_fwd', 'seq_bwd')), tr\n"
               "show('op', tr)\n"
               "r, tr, pl = parity.check_grad_probes('emu', %r, 5, 0.25, probes(), seq=False)\n"      # 160 tokens: chunks of 128, the last one 32 long
               "assert dispatched(tr, 'wgrad_queue', k_chunk=128, tail=1) and ('row', 127) in pl and ('row', 128) in pl, (tr, pl)\n"
               "show('op-chunks', tr)\n"
               "accumulate('emu', %r, 3, 0.25, seq=False)\n"
               "r, tr, pl = parity.check_grad_probes('emu', %r, 2, 0.25, probes())\n"
               "assert dispatched(tr, 'wgrad_queue') and not dispatched(tr, ('seq_fwd', 'seq_bwd')), tr\n"
               "show('encdec', tr)\n"
               "accumulate('emu', %r, 2, 0.25)\n"
               % (ENC, ENC, ENC, ENCDEC, ENCDEC))
    assert out.stdout.count("CASE") == 3, out.stdout


def test_probes_and_accumulation_on_the_sequence_resident_schedules_d32():
    """one workgroup per sequence (d32, 4 heads) and two per sequence (16 heads of 2: vector-ALU attention), their weight gradients through
    the grouped dispatch; and that dispatch in deterministic mode (one workgroup per gradient tile over all 160 tokens, where the default
    cuts them in two) on the one-kernel-per-op path"""
    out = _emu("r, tr, pl = parity.check_grad_probes('emu', %r, 3, 0.25, probes())\n"
               "assert dispatched(tr, 'seq_bwd', split=0) and dispatched(tr, 'wgrad_queue'), tr\n"
               "show('whole', tr)\n"
               "accumulate('emu', %r, 3, 0.25)\n"
               "h16 = cfg_dict(32, 16, 64, 2)\n"
               "r, tr, pl = parity.check_grad_probes('emu', h16, 2, 0.2, probes())\n"
               "assert dispatched(tr, 'seq_bwd', split=1, ride=0), tr\n"
               "show('split-h16', tr)\n"
               "accumulate('emu', h16, 2, 0.2)\n"
               "r, tr, pl = parity.check_grad_probes('emu', %r, 5, 0.1, probes(), seq=False, deterministic=True)\n"
               "q = dispatched(tr, 'wgrad_queue')\n"
               "assert q and all(d['splitk'] == 1 and d['K'] == 160 for d in q), q\n"
               "show('deterministic', tr)\n" % (ENC, ENC, ENC))
    assert out.stdout.count("CASE") == 3, out.stdout


D128 = cfg_dict(128, 4, 64, 2)                     # two layers: the in-proj riders need a layer above layer 0


def test_probes_and_accumulation_on_the_grouped_dispatch_d128():
    """d128, two workgroups per sequence, weight gradients as the grouped dispatch at the end of the backward"""
    out = _emu("r, tr, pl = parity.check_grad_probes('emu', %r, 3, 0.24, probes(), seq='split-noride')\n"
               "assert dispatched(tr, 'seq_bwd', split=1, ride=0) and dispatched(tr, 'wgrad_queue') and not dispatched(tr, 'seq_tail'), tr\n"
               "show('split-noride', tr)\n"
               "accumulate('emu', %r, 3, 0.24, seq='split-noride')\n" % (D128, D128))
    assert out.stdout.count("CASE") == 1, out.stdout


def test_probes_and_accumulation_on_the_riders_d128():
    """d128 with riders + the tail launch at 4 sequences: ride_last_k = 64 = the tail's chunk boundary (rows 63 | 64 are probed); the
    accumulating backward takes the adding store modes of the rider tiles and of the LayerNorm jobs"""
    out = _emu("r, tr, pl = parity.check_grad_probes('emu', %r, 4, 0.24, probes(parity.rider_rows), seq='split')\n"
               "assert [d for d in dispatched(tr, 'seq_bwd') if d['riders'] > 0] and dispatched(tr, 'seq_tail', kind='tail'), tr\n"
               "assert not dispatched(tr, 'wgrad_queue') and ('row', 63) in pl and ('row', 64) in pl, pl\n"
               "show('riders', tr)\n"
               "accumulate('emu', %r, 4, 0.24, seq='split')\n" % (D128, D128))
    assert out.stdout.count("CASE") == 1, out.stdout


def test_probes_on_the_bf16_operand_path():
    """precision 1: the per-operation check per probe (forward half compared once)"""
    out = _emu("r, tr, pl = parity.check_grad_probes('emu', %r, 3, 0.25, probes(), precision=1)\n"
               "assert dispatched(tr, 'wgrad_queue', prec=1) and not dispatched(tr, 'wgrad_queue', prec=0), tr\n"
               "show('bf16', tr)\n" % (ENC,))
    assert out.stdout.count("CASE") == 1, out.stdout
