"""Global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, norm type 2) without a GPU: gt_clip_grad_norm's two kernels against
numpy in fp64, the zero-gap contract of the flat gradient buffer they rely on, StepEngine's clipped step against the manual sequence
(backward, torch's clip, update), the exchanges' fail-safe, the data-parallel step over gloo, the drop-in function and train.py's
configuration.  The kernels run in the host-emulator build of the same sources (tests/emu); tests/test_clip_grad_norm_gpu.py repeats
the kernel and engine cases on the GPU."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest
import torch

from harness import Runner, cfg_dict, emu_lib, run_ranks
from transformergrooveinfilling_amd import _lib, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (d_model, n_heads, dim_feedforward, encoder layers, decoder layers)
KERNEL_SHAPES = {"d32_h16_l6": (32, 16, 512, 6, 0), "d128_h4_f512_l3": (128, 4, 512, 3, 0), "d512_l1": (512, 8, 2048, 1, 0),
                 "encdec_d32_l2_2": (32, 4, 64, 2, 2)}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if device.type == "cuda" else ctypes.c_void_p(0)


def _sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize()


def _state(device, grad_scale=1.0):
    st = _lib.GtStepState(1, 2, 0, 0, 0.05, grad_scale, 0.9, 0.999, 1e-8)
    return torch.from_numpy(np.frombuffer(bytes(st), dtype=np.uint8).copy()).to(device)


def _random_grads(total, entries, seed):
    """random values inside the layout's tensors, zeros in the alignment gaps, a huge guard element (it must never count)"""
    rng = np.random.default_rng(seed)
    g = np.zeros(total, np.float32)
    for off, size, _, _ in entries:
        g[off:off + size] = (rng.standard_normal(size) * rng.uniform(1e-3, 1e-1)).astype(np.float32)
    g[-1] = np.float32(1e30)
    return g


def _clip(lib, cfg, g, state, max_norm, out, scratch, device):
    lib.call("gt_clip_grad_norm", ctypes.byref(cfg), _ptr(g), _ptr(state), ctypes.c_float(max_norm), _ptr(out), _ptr(scratch),
             _stream(device))
    _sync(device)


def check_kernels(lib, device, dims, seed=0):
    """gt_clip_grad_norm on one shape's flat buffer (lib: the emulator or the HIP library, device: where the buffers live)"""
    device = torch.device(device)
    d, H, F, L, Ld = dims
    cfg = _lib.make_config(2, 16, d, H, F, L, Ld)
    total, entries = lib.param_layout(cfg)
    g0 = _random_grads(total, entries, seed)
    ref = float(np.sqrt(np.sum(g0[:-1].astype(np.float64) ** 2)))
    n_scr = int(lib.cdll.gt_clip_grad_norm_scratch_floats(ctypes.byref(cfg)))
    assert n_scr > 1
    scratch = torch.zeros(n_scr, dtype=torch.float32, device=device)
    out = torch.zeros(2, dtype=torch.float32, device=device)
    state = _state(device)

    def run(max_norm, st=state):
        g = torch.from_numpy(g0.copy()).to(device)
        _clip(lib, cfg, g, st, max_norm, out, scratch, device)
        return g.cpu().numpy(), out.cpu().numpy().copy()

    # clipping active
    mn = ref / 4
    g, o = run(mn)
    assert abs(float(o[0]) - ref) <= 1e-6 * ref, (o[0], ref)
    coef = np.float32(mn) / (np.float32(o[0]) + np.float32(1e-6))              # torch's formula, in fp32
    assert o[1] == coef and coef < 1
    want = g0[:-1] * coef
    assert (np.abs(g[:-1] - want) <= np.spacing(np.abs(want))).all()          # g * coef to 1 ulp
    assert g[-1:].view(np.uint32)[0] == g0[-1:].view(np.uint32)[0]            # the guard element: untouched, bitwise
    assert float(scratch.abs().max()) == 0.0                                 # scratch left zero (ticket re-armed, partials cleared)
    g2, o2 = run(mn)                                                          # bitwise reproducible
    assert np.array_equal(o2.view(np.uint32), o.view(np.uint32)) and np.array_equal(g2.view(np.uint32), g.view(np.uint32))
    # max_norm above the norm: nothing changes, coefficient exactly 1
    g, o = run(ref * 4)
    assert np.array_equal(g.view(np.uint32), g0.view(np.uint32)) and o[1] == 1.0
    assert abs(float(o[0]) - ref) <= 1e-6 * ref
    # +inf: measure only
    g, o = run(float("inf"))
    assert np.array_equal(g.view(np.uint32), g0.view(np.uint32)) and o[1] == 1.0
    assert abs(float(o[0]) - ref) <= 1e-6 * ref
    # grad_scale (data-parallel 1/world): the norm of the scaled gradient
    g, o = run(float("inf"), _state(device, 0.25))
    assert abs(float(o[0]) - 0.25 * ref) <= 1e-6 * 0.25 * ref
    assert float(scratch.abs().max()) == 0.0
    # bad arguments
    g = torch.from_numpy(g0.copy()).to(device)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(_lib.GrooveLibError, match="max_norm"):
            lib.call("gt_clip_grad_norm", ctypes.byref(cfg), _ptr(g), _ptr(state), ctypes.c_float(bad), _ptr(out), _ptr(scratch),
                     _stream(device))
    for args in ((None, _ptr(state), _ptr(out), _ptr(scratch)), (_ptr(g), None, _ptr(out), _ptr(scratch)),
                 (_ptr(g), _ptr(state), None, _ptr(scratch)), (_ptr(g), _ptr(state), _ptr(out), None)):
        with pytest.raises(_lib.GrooveLibError, match="NULL"):
            lib.call("gt_clip_grad_norm", ctypes.byref(cfg), args[0], args[1], ctypes.c_float(1.0), args[2], args[3], _stream(device))
    assert np.array_equal(g.cpu().numpy().view(np.uint32), g0.view(np.uint32))


@pytest.mark.parametrize("shape", list(KERNEL_SHAPES))
def test_kernels_against_numpy(shape):
    check_kernels(emu_lib(), "cpu", KERNEL_SHAPES[shape])


# ---- the contract the kernels rely on: after a backward, everything outside the layout's tensors (but the guard element) is zero ----
GAP_CASES = {
    "seq_whole_d32": (cfg_dict(32, 4, 16, 2), 2, True),
    "seq_split_d32_h16": (cfg_dict(32, 16, 512, 2), 2, "split"),
    "split_noride_d128": (cfg_dict(128, 4, 64, 2), 2, "split-noride"),
    "rider_d128": (cfg_dict(128, 4, 64, 3), 2, "split"),
    "op_d48": (cfg_dict(48, 4, 24, 2), 2, False),
    "op_encdec_d32": (cfg_dict(32, 4, 16, 1, 1), 2, False),
}


@pytest.mark.parametrize("case", list(GAP_CASES))
def test_gradient_gaps_are_zero_after_backward(case):
    from oracle import numpy_groove as ng
    cfg, B, seq = GAP_CASES[case]
    cfg = dict(cfg, dropout=0.1)
    r = Runner(cfg, B, "emu", seq=seq)
    r.set_params(ng.init_params(cfg, seed=3, perturb=0.05))
    x, y = ng.synthetic_batch(B, cfg["embedding_size_src"], seed=4)
    r.train_step(x, y, 0.47, skip_update=1)
    g = r.grads.numpy()
    inside = np.zeros(r.total, bool)
    for off, size, _, _ in r.entries:
        inside[off:off + size] = True
    assert np.abs(g[inside]).max() > 0
    gaps = g[:-1][~inside[:-1]]
    assert gaps.size > 0 and np.array_equal(gaps, np.zeros_like(gaps)), (case, np.flatnonzero(g[:-1] * ~inside[:-1])[:8])
    assert g[-1] == 0.0


# ---- StepEngine ---------------------------------------------------------------------------------------------------------------------
ENGINE_DIMS = {"seq_d32": dict(d_model=32, n_heads=4, dim_feedforward=16, num_encoder_layers=2),
               "op_d48": dict(d_model=48, n_heads=4, dim_feedforward=24, num_encoder_layers=2)}


def _defaults(lib):
    for f in ("gt_set_seq_quad", "gt_set_seq_split", "gt_set_seq_ride"):      # (process-global switches other tests may have left)
        getattr(lib.cdll, f)(-1)
    lib.cdll.gt_set_seq(1)


def _engine(dims, B, optimizer="sgd", dropout=0.2, lib=None, device="cpu", **kw):
    from transformergrooveinfilling_amd.engine import StepEngine
    if lib is None:                                 # (the HIP library keeps the switches other tests of the process expect)
        lib = emu_lib()
        _defaults(lib)
    d = dict(dims, num_decoder_layers=dims.get("num_decoder_layers", 0), dropout=dropout, embedding_size_src=16)
    eng = StepEngine(batch_size=B, optimizer=optimizer, learning_rate=0.05, hit_loss_penalty=0.47, seed=3, device=device, lib=lib,
                     **d, **kw)
    eng.load_named(layout.init_params(d, seed=5))
    return eng


def torch_clip_on(eng, max_norm):
    """torch.nn.utils.clip_grad_norm_ over the engine's gradient views (the manual sequence's clip) -> its norm"""
    ps = []
    for g in eng.views(eng.grads).values():
        p = torch.nn.Parameter(torch.empty_like(g))
        p.grad = g                                  # (a view: torch scales the flat buffer in place)
        ps.append(p)
    return float(torch.nn.utils.clip_grad_norm_(ps, max_norm))


def check_engine_against_manual(make, B, max_norm, steps=3, sgd_lr=None, shared_grads=False):
    """make(**kw) -> engine.  Clipped engine vs backward / torch clip / update on a twin, teacher-forced: the twin starts every step from
    the clipped engine's parameters (and Adam moments) -- Adam turns the sign noise of a near-zero gradient element into a whole step of
    lr, which a free-running comparison would carry on.  shared_grads: the twin's update also takes the clipped engine's own gradients
    (read before its clip; the clipped engine then steps through the split sequence) -- on the GPU the weight-gradient atomics leave
    last-bit noise between two backward passes, which Adam's first steps turn into a sizeable part of lr on a near-zero element.
    Returns both engines and the clipped engine's per-step norms."""
    clipped, manual = make(max_grad_norm=max_norm), make()
    x, y = layout.synthetic_batch(B, 16, seed=9)
    x, y = torch.from_numpy(x).to(clipped.device), torch.from_numpy(y).to(clipped.device)
    norms = []
    for step in range(steps):
        before = clipped.params.clone()
        manual.params.copy_(clipped.params)
        if clipped.m is not None:
            manual.m.copy_(clipped.m); manual.v.copy_(clipped.v)
        g = []
        st = clipped.train_step(x, y, on_grads=(lambda: g.append(clipped.grads.clone())) if shared_grads else None).cpu().numpy().copy()
        box = []

        def manual_clip():
            if shared_grads:
                manual.grads.copy_(g[0])
            box.append(torch_clip_on(manual, max_norm))
        manual.train_step(x, y, on_grads=manual_clip)
        assert abs(st[6] - box[0]) <= 1e-6 * box[0], (step, st[6], box[0])
        assert st[7] < 1.0, "clipping must be active on every step"
        assert st[7] == np.float32(max_norm) / (np.float32(st[6]) + np.float32(1e-6))
        assert float((clipped.params - manual.params).abs().max()) <= 1e-6, step
        if sgd_lr is not None:                      # SGD: ||delta theta||_2 <= lr * max_norm
            dn = float(torch.linalg.vector_norm((clipped.params - before).double()))
            assert dn <= sgd_lr * max_norm * (1 + 1e-6), (step, dn)
        norms.append(float(st[6]))
    return clipped, manual, norms


@pytest.mark.parametrize("case", list(ENGINE_DIMS))
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_engine_clipped_step_matches_manual_sequence(case, optimizer):
    B = 4
    make = lambda **kw: _engine(ENGINE_DIMS[case], B, optimizer, **kw)
    probe = make()
    x, y = layout.synthetic_batch(B, 16, seed=9)
    box = []
    probe.train_step(torch.from_numpy(x), torch.from_numpy(y), on_grads=lambda: box.append(torch_clip_on(probe, float("inf"))))
    check_engine_against_manual(make, B, 0.3 * box[0], sgd_lr=0.05 if optimizer == "sgd" else None)


def test_engine_without_clipping_is_bitwise_unchanged():
    B = 4
    a = _engine(ENGINE_DIMS["seq_d32"], B, "adam")
    b = _engine(ENGINE_DIMS["seq_d32"], B, "adam", max_grad_norm=None)
    x, y = layout.synthetic_batch(B, 16, seed=9)
    for _ in range(3):
        sa = a.train_step(torch.from_numpy(x), torch.from_numpy(y)).clone()
        sb = b.train_step(torch.from_numpy(x), torch.from_numpy(y)).clone()
        assert torch.equal(sa, sb) and torch.equal(a.params, b.params) and torch.equal(a.m, b.m)
        assert float(sa[6]) == 0.0 and float(sa[7]) == 0.0


def test_clip_inf_logs_the_norm_and_changes_nothing():
    B = 4
    a = _engine(ENGINE_DIMS["op_d48"], B)
    b = _engine(ENGINE_DIMS["op_d48"], B, max_grad_norm=float("inf"))
    x, y = layout.synthetic_batch(B, 16, seed=9)
    for _ in range(2):
        a.train_step(torch.from_numpy(x), torch.from_numpy(y))
        st = b.train_step(torch.from_numpy(x), torch.from_numpy(y))
        assert float(st[6]) > 0 and float(st[7]) == 1.0
    assert float((a.params - b.params).abs().max()) <= 1e-6


def test_engine_rejects_a_bad_max_norm():
    eng = _engine(ENGINE_DIMS["seq_d32"], 2, max_grad_norm=0.0)
    x, y = layout.synthetic_batch(2, 16, seed=9)
    with pytest.raises(ValueError, match="max_grad_norm"):
        eng.train_step(torch.from_numpy(x), torch.from_numpy(y))


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_clipped_step_keeps_the_exchange_fail_safe(optimizer):
    dims = dict(d_model=128, n_heads=4, dim_feedforward=32, num_encoder_layers=1)
    eng = _engine(dims, 2, optimizer, dropout=0.0, max_grad_norm=1e-3)
    try:
        x, y = layout.synthetic_batch(2, 16, seed=9)
        x, y = torch.from_numpy(x), torch.from_numpy(y)
        s = eng.slot(2)
        assert eng.lib.ws_find(s.cfg, "xchg_err")[0] >= 0
        eng.train_step(x, y)
        before, t0 = eng.params.clone(), eng.state_struct().opt_step
        m0 = None if eng.m is None else eng.m.clone()
        w = eng._xchg_word(s)
        w[0] = 1                                    # the error word, raised by hand in host memory
        eng.train_step(x, y)
        assert torch.equal(eng.params, before) and eng.state_struct().opt_step == t0
        assert float(eng.grads.abs().max()) == 0.0
        if m0 is not None:
            assert torch.equal(eng.m, m0)
    finally:
        eng.lib.cdll.gt_set_seq_quad(-1)


def test_module_api_clip_and_drop_in_function(monkeypatch):
    import transformergrooveinfilling_amd as pkg
    B = 4
    eng = _engine(ENGINE_DIMS["op_d48"], B)
    x, y = layout.synthetic_batch(B, 16, seed=9)
    seen = []
    eng.train_step(torch.from_numpy(x), torch.from_numpy(y), on_grads=lambda: seen.append(eng.grads.clone()))
    eng.grads.copy_(seen[0])                        # (a backward's gradients, as the module API leaves them for the clip)
    params = []
    for (n, p), g in zip(eng.views().items(), eng.views(eng.grads).values()):
        q = torch.nn.Parameter(p)                   # (shares the flat buffer, as the model's Parameters do)
        q.grad = g
        params.append(q)
    ref = [q.grad.clone() for q in params]
    ref_params = []
    for q, g in zip(params, ref):
        r = torch.nn.Parameter(torch.empty_like(g))
        r.grad = g
        ref_params.append(r)
    norm_ref = float(torch.nn.utils.clip_grad_norm_(ref_params, 0.01))
    real = torch.nn.utils.clip_grad_norm_

    def refuse(*a, **k):
        raise AssertionError("the fused path must not call torch's clip_grad_norm_")
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", refuse)
    norm = pkg.clip_grad_norm_(iter(params), 0.01)
    assert norm.dim() == 0 and abs(float(norm) - norm_ref) <= 1e-6 * norm_ref
    for q, r in zip(params, ref_params):
        assert float((q.grad - r.grad).abs().max()) <= 1e-6 * float(r.grad.abs().max() + 1e-30)
    # a subset, norm_type 1, error_if_nonfinite: torch's own function
    calls = []
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    pkg.clip_grad_norm_(params[:-1], 1.0)
    pkg.clip_grad_norm_(params, 1.0, norm_type=1)
    pkg.clip_grad_norm_(params, 1.0, error_if_nonfinite=True)
    assert len(calls) == 3 and calls[1]["norm_type"] == 1


# ---- data parallel over gloo --------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out, case, max_norm):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from harness import emu_lib
    from transformergrooveinfilling_amd import layout, parallel
    from transformergrooveinfilling_amd.engine import StepEngine
    parallel.init_distributed("gloo")
    lib = emu_lib()
    for f in ("gt_set_seq_quad", "gt_set_seq_split", "gt_set_seq_ride"):
        getattr(lib.cdll, f)(-1)
    lib.cdll.gt_set_seq(1)
    dims = dict(ENGINE_DIMS[case], num_decoder_layers=0, dropout=0.0, embedding_size_src=16)
    B = 4
    eng = StepEngine(batch_size=B // world, optimizer="sgd", learning_rate=0.05, hit_loss_penalty=0.47, seed=3 | (rank << 32),
                     device="cpu", world_size=world, lib=lib, max_grad_norm=max_norm, **dims)
    eng.load_named(layout.init_params(dims, seed=5))
    x, y = layout.synthetic_batch(B, 16, seed=9)
    sl = slice(rank * (B // world), (rank + 1) * (B // world))
    norms = []
    for _ in range(2):
        st = eng.train_step(torch.from_numpy(x[sl]), torch.from_numpy(y[sl]))
        norms.append(float(st[6]))
    torch.save({"params": eng.params.clone(), "norms": norms}, out % rank)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", list(ENGINE_DIMS))
def test_data_parallel_clipping_matches_single_process(tmp_path, case):
    B, world = 4, 2
    dims = dict(ENGINE_DIMS[case])
    x, y = layout.synthetic_batch(B, 16, seed=9)
    probe = _engine(dims, B, dropout=0.0, max_grad_norm=float("inf"))
    full = float(probe.train_step(torch.from_numpy(x), torch.from_numpy(y))[6])
    local = _engine(dims, B // world, dropout=0.0, max_grad_norm=float("inf"))
    own = float(local.train_step(torch.from_numpy(x[:B // world]), torch.from_numpy(y[:B // world]))[6])
    assert abs(own - full) > 1e-3 * full                  # (a rank's own gradient has another norm)
    max_norm = 0.3 * full
    out = str(tmp_path / "clip%d.pt")
    run_ranks(_dp_worker, world, out, case, max_norm)
    a, b = torch.load(out % 0), torch.load(out % 1)
    assert torch.equal(a["params"], b["params"])          # replicas bitwise identical
    assert a["norms"] == b["norms"]
    single = _engine(dims, B, dropout=0.0, max_grad_norm=max_norm)
    for i in range(2):
        st = single.train_step(torch.from_numpy(x), torch.from_numpy(y))
        assert abs(a["norms"][i] - float(st[6])) <= 1e-5 * float(st[6]), (i, a["norms"][i], float(st[6]))   # the averaged gradient's norm
        assert float(st[7]) < 1.0
    assert abs(a["norms"][0] - full) <= 1e-5 * full
    assert float((a["params"] - single.params).abs().max()) <= 1e-6


# ---- train.py ---------------------------------------------------------------------------------------------------------------------------
def test_train_cli_and_yaml_key(tmp_path):
    sys.path.insert(0, ROOT)
    import train
    p = train.build_parser()
    assert train.load_hyperparameters(p.parse_args(["--experiment", "X"]))["max_grad_norm"] is None
    assert train.load_hyperparameters(p.parse_args(["--experiment", "X", "--max_grad_norm", "0.5"]))["max_grad_norm"] == 0.5
    assert train.load_hyperparameters(p.parse_args(["--experiment", "X", "--max_grad_norm", "inf"]))["max_grad_norm"] == float("inf")
    cfgs = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "reference_configs", "*.yaml")))
    assert cfgs
    for f in cfgs:                                        # the reference's YAMLs lack the key: no clipping, as there
        assert train.load_hyperparameters(p.parse_args(["--config", f]))["max_grad_norm"] is None, f
    y = tmp_path / "clip.yaml"
    y.write_text(open(cfgs[0]).read() + "\nmax_grad_norm: 1.5\n")
    assert train.load_hyperparameters(p.parse_args(["--config", str(y)]))["max_grad_norm"] == 1.5
