"""The optimizer's extras -- SGD momentum / Nesterov / weight decay, Adam's L2 weight decay, AdamW -- as a pass in front of the unchanged
update, without a GPU: gt_optimizer_prepare's kernel against an fp64 restatement of its formulas, StepEngine's steps against torch.optim on
the CPU (teacher-forced), the everything-off step, the exchanges' fail-safe, the data-parallel step over gloo, the optimizer classes and
train.py's configuration.  The kernels run in the host-emulator build of the same sources (tests/emu); tests/test_optimizer_prepare_gpu.py
repeats the kernel and engine cases on the GPU."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest
import torch

from harness import emu_lib, run_ranks
from test_clip_grad_norm import ENGINE_DIMS, KERNEL_SHAPES, _engine, _ptr, _random_grads, _stream, _sync, torch_clip_on
from transformergrooveinfilling_amd import _lib, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LR = 0.05
# name: (algo, weight_decay, momentum, nesterov, decoupled)
VARIANTS = {"momentum": (0, 0.0, 0.9, 0, 0), "nesterov": (0, 0.0, 0.9, 1, 0), "weight_decay": (0, 5e-2, 0.0, 0, 0),
            "all_three": (0, 5e-2, 0.9, 1, 0), "adam_l2": (1, 5e-2, 0.0, 0, 0), "adamw": (1, 5e-2, 0.0, 0, 1)}
# everything gt_optimizer_prepare must refuse before any launch: (algo, weight_decay, momentum, nesterov, decoupled, with mbuf)
REJECTED = [(1, 0.0, 0.9, 0, 0, True), (0, 0.01, 0.0, 0, 1, True), (0, 0.01, 0.0, 1, 0, True), (0, -0.01, 0.0, 0, 0, True),
            (0, 0.0, -0.5, 0, 0, True), (0, 0.0, 0.9, 0, 0, False), (2, 0.01, 0.0, 0, 0, True), (0, float("nan"), 0.0, 0, 0, True)]
UNIT = 2.0 ** -24


def _state(device, grad_scale):
    st = _lib.GtStepState(1, 2, 5, 7, LR, grad_scale, 0.9, 0.999, 1e-8)
    return torch.from_numpy(np.frombuffer(bytes(st), dtype=np.uint8).copy()).to(device)


def _prepare(lib, cfg, algo, p, g, mb, state, hp, device, ws=None):
    lib.call("gt_optimizer_prepare", ctypes.byref(cfg), algo, _ptr(p), _ptr(g), None if mb is None else _ptr(mb),
             None if ws is None else _ptr(ws), _ptr(state), ctypes.byref(_lib.GtOptHparams(*hp)), _stream(device))
    _sync(device)


def restate_fp64(algo, wd, mom, nesterov, decoupled, lr, gs, p, g, b):
    """gt_optimizer_prepare's formulas in fp64 -> (params, grads, mbuf, S): S = per element the sum of the absolute values of the
    terms of each output's formula (the bound's scale)"""
    p, g, b = p.astype(np.float64), g.astype(np.float64), b.astype(np.float64)
    if algo == 1 and decoupled:
        return p * (1.0 - lr * wd), g, b, (np.abs(p) + np.abs(lr * wd * p), np.zeros_like(g), np.zeros_like(b))
    x = g * gs + wd * p
    S = np.abs(g * gs) + np.abs(wd * p)
    Sb = np.zeros_like(b)
    if mom:
        Sb = np.abs(mom * b) + S
        b = mom * b + x
        S = (S + np.abs(mom) * Sb) if nesterov else Sb
        x = x + mom * b if nesterov else b
    return p, x / gs, b, (np.zeros_like(p), S / gs, Sb)


def check_kernel(lib, device, dims, seed=0):
    """gt_optimizer_prepare on one shape's flat buffers (lib: the emulator or the HIP library, device: where the buffers live): every
    variant at grad_scale 1 and 0.25 against the fp64 restatement, within 8 roundings (8 * 2^-24 * S: one per fp32 operation of the
    longest variant); guard elements, gaps, repeatability, the rejected argument combinations and the all-off call"""
    device = torch.device(device)
    d, H, F, L, Ld = dims
    cfg = _lib.make_config(2, 16, d, H, F, L, Ld)
    total, entries = lib.param_layout(cfg)
    g0, p0, b0 = (_random_grads(total, entries, seed + k) for k in range(3))      # (zeros in the gaps)
    p0 *= 10.0
    p0[-1], b0[-1] = np.float32(-3e29), np.float32(7e28)                           # guard elements: never read as data, never written
    inside = np.zeros(total, bool)
    for off, size, _, _ in entries:
        inside[off:off + size] = True
    assert (total - 1) % 4096 != 0                                                 # (the scalar tail runs)
    bits = lambda a: a.view(np.uint32)

    def run(algo, hp, gs):
        p, g, b = (torch.from_numpy(a.copy()).to(device) for a in (p0, g0, b0))
        _prepare(lib, cfg, algo, p, g, b, _state(device, gs), hp, device)
        return p.cpu().numpy(), g.cpu().numpy(), b.cpu().numpy()

    for name, (algo, wd, mom, nest, dec) in VARIANTS.items():
        for gs in (1.0, 0.25):
            got = run(algo, (wd, mom, nest, dec), gs)
            want = restate_fp64(algo, np.float64(np.float32(wd)), np.float64(np.float32(mom)), nest, dec, np.float64(np.float32(LR)), gs,
                                p0[:-1], g0[:-1], b0[:-1])
            for what, a, w, S, a0 in zip("pgb", got, want[:3], want[3], (p0, g0, b0)):
                err = np.abs(a[:-1].astype(np.float64) - w)
                units = float((err / np.maximum(8 * UNIT * S, 1e-300)).max()) if S.any() else 0.0
                print("%s gs=%g %s: %.3f of the bound" % (name, gs, what, units))
                if S.any():
                    assert (err <= 8 * UNIT * S).all(), (name, gs, what, units)
                else:                                                               # a buffer this variant must not write
                    assert np.array_equal(bits(a), bits(a0)), (name, gs, what)
                assert bits(a[-1:])[0] == bits(a0[-1:])[0], (name, gs, what)        # guard element: untouched, bitwise
                assert not a[:-1][~inside[:-1]].any(), (name, gs, what)             # gaps still zero
            again = run(algo, (wd, mom, nest, dec), gs)                             # bitwise reproducible
            assert all(np.array_equal(bits(a), bits(c)) for a, c in zip(got, again)), (name, gs)
    # rejected combinations: a message, and nothing written
    p, g, b = (torch.from_numpy(a.copy()).to(device) for a in (p0, g0, b0))
    st = _state(device, 1.0)
    for algo, wd, mom, nest, dec, with_mbuf in REJECTED:
        with pytest.raises(_lib.GrooveLibError, match="momentum|weight_decay|nesterov|decoupled|algo"):
            _prepare(lib, cfg, algo, p, g, b if with_mbuf else None, st, (wd, mom, nest, dec), device)
    with pytest.raises(_lib.GrooveLibError, match="NULL"):
        lib.call("gt_optimizer_prepare", ctypes.byref(cfg), 0, _ptr(p), None, _ptr(b), None, _ptr(st), ctypes.byref(_lib.GtOptHparams(0.1, 0, 0, 0)),
                 _stream(device))
    # everything off: returns 0 and launches nothing
    _prepare(lib, cfg, 0, p, g, b, st, (0.0, 0.0, 0, 0), device)
    _prepare(lib, cfg, 1, p, g, None, st, (0.0, 0.0, 0, 1), device)
    for t, a0 in ((p, p0), (g, g0), (b, b0)):
        assert np.array_equal(bits(t.cpu().numpy()), bits(a0))


@pytest.mark.parametrize("shape", list(KERNEL_SHAPES))
def test_kernel_against_fp64_restatement(shape):
    check_kernel(emu_lib(), "cpu", KERNEL_SHAPES[shape])


def test_torch_sgd_is_inside_the_same_bound():
    """the reference of the engine tests, torch's own fp32 SGD.step, against the fp64 restatement followed by the plain update: well
    inside the kernel's bound (so the bound is not tighter than fp32 arithmetic allows)"""
    rng = np.random.default_rng(0)
    n = 4096
    p0, g0, b0 = (rng.standard_normal(n).astype(np.float32) * s for s in (1.0, 0.05, 0.05))
    wd, mom = 5e-2, 0.9
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    p.grad = torch.from_numpy(g0.copy())
    opt = torch.optim.SGD([p], lr=LR, momentum=mom, nesterov=True, weight_decay=wd)
    opt.state[p]["momentum_buffer"] = torch.from_numpy(b0.copy())
    opt.step()
    _, g, b, (_, S, _) = restate_fp64(0, wd, mom, 1, 0, LR, 1.0, p0, g0, b0)
    err = np.abs(p.detach().numpy().astype(np.float64) - (p0.astype(np.float64) - LR * g))
    assert (err <= 8 * UNIT * (np.abs(p0) + LR * S)).all()


# ---- StepEngine against torch.optim ---------------------------------------------------------------------------------------------------
# name: (optimizer, engine keywords)
ENGINE_VARIANTS = {"sgd_momentum": ("sgd", dict(momentum=0.9)), "sgd_nesterov_wd": ("sgd", dict(momentum=0.9, nesterov=True, weight_decay=5e-2)),
                   "sgd_wd": ("sgd", dict(weight_decay=5e-2)), "adam_l2": ("adam", dict(weight_decay=5e-2)), "adamw": ("adamw", dict(weight_decay=5e-2))}


def torch_step(eng, optimizer, kw, p0, g_raw, mbuf0, m0, v0, t0, max_norm=None):
    """One step of torch.optim.SGD / Adam / AdamW on the CPU over the engine's tensors: parameters-before, raw gradient (as on_grads sees
    it: before clip and transform; data-parallel sums are averaged by grad_scale), momentum / moment buffers-before.  -> (params, mbuf) flat"""
    gs = eng.state_struct().grad_scale
    flat = lambda t: None if t is None else t.detach().cpu().clone()
    p, g, mb, m, v = flat(p0), flat(g_raw) * gs, flat(mbuf0), flat(m0), flat(v0)
    ps = []
    for (n, pv), gv in zip(eng.views(p).items(), eng.views(g).values()):
        q = torch.nn.Parameter(pv)                  # (views: the optimizer steps the flat copies in place)
        q.grad = gv
        ps.append(q)
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
    if optimizer == "sgd":
        opt = torch.optim.SGD(ps, lr=LR, **kw)
        if mb is not None:
            for q, b in zip(ps, eng.views(mb).values()):
                opt.state[q]["momentum_buffer"] = b
    else:
        opt = (torch.optim.AdamW if optimizer == "adamw" else torch.optim.Adam)(ps, lr=LR, **kw)
        for q, a, b in zip(ps, eng.views(m).values(), eng.views(v).values()):
            opt.state[q] = {"step": torch.tensor(float(t0)), "exp_avg": a, "exp_avg_sq": b}
    opt.step()
    if optimizer == "sgd" and kw.get("momentum"):
        mb = torch.zeros_like(p) if mb is None else mb
        for q, b in zip(ps, eng.views(mb).values()):
            b.copy_(opt.state[q]["momentum_buffer"])            # (torch's first step clones the gradient into a new tensor)
    return p, mb


def check_engine_against_torch(eng, optimizer, kw, x, y, steps=3, max_norm=None, tol=1e-6, twin=None):
    """Teacher-forced: every step torch.optim starts from the engine's own parameters, buffers and raw gradient (read through on_grads),
    and the engine's parameters and momentum buffer after the step must agree with torch's to `tol` absolute.  Three steps: the buffer
    from zero, then carried.  twin: a second engine that starts every step from the first one's state and takes it WITHOUT on_grads (the
    fused branch: the captured graph where graphs are on); with SGD it must land on the same parameters and buffer to `tol` (Adam turns
    the last-bit noise between two backward passes of the GPU into a sizeable part of lr on a near-zero element: finite is all that is
    asked of it there)."""
    for step in range(steps):
        p0 = eng.params.clone()
        mb0 = None if eng.mbuf is None else eng.mbuf.clone()
        m0, v0 = (None, None) if eng.m is None else (eng.m.clone(), eng.v.clone())
        t0 = eng.state_struct().opt_step
        if twin is not None:
            twin.params.copy_(p0); twin.state.copy_(eng.state)
            twin._opt_extras()                      # (allocates its momentum buffer)
            for name, t in (("mbuf", mb0), ("m", m0), ("v", v0)):
                if t is not None:
                    getattr(twin, name).copy_(t)
                elif name == "mbuf" and twin.mbuf is not None:
                    twin.mbuf.zero_()
        g = []
        eng.train_step(x, y, on_grads=lambda: g.append(eng.grads.clone()))
        assert float(g[0].abs().max()) > 0
        want_p, want_mb = torch_step(eng, optimizer, kw, p0, g[0], mb0, m0, v0, t0, max_norm)
        dp = float((eng.params.cpu() - want_p).abs().max())
        print("step %d: |params - torch| max %.3g" % (step, dp))
        assert dp <= tol, (step, dp)
        if kw.get("momentum"):
            db = float((eng.mbuf.cpu() - want_mb).abs().max())
            print("step %d: |mbuf - torch| max %.3g" % (step, db))
            assert db <= tol, (step, db)
            assert step == 0 or float(mb0.abs().max()) > 0          # (steps 2 and 3 carry a buffer)
        else:
            assert eng.mbuf is None
        assert eng.state_struct().opt_step == t0 + 1
        if twin is not None:
            twin.train_step(x, y)
            assert torch.isfinite(twin.params).all() and twin.state_struct().opt_step == t0 + 1
            if optimizer == "sgd":
                dt = float((twin.params - eng.params).abs().max())
                print("step %d: |twin - engine| max %.3g" % (step, dt))
                assert dt <= tol, (step, dt)
                if kw.get("momentum"):
                    assert float((twin.mbuf - eng.mbuf).abs().max()) <= tol, step
    assert float((eng.params - p0).abs().max()) > 0


def _batch(B, device="cpu"):
    x, y = layout.synthetic_batch(B, 16, seed=9)
    return torch.from_numpy(x).to(device), torch.from_numpy(y).to(device)


@pytest.mark.parametrize("variant", list(ENGINE_VARIANTS))
@pytest.mark.parametrize("case", list(ENGINE_DIMS))
def test_engine_step_matches_torch_optim(case, variant):
    optimizer, kw = ENGINE_VARIANTS[variant]
    eng, twin = (_engine(ENGINE_DIMS[case], 4, optimizer, **kw) for _ in range(2))
    check_engine_against_torch(eng, optimizer, kw, *_batch(4), twin=twin)


@pytest.mark.parametrize("variant", ["sgd_nesterov_wd", "adamw"])
def test_engine_clips_first_then_transforms(variant):
    optimizer, kw = ENGINE_VARIANTS[variant]
    probe = _engine(ENGINE_DIMS["seq_d32"], 4, optimizer)
    x, y = _batch(4)
    box = []
    probe.train_step(x, y, on_grads=lambda: box.append(torch_clip_on(probe, float("inf"))))
    eng = _engine(ENGINE_DIMS["seq_d32"], 4, optimizer, max_grad_norm=0.3 * box[0], **kw)
    check_engine_against_torch(eng, optimizer, kw, x, y, max_norm=0.3 * box[0])


def test_fused_branches_take_the_split_sequence_with_extras():
    """without on_grads (the fused branches of train_step / train_step_indexed) the same parameters as the watched step, bit for bit"""
    kw = dict(momentum=0.9, nesterov=True, weight_decay=5e-2)
    a, b, c = (_engine(ENGINE_DIMS["seq_d32"], 4, "sgd", **kw) for _ in range(3))
    x, y = _batch(4)
    xs, ys = torch.cat([x, x]), torch.cat([y, y])
    for _ in range(2):
        a.train_step(x, y, on_grads=lambda: None)
        b.train_step(x, y)
        c.train_step_indexed(xs, ys, torch.arange(4, 8))
    assert torch.equal(a.params, b.params) and torch.equal(a.mbuf, b.mbuf) and float(b.mbuf.abs().max()) > 0
    assert torch.equal(a.params, c.params) and torch.equal(a.mbuf, c.mbuf)
    assert float(b.grads.abs().max()) == 0.0


def test_engine_with_everything_off_is_bitwise_unchanged():
    for optimizer in ("sgd", "adam"):
        a = _engine(ENGINE_DIMS["seq_d32"], 4, optimizer)
        b = _engine(ENGINE_DIMS["seq_d32"], 4, optimizer, weight_decay=0.0, momentum=0.0, nesterov=False)
        x, y = _batch(4)
        for _ in range(3):
            sa, sb = a.train_step(x, y).clone(), b.train_step(x, y).clone()
            assert torch.equal(sa, sb) and torch.equal(a.params, b.params)
        assert b.mbuf is None and b._opt_extras() is None
        assert b._split_recipe(b.slot(4), "fused") is None          # the fused step, under its old graph key


@pytest.mark.parametrize("kw", [dict(optimizer="adam", momentum=0.9), dict(optimizer="sgd", nesterov=True), dict(optimizer="sgd", weight_decay=-1.0),
                                dict(optimizer="sgd", momentum=-0.1)])
def test_engine_rejects_bad_combinations_before_any_launch(kw):
    kw = dict(kw)
    eng = _engine(ENGINE_DIMS["seq_d32"], 2, kw.pop("optimizer"), **kw)
    x, y = _batch(2)
    before = eng.state.clone()
    with pytest.raises(ValueError, match="momentum|nesterov|weight_decay"):
        eng.train_step(x, y)
    assert torch.equal(eng.state, before) and float(eng.grads.abs().max()) == 0.0


@pytest.mark.parametrize("optimizer,kw", [("sgd", dict(momentum=0.9, weight_decay=5e-2)), ("adamw", dict(weight_decay=5e-2))])
def test_extras_keep_the_exchange_fail_safe(optimizer, kw):
    dims = dict(d_model=128, n_heads=4, dim_feedforward=32, num_encoder_layers=1)
    eng = _engine(dims, 2, optimizer, dropout=0.0, **kw)
    try:
        x, y = _batch(2)
        s = eng.slot(2)
        assert eng.lib.ws_find(s.cfg, "xchg_err")[0] >= 0
        eng.train_step(x, y)
        keep = {k: getattr(eng, k).clone() for k in ("params", "mbuf", "m", "v") if getattr(eng, k) is not None}
        assert ("mbuf" in keep) == (optimizer == "sgd") and ("m" in keep) == (optimizer == "adamw")
        t0 = eng.state_struct().opt_step
        eng._xchg_word(s)[0] = 1                    # the error word, raised by hand in host memory
        eng.train_step(x, y)
        for k, t in keep.items():
            assert torch.equal(getattr(eng, k), t), k
        assert eng.state_struct().opt_step == t0 and float(eng.grads.abs().max()) == 0.0
    finally:
        eng.lib.cdll.gt_set_seq_quad(-1)


# ---- data parallel over gloo --------------------------------------------------------------------------------------------------------
DP_KW = dict(momentum=0.9, weight_decay=5e-2)


def _dp_worker(rank, world, port, out, case):
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
    eng = StepEngine(batch_size=B // world, optimizer="sgd", learning_rate=LR, hit_loss_penalty=0.47, seed=3 | (rank << 32),
                     device="cpu", world_size=world, lib=lib, **DP_KW, **dims)
    eng.load_named(layout.init_params(dims, seed=5))
    x, y = layout.synthetic_batch(B, 16, seed=9)
    sl = slice(rank * (B // world), (rank + 1) * (B // world))
    for _ in range(2):
        eng.train_step(torch.from_numpy(x[sl]), torch.from_numpy(y[sl]))
    torch.save({"params": eng.params.clone(), "mbuf": eng.mbuf.clone()}, out % rank)
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_extras_match_single_process(tmp_path):
    case, B, world = "seq_d32", 4, 2
    out = str(tmp_path / "prep%d.pt")
    run_ranks(_dp_worker, world, out, case)
    a, b = torch.load(out % 0), torch.load(out % 1)
    assert torch.equal(a["params"], b["params"]) and torch.equal(a["mbuf"], b["mbuf"])          # replicas bitwise identical
    single = _engine(ENGINE_DIMS[case], B, "sgd", dropout=0.0, **DP_KW)
    x, y = _batch(B)
    for _ in range(2):
        single.train_step(x, y)
    assert float((a["params"] - single.params).abs().max()) <= 1e-6
    assert float((a["mbuf"] - single.mbuf).abs().max()) <= 1e-6 and float(single.mbuf.abs().max()) > 0


# ---- the optimizer classes (host side: the engine lives in the emulator) -------------------------------------------------------------
def _optimizer(cls_name, dims=None, **kw):
    from transformergrooveinfilling_amd import training
    eng = _engine(dims or ENGINE_DIMS["seq_d32"], 4, "sgd")
    params = [torch.nn.Parameter(v) for v in eng.views().values()]              # (share the flat buffer, as the model's Parameters do)
    return eng, params, getattr(training, cls_name)(params, LR, eng, **kw)


def _grads_of_a_backward(eng):
    x, y = _batch(4)
    seen = []
    eng.train_step(x, y, on_grads=lambda: seen.append(eng.grads.clone()))
    return seen[0]


def test_sgd_state_dict_round_trip_and_none_buffers():
    eng, _, opt = _optimizer("GrooveSGD", momentum=0.9, weight_decay=5e-2)
    views = list(eng.views(eng.mbuf).values())
    assert all(opt.state[p]["momentum_buffer"].data_ptr() == v.data_ptr() for p, v in zip(opt.param_groups[0]["params"], views))
    _grads_of_a_backward(eng)                       # (a momentum step: the buffers are no longer zero)
    assert float(eng.mbuf.abs().max()) > 0
    sd = opt.state_dict()
    assert sd["param_groups"][0]["momentum"] == 0.9 and sd["param_groups"][0]["weight_decay"] == 5e-2
    assert all(torch.equal(sd["state"][i]["momentum_buffer"], v) for i, v in enumerate(views))
    eng2, _, opt2 = _optimizer("GrooveSGD", momentum=0.9)
    opt2.load_state_dict({"state": {k: {"momentum_buffer": v["momentum_buffer"].clone()} for k, v in sd["state"].items()},
                          "param_groups": sd["param_groups"]})
    assert torch.equal(eng2.mbuf, eng.mbuf)          # the buffers land in the engine's flat buffer
    # a checkpoint without buffers (a momentum-free run, the reference's): a momentum run resumes from zeros
    _, _, plain = _optimizer("GrooveSGD")
    psd = plain.state_dict()
    assert psd["state"][0] == {"momentum_buffer": None} and psd["param_groups"][0]["momentum"] == 0
    opt2.load_state_dict(psd)
    assert float(eng2.mbuf.abs().max()) == 0.0 and eng2.momentum == 0.9
    assert opt2.state[opt2.param_groups[0]["params"][0]]["momentum_buffer"] is not None


def test_param_groups_edits_take_effect_between_steps():
    eng, params, opt = _optimizer("GrooveSGD")
    g = _grads_of_a_backward(eng)                   # (also one plain step)
    assert eng.mbuf is None and opt.state[params[0]]["momentum_buffer"] is None
    for step, (mom, wd) in enumerate([(0.0, 0.0), (0.9, 0.0), (0.5, 5e-2)]):
        opt.param_groups[0]["momentum"], opt.param_groups[0]["weight_decay"] = mom, wd
        eng.grads.copy_(g)
        p0, mb0 = eng.params.clone(), None if eng.mbuf is None else eng.mbuf.clone()
        opt.step()
        want_p, want_mb = torch_step(eng, "sgd", dict(momentum=mom, weight_decay=wd), p0, g, mb0, None, None, 0)
        assert float((eng.params - want_p).abs().max()) <= 1e-6, step
        if mom:
            assert float((eng.mbuf - want_mb).abs().max()) <= 1e-6, step
            assert opt.state[params[0]]["momentum_buffer"].data_ptr() == next(iter(eng.views(eng.mbuf).values())).data_ptr()
            # the one deviation from torch: .grad keeps the transformed gradient (here the momentum step) until zero_grad()
            assert float((eng.grads - eng.mbuf).abs().max()) <= 1e-6
            assert (step == 1) == torch.equal(eng.grads, g)         # (a first momentum step's buffer is the gradient itself)
    opt.zero_grad()
    assert float(eng.grads.abs().max()) == 0.0


def test_adamw_class_and_unsupported_arguments():
    from transformergrooveinfilling_amd import training
    eng, params, opt = _optimizer("GrooveAdamW")
    assert isinstance(opt, torch.optim.AdamW) and opt.param_groups[0]["weight_decay"] == 1e-2          # torch's default
    assert eng.algo == 1 and eng.decoupled and eng.weight_decay == 1e-2 and eng._opt_extras() == (1e-2, 0.0, False, True)
    g = _grads_of_a_backward(eng)
    eng.grads.copy_(g)
    p0, m0, v0, t0 = eng.params.clone(), eng.m.clone(), eng.v.clone(), eng.state_struct().opt_step
    opt.step()
    want_p, _ = torch_step(eng, "adamw", dict(weight_decay=1e-2), p0, g, None, m0, v0, t0)
    assert float((eng.params - want_p).abs().max()) <= 1e-6
    assert torch.equal(eng.grads, g)                # AdamW leaves the gradients alone
    eng2, _, adam = _optimizer("GrooveAdam", weight_decay=5e-2)
    assert not eng2.decoupled and eng2._opt_extras() == (5e-2, 0.0, False, False)
    for cls, kw in (("GrooveSGD", dict(dampening=0.1)), ("GrooveSGD", dict(maximize=True)), ("GrooveAdam", dict(amsgrad=True)),
                    ("GrooveAdamW", dict(amsgrad=True)), ("GrooveAdam", dict(maximize=True))):
        with pytest.raises(ValueError, match="not supported"):
            _optimizer(cls, **kw)
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        opt.step()
    with pytest.raises(ValueError, match="nesterov|Nesterov"):
        _optimizer("GrooveSGD", nesterov=True)
    assert training.GrooveAdamW.__mro__.index(training._FusedMixin) < training.GrooveAdamW.__mro__.index(torch.optim.AdamW)


# ---- train.py ---------------------------------------------------------------------------------------------------------------------------
def test_train_cli_flags_and_yaml_keys(tmp_path):
    sys.path.insert(0, ROOT)
    import train
    p = train.build_parser()
    off = {"momentum": 0.0, "nesterov": False, "weight_decay": None}
    pick = lambda hp: {k: hp[k] for k in off}
    assert pick(train.load_hyperparameters(p.parse_args(["--experiment", "X"]))) == off
    hp = train.load_hyperparameters(p.parse_args(["--experiment", "X", "--momentum", "0.9", "--nesterov", "--weight_decay", "5e-4",
                                                  "--optimizer_algorithm", "adamw"]))
    assert pick(hp) == {"momentum": 0.9, "nesterov": True, "weight_decay": 5e-4} and hp["optimizer_algorithm"] == "adamw"
    tp = train.model_params(hp, "cuda:0")["training"]
    assert (tp["momentum"], tp["nesterov"], tp["weight_decay"]) == (0.9, True, 5e-4)
    cfgs = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "reference_configs", "*.yaml")))
    assert cfgs
    for f in cfgs:                                        # the reference's YAMLs lack the keys: plain SGD / Adam, as there
        hp = train.load_hyperparameters(p.parse_args(["--config", f]))
        assert pick(hp) == off, f
        tp = train.model_params(hp, "cuda:0")["training"]
        assert set(tp) == {"learning_rate", "batch_size", "hit_loss_penalty"}, f
    y = tmp_path / "extras.yaml"
    y.write_text(open(cfgs[0]).read() + "\nmomentum: 0.8\nnesterov: true\nweight_decay: 0.001\n")
    assert pick(train.load_hyperparameters(p.parse_args(["--config", str(y)]))) == {"momentum": 0.8, "nesterov": True, "weight_decay": 0.001}
