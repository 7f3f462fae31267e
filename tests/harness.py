"""Shared test driver: runs the C ABI (include/groove_hip.h) on either the real HIP library
(torch CUDA buffers) or the host fiber-emulator build of the same sources (numpy buffers), and
exposes results as numpy arrays for comparison with the oracle."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from transformergrooveinfilling_amd import _lib, layout  # noqa: E402

EMU_SO = os.environ.get("GT_EMU_LIB_PATH") or os.path.join(ROOT, "tests", "emu", "libgroove_emu.so")   # override: tile-rule variants
_CSRC = os.path.join(ROOT, "transformergrooveinfilling_amd", "csrc")
# what the emulator library is built from: every source and header of csrc/, the emulator's runtime, both public headers
_SRC = [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f.endswith((".hip", ".h"))] + \
       [os.path.join(ROOT, "tests", "emu", "hip_emu.h")] + [os.path.join(ROOT, "include", h) for h in ("groove_hip.h", "groove_hip_debug.h")]


def emu_lib():
    if (not os.path.exists(EMU_SO)) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in _SRC):
        subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")], stdout=subprocess.DEVNULL)
    return _lib.GrooveLib(EMU_SO)


class NpBuf:
    def __init__(self, arr):
        self.a = np.ascontiguousarray(arr)
        self.ptr = ctypes.c_void_p(self.a.ctypes.data)

    def numpy(self):
        return self.a


class CudaBuf:
    def __init__(self, arr):
        import torch
        self.t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        self.ptr = ctypes.c_void_p(self.t.data_ptr())

    def numpy(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy()


def _signed32(pattern):
    return int(np.uint32(pattern).astype(np.int32))


def _filled(Buf, n, pattern):
    """n floats that all hold the 32-bit pattern, as a Buf (filled on the device for a CudaBuf: a workspace can be hundreds of megabytes)"""
    if hasattr(Buf, "_adopt"):                       # a guarded class: the data between its red zones
        b = Buf.__new__(Buf)
        b._adopt(None, (n,), np.dtype(np.float32))
    elif issubclass(Buf, CudaBuf):
        import torch
        b = Buf.__new__(Buf)
        b.t = torch.empty(n, dtype=torch.float32, device="cuda")
        b.ptr = ctypes.c_void_p(b.t.data_ptr())
    else:
        return Buf(np.full(n, pattern, np.uint32).view(np.float32))
    if issubclass(Buf, CudaBuf):
        import torch
        b.t.view(torch.int32).fill_(_signed32(pattern))
    else:
        b.a.view(np.uint32)[:] = pattern
    return b


def redzone_floats(row_width):
    """floats of ONE red zone of a guarded buffer: 128 rows (the tallest tile the library has) of the buffer's row width, at least 4096,
    rounded up to a multiple of 64 floats -- 256 bytes, so the inner pointer keeps the alignment the allocator gave the whole block"""
    return (max(128 * int(row_width), 4096) + 63) // 64 * 64


def guarded(Buf, pattern, flat_width, registry):
    """Buf (NpBuf / CudaBuf) whose memory is the INSIDE of a larger allocation: a red zone of redzone_floats(row width) floats on each side,
    every word the 32-bit `pattern`.  Row width: the last dimension of a 2-D array, flat_width for anything else (a flat parameter, gradient
    or workspace buffer: the widest row of a tensor inside it).  The upper zone starts at the first byte behind the data.  Every buffer made
    is appended to `registry` as a weak reference; intact() compares both zones bit for bit."""
    import weakref
    on_device = issubclass(Buf, CudaBuf)
    word = np.frombuffer(np.uint32(pattern).tobytes(), np.uint8)

    class Guarded(Buf):
        def __init__(self, arr):
            a = np.ascontiguousarray(arr)
            self._adopt(a, a.shape, a.dtype)

        def _adopt(self, a, shape, dtype):
            n = int(np.prod(shape)) * dtype.itemsize
            assert n % 4 == 0, "a guarded buffer holds whole 32-bit words"
            rz = 4 * redzone_floats(shape[-1] if len(shape) >= 2 else flat_width)
            self._lo, self._n, self._rz = rz, n, rz
            if on_device:
                import torch
                self.full = torch.empty(2 * rz + n, dtype=torch.uint8, device="cuda")
                for z in (self.full[:rz], self.full[rz + n:]):
                    z.view(torch.int32).fill_(_signed32(pattern))
                inner = self.full[rz:rz + n]
                if a is not None:
                    inner.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
                self.t = inner.view({np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32,
                                     np.dtype(np.int64): torch.int64, np.dtype(np.uint32): torch.int32}[dtype]).reshape(shape)
                self.ptr = ctypes.c_void_p(self.t.data_ptr())
            else:
                self.full = np.empty(2 * rz + n, np.uint8)
                self.full[:rz] = np.tile(word, rz // 4)
                self.full[rz + n:] = np.tile(word, rz // 4)
                if a is not None:
                    self.full[rz:rz + n] = a.reshape(-1).view(np.uint8)
                self.a = self.full[rz:rz + n].view(dtype).reshape(shape)
                self.ptr = ctypes.c_void_p(self.a.ctypes.data)
            registry.append(weakref.ref(self))

        def intact(self):
            rz, n = self._rz, self._n
            if on_device:
                import torch
                torch.cuda.synchronize()
                want = _signed32(pattern)
                return bool((self.full[:rz].view(torch.int32) == want).all()) and bool((self.full[rz + n:].view(torch.int32) == want).all())
            want = np.tile(word, rz // 4)
            return np.array_equal(self.full[:rz], want) and np.array_equal(self.full[rz + n:], want)

    Guarded.__name__ = "Guarded" + Buf.__name__
    return Guarded


def cfg_dict(d_model, n_heads, dim_feedforward, num_encoder_layers, num_decoder_layers=0, embedding_size_src=16,
             dropout=0.0, precision=0):
    d = dict(d_model=d_model, n_heads=n_heads, dim_feedforward=dim_feedforward,
             num_encoder_layers=num_encoder_layers, num_decoder_layers=num_decoder_layers,
             embedding_size_src=embedding_size_src, dropout=dropout)
    if precision:
        d["precision"] = precision                 # 1 = bf16 GEMM operands (gt_config.precision)
    return d


class Runner:
    """One model instance behind the C ABI.  backend = 'emu' | 'hip'."""

    def __init__(self, cfg, B, backend="emu", rng=(1234, 99, 0), lr=0.094, seq=True, flags=0, ws_fill=None, guard=None):
        """ws_fill: the 32-bit pattern the workspace holds before gt_workspace_init (None: the float 7.25).  guard: a 32-bit pattern -- every
        buffer this Runner hands to the library (self.Buf, also for buffers a test makes later) then lies between two red zones of that
        pattern (guarded()); redzones_intact() names the buffers whose zones changed.  None: plain allocations."""
        self.cfgd, self.B, self.backend = cfg, B, backend
        self.lib = ledgered(emu_lib() if backend == "emu" else _lib.get_lib())
        self.lib.cdll.gt_set_seq(int(bool(seq)))  # process-global switch: sequence-resident kernels (default where supported)
        # seq = "split" / "whole": force / forbid their two-workgroups-per-sequence mode (d_model 128); True: the library's choice
        self.lib.cdll.gt_set_seq_split(1 if seq in ("split", "split-noride", "split-noquad") else 0 if seq == "whole" else -1)
        # the SPLIT forward with four workgroups per sequence (column partners + pair exchange) is the library's choice wherever
        # 4 x batch workgroups fit the chip; "split-noquad": two workgroups per sequence in the forward too
        self.lib.cdll.gt_set_seq_quad(0 if seq == "split-noquad" else -1)
        # "split": weight gradients as rider workgroups of the backward phases where the library chooses to (idle CUs); "split-noride":
        # the grouped dispatch at the end of backward
        self.lib.cdll.gt_set_seq_ride(0 if seq == "split-noride" else -1)
        self.Buf = NpBuf if backend == "emu" else CudaBuf
        self._guarded = []
        if guard is not None:                        # widest row of a tensor inside a flat buffer: a Linear's weight or an activation
            width = max(3 * cfg["d_model"], cfg["dim_feedforward"], cfg["embedding_size_src"], 27)
            self.Buf = guarded(self.Buf, guard, width, self._guarded)
        self.c = _lib.make_config(B, cfg["embedding_size_src"], cfg["d_model"], cfg["n_heads"], cfg["dim_feedforward"],
                                  cfg["num_encoder_layers"], cfg.get("num_decoder_layers", 0), cfg.get("dropout", 0.0),
                                  cfg.get("precision", 0), flags=flags)      # flags: gt_config.flags (_lib.CFG_NO_QUAD | _lib.CFG_NO_LN_XCHG)
        self.total, self.entries = self.lib.param_layout(self.c)
        self.names = layout.param_names(cfg["d_model"], cfg["dim_feedforward"], cfg["embedding_size_src"],
                                        cfg["num_encoder_layers"], cfg.get("num_decoder_layers", 0))
        assert len(self.names) == len(self.entries)
        for (n, shp), (off, size, rows, cols) in zip(self.names, self.entries):
            assert int(np.prod(shp)) == size and shp[0] == rows, (n, shp, size, rows, cols)
        self.M = B * 32
        if ws_fill is None:
            self.ws = self.Buf(np.full(self.lib.workspace_floats(self.c), 7.25, np.float32))     # (garbage: gt_workspace_init zeroes what must be zero)
        else:
            self.ws = _filled(self.Buf, self.lib.workspace_floats(self.c), ws_fill)
        self.lib.call("gt_workspace_init", ctypes.byref(self.c), self.ws.ptr, ctypes.c_void_p(0))
        self.pe = self.Buf(layout.positional_encoding(cfg["d_model"]))
        self.hvo = self.Buf(np.zeros((self.M, 27), np.float32))
        self.grads = self.Buf(np.zeros(self.total, np.float32))
        self.stats = self.Buf(np.zeros(8, np.float32))
        self.d_hvo = self.Buf(np.zeros((self.M, 27), np.float32))
        self.tgt = self.Buf(np.zeros((self.M, 27), np.float32))
        st = _lib.GtStepState(rng[0], rng[1], rng[2], 0, lr, 1.0, 0.9, 0.999, 1e-8)
        self.state = self.Buf(np.frombuffer(bytes(st), dtype=np.uint8).copy())
        self.stream = ctypes.c_void_p(0)
        self.params = None
        self.d_hvo_from = None                       # whose self.d_hvo is: "loss" (gt_loss wrote it: self.y, self.loss_penalty) or "caller" (backward(d_hvo))

    def redzones_intact(self):
        """names of the live guarded buffers (the attribute that holds one, "buf#<k>" for the k-th made otherwise) whose red zones differ
        from the guard pattern by even one bit; [] without a guard"""
        names = {id(b): k for k, b in vars(self).items() if hasattr(b, "intact")}
        live = [(i, ref()) for i, ref in enumerate(self._guarded)]
        return [names.get(id(b), "buf#%d" % i) for i, b in live if b is not None and not b.intact()]

    # ---- parameters -------------------------------------------------------------------------
    def flatten(self, P):
        flat = np.zeros(self.total, np.float32)
        for (n, shp), (off, size, _, _) in zip(self.names, self.entries):
            flat[off:off + size] = np.asarray(P[n], np.float32).reshape(-1)
        return flat

    def unflatten(self, flat):
        return {n: flat[off:off + size].reshape(shp).copy() for (n, shp), (off, size, _, _) in zip(self.names, self.entries)}

    def set_params(self, P):
        self.params = self.Buf(self.flatten(P))

    # ---- calls ------------------------------------------------------------------------------
    def forward(self, x, tgt_in=None, train=False):
        self.x = self.Buf(np.asarray(x, np.float32).reshape(self.M, -1))
        self.tgt_in = self.Buf(np.asarray(tgt_in, np.float32).reshape(self.M, 27)) if tgt_in is not None else None
        self.lib.call("gt_forward", ctypes.byref(self.c), self.params.ptr, self.pe.ptr, self.x.ptr,
                      self.tgt_in.ptr if self.tgt_in else None, self.hvo.ptr, self.ws.ptr, self.state.ptr, int(train),
                      self.stream)
        return self.hvo.numpy().reshape(self.B, 32, 27).copy()

    def loss(self, y, penalty, want_grad=True):
        self.y = self.Buf(np.asarray(y, np.float32).reshape(self.M, 27))
        self.lib.call("gt_loss", ctypes.byref(self.c), self.hvo.ptr, self.y.ptr, ctypes.c_float(penalty), self.stats.ptr,
                      self.d_hvo.ptr if want_grad else None, self.stream)
        if want_grad:
            self.d_hvo_from, self.loss_penalty = "loss", penalty
        return self.stats.numpy().copy(), self.d_hvo.numpy().reshape(self.B, 32, 27).copy()

    def backward(self, d_hvo=None, train=False, accumulate=0):
        """accumulate: gt_backward's argument -- 1 adds onto what self.grads holds (the nn.Module path), 0 overwrites it"""
        if d_hvo is not None:
            self.d_hvo = self.Buf(np.asarray(d_hvo, np.float32).reshape(self.M, 27))
            self.d_hvo_from = "caller"
        self.lib.call("gt_backward", ctypes.byref(self.c), self.params.ptr, self.grads.ptr, self.x.ptr,
                      self.tgt_in.ptr if self.tgt_in else None, self.hvo.ptr, self.d_hvo.ptr, self.ws.ptr, self.state.ptr,
                      int(train), int(accumulate), self.stream)
        self._grads_dirty = True
        return self.unflatten(self.grads.numpy())

    def optimizer_step(self, algo=0):
        if algo == 1 and not hasattr(self, "m"):
            self.m, self.v = self.Buf(np.zeros(self.total, np.float32)), self.Buf(np.zeros(self.total, np.float32))
        self.lib.call("gt_optimizer_step", algo, self.params.ptr, self.grads.ptr, self.m.ptr if algo == 1 else None,
                      self.v.ptr if algo == 1 else None, ctypes.c_int64(self.total), self.state.ptr, 0, self.stream)
        return self.unflatten(self.params.numpy())

    def train_step(self, x, y, penalty, algo=0, skip_update=False):
        self.x = self.Buf(np.asarray(x, np.float32).reshape(self.M, -1))
        self.y = self.Buf(np.asarray(y, np.float32).reshape(self.M, 27))
        if algo == 1 and not hasattr(self, "m"):
            self.m, self.v = self.Buf(np.zeros(self.total, np.float32)), self.Buf(np.zeros(self.total, np.float32))
        if getattr(self, "_grads_dirty", False):           # gt_train_step precondition: grads are zero on entry
            self.grads = self.Buf(np.zeros(self.total, np.float32))
            self._grads_dirty = False
        self.lib.call("gt_train_step", ctypes.byref(self.c), algo, self.params.ptr, self.grads.ptr,
                      self.m.ptr if algo == 1 else None, self.v.ptr if algo == 1 else None, self.pe.ptr, self.x.ptr, self.y.ptr,
                      ctypes.c_float(penalty), self.hvo.ptr, self.stats.ptr, self.tgt.ptr, self.ws.ptr, self.state.ptr,
                      int(skip_update), self.stream)
        return self.stats.numpy().copy()

    def predict(self, x, thres=0.5, use_thres=True, pd_seed=None):
        self.x = self.Buf(np.asarray(x, np.float32).reshape(self.M, -1))
        if pd_seed is not None:
            self.lib.call("gt_predict_pd", ctypes.byref(self.c), self.params.ptr, self.pe.ptr, self.x.ptr, self.hvo.ptr,
                          ctypes.c_uint32(pd_seed), self.tgt.ptr, self.ws.ptr, self.stream)
            return self.hvo.numpy().reshape(self.B, 32, 27).copy()
        self.lib.call("gt_predict", ctypes.byref(self.c), self.params.ptr, self.pe.ptr, self.x.ptr, self.hvo.ptr,
                      ctypes.c_float(thres), int(use_thres), self.tgt.ptr, self.ws.ptr, self.stream)
        return self.hvo.numpy().reshape(self.B, 32, 27).copy()

    BF16_ONLY = ("ctx", "hact", "dhid", "dqkv", "dzAm", "dzBm")

    def precision_in_force(self):
        """0 / 1 / 2: what gt_config.precision really runs as for this shape (2 needs the level-2 operand shadows and 64- / 128-wide heads)"""
        return int(self.lib.cdll.gt_precision_in_force(ctypes.byref(self.c)))

    def bf16_only(self, name, layer=0):
        """Is this saved tensor stored in bf16 alone (gt_set_operand_shadows level 2: the encoder layers' operand-only tensors;
        precision 2: qkv as well)?"""
        if name == "qkv":
            return layer < self.cfgd["num_encoder_layers"] and self.precision_in_force() == 2
        return (name in self.BF16_ONLY and layer < self.cfgd["num_encoder_layers"]
                and self.lib.cdll.gt_operand_shadow_level(ctypes.byref(self.c)) == 2)

    def ws_get(self, name, layer=0):
        off, cnt = self.lib.ws_find(self.c, name, layer)
        if self.bf16_only(name, layer):           # the live tensor is "<name>16": widened to fp32 (exact)
            o16, _ = self.lib.ws_find(self.c, name + "16", layer)
            u = self.ws.numpy()[o16:o16 + (cnt + 1) // 2].view(np.uint16)[:cnt].astype(np.uint32) << 16
            return u.view(np.float32).copy()
        return self.ws.numpy()[off:off + cnt].copy()

    def step_state(self):
        return _lib.GtStepState.from_buffer_copy(self.state.numpy().tobytes())


def free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def run_ranks(fn, world, *args):
    """mp.start_processes(fn, (world, port) + args) on a free rendezvous port -- once more on a fresh port when the first attempt dies (the
    port is picked, released and re-bound by rank 0: two pytest-xdist workers running multi-rank tests at once can pick the same one)."""
    import torch.multiprocessing as mp
    for attempt in (0, 1):
        try:
            mp.start_processes(fn, args=(world, free_port()) + tuple(args), nprocs=world, join=True, start_method="spawn")
            return
        except Exception:
            if attempt:
                raise


# ---- GT_TRACE_DISPATCH=1 (csrc/gt_common.h; DESIGN.md "Dispatch trace"): "[dispatch] <family> key value ..." on stderr, one line per launch
# (family "wgrad_queue": one per queued weight-gradient problem instead).  GT_TRACE_DISPATCH=2, what trace_dispatch and the ledger ask for:
# the same lines, the seq_fwd / seq_bwd ones with SEQ_INST_KEYS behind the level-1 keys ---------------------------------------------------
TRACE_LEVEL = "2"
# the instantiation kernel<DP, HDC, EXACT, ...> and the branches inside it: head-dim class, d_model equals its class, attention form (mfma /
# mfma-pad / valu), the fused loss rides in this launch
SEQ_INST_KEYS = ("hc", "exact", "attn", "loss")
DISPATCH_KEYS = {
    "kernel": ("grid", "gy", "gz", "block"),
    "gemm_cfg": ("BM", "BN", "BK", "M", "N", "K", "form", "epi", "prec", "splitk", "row", "rowx", "edge"),
    "gemm32": ("BM", "BN", "M", "N", "K", "form", "epi", "prec", "src", "rowx"),
    "gemm32h": ("BM", "BN", "M", "N", "K", "form", "epi", "prec", "src", "rowx"),
    "gemm32row": ("BM", "BN", "M", "N", "K", "form", "epi", "prec", "src", "rowx"),
    "gemm64": ("BM", "BN", "M", "N", "K", "form", "epi", "prec", "src", "rowx"),
    "gemm64h": ("BM", "BN", "M", "N", "K", "form", "epi", "prec", "src", "rowx"),
    "wgrad_queue": ("cls", "M", "N", "K", "k_chunk", "splitk", "prec", "tail"),
    "wgrad_flush": ("cls", "n", "wgs", "prec"),
    "ln_fwd": ("variant", "M", "d", "in16"),
    "ln_bwd": ("variant", "M", "d", "rpw", "in16"),
    "ln_param_reduce": ("jobs", "d"),
    "attn_fwd": ("kernel", "pairs"),
    "attn_bwd": ("kernel", "pairs"),
    "heads": ("M", "d", "prec", "loss"),
    "seq_pack": ("B", "d", "F", "L"),
    "seq_fwd": ("phase", "split", "quad", "ride", "fuse_b0", "B", "d", "F", "L") + SEQ_INST_KEYS,
    "seq_bwd": ("phase", "split", "quad", "ride", "riders", "fuse_b0", "B", "d", "F", "L") + SEQ_INST_KEYS,
    "seq_tail": ("kind", "B", "d", "F", "L"),
    "update": ("kind", "algo", "n"),
}


def parse_dispatch(stderr_text):
    """[(family, {key: int | str})] of the "[dispatch]" lines in a captured stderr (a level-2 trace: TRACE_LEVEL); every line must have exactly
    its family's documented keys."""
    out = []
    for ln in stderr_text.splitlines():
        if not ln.startswith("[dispatch] "):
            continue
        tok = ln.split()[1:]
        fam, kv = tok[0], tok[1:]
        assert fam in DISPATCH_KEYS, ln
        assert len(kv) % 2 == 0 and tuple(kv[0::2]) == DISPATCH_KEYS[fam], ln
        out.append((fam, {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in zip(kv[0::2], kv[1::2])}))
    return out


def trace_dispatch(fn):
    """fn() with GT_TRACE_DISPATCH=2 and file descriptor 2 sent to a temporary file (the library writes the lines with fprintf: below
    sys.stderr) -- works under pytest's capture and in a plain subprocess alike.  Returns (fn's result, parsed [dispatch] lines); whatever
    else arrived on stderr meanwhile is passed on, the trace lines too when fn raises."""
    import tempfile
    sys.stderr.flush()
    saved = os.dup(2)
    old = os.environ.get("GT_TRACE_DISPATCH")
    text, failed = "", True
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["GT_TRACE_DISPATCH"] = TRACE_LEVEL
        try:
            out = fn()
            failed = False
        finally:
            if old is None:
                del os.environ["GT_TRACE_DISPATCH"]
            else:
                os.environ["GT_TRACE_DISPATCH"] = old
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
            tmp.seek(0)
            text = tmp.read().decode(errors="replace")
            rest = "".join(ln + "\n" for ln in text.splitlines() if failed or not ln.startswith("[dispatch] "))
            if rest:
                sys.stderr.write(rest)
    trace = parse_dispatch(text)
    assert trace, "no [dispatch] line: the trace is off"
    ledger_append(trace)
    return out, trace


def dispatched(trace, family, **kv):
    """the trace's lines of `family` (a name or a tuple of names) whose keys have the given values"""
    fams = (family,) if isinstance(family, str) else family
    return [d for f, d in trace if f in fams and all(d.get(k) == v for k, v in kv.items())]


# ---- GT_VARIANT_LEDGER=<file> (tests/variant_ledger.py; DESIGN.md 4a "Variant ledger"): every launch a Runner or trace_dispatch makes is
# appended to <file> as "signature <tab> $PYTEST_CURRENT_TEST".  Unset (the default): Runner.lib is the library itself, nothing is redirected
# and no variable is touched. ------------------------------------------------------------------------------------------------------------
def ledger_append(trace):
    """the distinct signatures of a parsed trace, one short O_APPEND write each (parallel workers may share the file)"""
    path = os.environ.get("GT_VARIANT_LEDGER")
    if not path:
        return
    from variant_ledger import signatures
    test = os.environ.get("PYTEST_CURRENT_TEST", "")
    fd = os.open(path, os.O_WRONLY | os.O_APPEND | os.O_CREAT, 0o644)
    try:
        for sig in sorted(set(signatures(trace))):
            os.write(fd, ("%s\t%s\n" % (sig, test)).encode())
    finally:
        os.close(fd)


def ledger_call(fn):
    """fn() under GT_TRACE_DISPATCH=2 with file descriptor 2 in a temporary file, as trace_dispatch runs it; its launches go to the ledger.
    What arrived on stderr is passed on to file descriptor 2 afterwards -- the [dispatch] lines only where the caller had the trace on
    already (a capfd test, or an enclosing trace_dispatch, reads them there)."""
    import tempfile
    sys.stderr.flush()
    saved = os.dup(2)
    old = os.environ.get("GT_TRACE_DISPATCH")
    text = ""
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        os.environ["GT_TRACE_DISPATCH"] = TRACE_LEVEL
        try:
            return fn()
        finally:
            if old is None:
                del os.environ["GT_TRACE_DISPATCH"]
            else:
                os.environ["GT_TRACE_DISPATCH"] = old
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
            tmp.seek(0)
            text = tmp.read().decode(errors="replace")
            keep = old is not None and old[:1] in ("1", "2")
            rest = "".join(ln + "\n" for ln in text.splitlines() if keep or not ln.startswith("[dispatch] "))
            if rest:
                os.write(2, rest.encode())
            ledger_append(parse_dispatch(text))


class LedgeredLib:
    """GrooveLib with call() -- the one place through which Runner reaches an entry point that launches -- run under ledger_call"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def call(self, name, *args):
        ledger_call(lambda: self._lib.call(name, *args))


def ledgered(lib):
    return LedgeredLib(lib) if os.environ.get("GT_VARIANT_LEDGER") else lib
