"""C-ABI checks that need no GPU: the HIP library loads, exports every symbol include/groove_hip.h
declares, validates configs like the reference's torch modules do, and lays parameters out in the
checkpoint's state-dict order."""
import ctypes
import os
import re

import numpy as np
import pytest

from transformergrooveinfilling_amd import _lib, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.DEFAULT_LIB):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.GrooveLib()


def test_exports_every_declared_symbol(lib):
    public, debug = (open(os.path.join(ROOT, "include", h)).read() for h in ("groove_hip.h", "groove_hip_debug.h"))
    declared = set(re.findall(r"\b(gt_[a-z_]+)\s*\(", public + debug))
    assert declared == set(_lib.EXPORTS)
    # the contract declares no process-wide switch and no test aid: those live in the debug header
    assert re.findall(r"\b(gt_(?:set|debug)_[a-z_]+)\s*\(", public) == []
    for name in declared:
        assert hasattr(lib.cdll, name), name
    assert lib.cdll.gt_version() >= 1


def test_struct_sizes_match_header():
    assert ctypes.sizeof(_lib.GtConfig) == 40          # 8 x int32/float + precision + flags
    assert ctypes.sizeof(_lib.GtStepState) == 48
    assert [f[0] for f in _lib.GtConfig._fields_] == ["batch", "src_dim", "d_model", "n_heads", "dim_ff", "n_enc_layers",
                                                      "n_dec_layers", "dropout", "precision", "flags"]
    hdr = open(os.path.join(ROOT, "include", "groove_hip.h")).read()
    body = hdr[hdr.index("typedef struct gt_config {"):hdr.index("} gt_config;")]
    assert re.findall(r"^\s*(?:int32_t|float)\s+(\w+);", body, re.M) == [f[0] for f in _lib.GtConfig._fields_]
    assert int(re.search(r"#define GT_CFG_NO_QUAD (\d+)", hdr).group(1)) == _lib.CFG_NO_QUAD
    assert int(re.search(r"#define GT_CFG_NO_LN_XCHG (\d+)", hdr).group(1)) == _lib.CFG_NO_LN_XCHG


def test_config_validation(lib):
    bad = [_lib.make_config(2, 16, 30, 4, 16, 2),      # embed_dim % heads (torch:nn/functional.py:6415-6417)
           _lib.make_config(0, 16, 32, 4, 16, 2), _lib.make_config(2, 16, 1024, 4, 16, 2),
           _lib.make_config(2, 16, 32, 4, 16, 0), _lib.make_config(2, 16, 32, 4, 16, 2, 0, 1.0)]
    unknown_precision = _lib.make_config(2, 16, 32, 4, 16, 2)
    unknown_precision.precision = 7
    bad.append(unknown_precision)
    bad.append(_lib.make_config(2, 16, 32, 4, 16, 2, flags=64))
    for c in bad:
        with pytest.raises(_lib.GrooveLibError):
            lib.param_layout(c)
    assert b"divisible" in lib.cdll.gt_last_error() or True


@pytest.mark.parametrize("shape", [(32, 16, 16, 6, 0), (128, 512, 16, 3, 0), (512, 512, 27, 6, 0), (256, 512, 16, 6, 6)])
def test_param_layout_is_state_dict_order(lib, shape):
    d, F, S, L, Ld = shape
    c = _lib.make_config(4, S, d, 4, F, L, Ld)
    total, entries = lib.param_layout(c)
    names = layout.param_names(d, F, S, L, Ld)
    assert len(names) == len(entries)
    end = 0
    for (n, shp), (off, size, rows, cols) in zip(names, entries):
        assert off >= end and off % 64 == 0, n
        assert size == int(np.prod(shp)) and rows == shp[0] and cols == (shp[1] if len(shp) == 2 else 0), n
        end = off + size
    assert total >= end
    assert sum(e[1] for e in entries) == {(32, 16, 16, 6, 0): 34043, (128, 512, 16, 3, 0): 600731,
                                          (512, 512, 27, 6, 0): 9497115, (256, 512, 16, 6, 6): 7926811}[shape]  # BASELINE.md param counts


def test_demo_checkpoint_names_match_layout():
    z = np.load(os.path.join(ROOT, "tests", "golden", "demo_ckpt.npz"))
    keys = [k[3:] for k in z.files if k.startswith("sd/") and not k.endswith(".pe")]
    assert keys == [n for n, _ in layout.param_names(32, 16, 16, 6, 0)]
    assert np.abs(z["sd/InputLayerEncoder.PositionalEncoding.pe"][0] - layout.positional_encoding(32)).max() < 1e-6


def test_workspace_lookup(lib):
    c = _lib.make_config(3, 16, 64, 2, 32, 2, 2)
    n = lib.workspace_floats(c)
    seen = []
    for name, layer in [("x0", 0), ("qkv", 0), ("P", 1), ("hact", 3), ("kvx", 2), ("memory", 0), ("dlogits", 0)]:
        off, cnt = lib.ws_find(c, name, layer)
        assert 0 <= off and off + cnt <= n
        seen.append((off, off + cnt))
    seen.sort()
    assert all(a[1] <= b[0] for a, b in zip(seen, seen[1:]))
    with pytest.raises(_lib.GrooveLibError):
        lib.ws_find(c, "kvx", 0)          # encoder layers have no cross-attention buffers
    with pytest.raises(_lib.GrooveLibError):
        lib.ws_find(c, "nope", 0)
    try:
        for level, cfg, answers in [
                (2, _lib.make_config(3, 16, 128, 4, 512, 2), "seq_xchg"),                      # pair-exchange region
                (2, _lib.make_config(2, 16, 32, 16, 64, 2), "amask"),
                (2, c, "dmem"),                                                                # decoder regions
                (1, _lib.make_config(128, 16, 256, 4, 512, 2, precision=1), "hact16"),         # operand shadows beside the fp32 tensors
                (2, _lib.make_config(128, 16, 256, 4, 512, 2, precision=1), "hact16"),         # ... and the bf16-only tensors
                (2, _lib.make_config(128, 16, 512, 8, 512, 2, precision=2), "qkv16")]:         # in-place qkv16 / dctx16
            lib.cdll.gt_set_operand_shadows(level)
            lib.ws_find(cfg, answers, 0)
            _check_workspace_table(lib, cfg)
            lib.cdll.gt_set_operand_shadows(0)
            with pytest.raises(_lib.GrooveLibError):
                lib.ws_find(cfg, "ctx16", 0)
    finally:
        lib.cdll.gt_set_operand_shadows(-1)


WS_ONCE = "x0 a0 enc_xhat enc_rstd memory y0 b0 dec_final dlogits dmem dctx seq_xchg rowx amask pack_f pack_b".split()
WS_PER_LAYER = ("qkv P ctx xhat1 rstd1 x1 qx kvx Px ctxx xhatx rstdx x2 hact xhat2 rstd2 xout "
                "dzA dzAm dzB dzBm dzC dzCm dhid dqkv dqkvx").split()


def _check_workspace_table(lib, cfg):
    """every answer of gt_ws_find for one configuration: inside the workspace, aligned, and overlapping only where the layout says so"""
    total = lib.workspace_floats(cfg)
    nl = cfg.n_enc_layers + cfg.n_dec_layers
    p2 = lib.cdll.gt_precision_in_force(ctypes.byref(cfg)) == 2

    def find(name, layer):
        try:
            return lib.ws_find(cfg, name, layer)
        except _lib.GrooveLibError:
            return None

    keys = [(n, 0) for n in WS_ONCE] + [(n, l) for n in WS_PER_LAYER for l in range(nl)]
    fp32 = {k: find(*k) for k in keys}
    fp32 = {k: v for k, v in fp32.items() if v is not None}
    assert {"x0", "qkv", "hact", "dlogits", "dzA", "dqkv"} <= {k[0] for k in fp32}
    for k, (off, cnt) in fp32.items():
        assert 0 <= off and cnt > 0 and off + cnt <= total and off % 64 == 0, k
    spans = sorted((off, off + cnt, k) for k, (off, cnt) in fp32.items())
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0], (a, b)
    err = find("xchg_err", 0)
    xchg = [fp32[(n, 0)] for n in ("seq_xchg", "rowx") if (n, 0) in fp32]
    assert len(xchg) <= 1 and (err is None) == (not xchg)
    if err:
        assert err == (xchg[0][0], 2) and xchg[0][1] >= 2
    n16 = 0
    for k, (off, cnt) in fp32.items():
        s = find(k[0] + "16", k[1])
        if s is None:
            continue
        n16 += 1
        assert s[1] == (cnt + 1) // 2 and 0 <= s[0] and s[0] + s[1] <= total, k
        if p2 and k[0] in ("qkv", "dctx"):
            assert s[0] == off, k                      # precision 2: the bf16 tensor lies at the head of its fp32 region
        else:
            assert all(s[0] + s[1] <= a or b <= s[0] for a, b, _ in spans), k
    shadows = lib.cdll.gt_operand_shadow_level(ctypes.byref(cfg)) > 0
    for l in range(nl):
        for a, b in (("dzA16", "dzAm16"), ("dzB16", "dzBm16")):
            assert find(a, l) == find(b, l)
            assert (find(a, l) is not None) == (shadows and l < cfg.n_enc_layers), (a, l)
    assert (n16 > 0) == shadows and (find("ctx16", 0) is not None) == shadows and (find("dzA16", 0) is not None) == shadows
    assert (find("qkv16", 0) is not None) == p2 and (find("dctx16", 0) is not None) == p2
    assert find("kvx", 0) is None and find("nope", 0) is None
    if cfg.n_dec_layers == 0:
        assert find("y0", 0) is None
    else:
        assert find("y0", 0) is not None and find("kvx", cfg.n_enc_layers) is not None


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(_lib.GrooveLibError, match="no CPU fallback"):
        _lib.GrooveLib(str(tmp_path / "libgroove_hip.so"))


def test_too_many_layernorm_instances_are_rejected_up_front():
    """a config whose LayerNorm count exceeds the backward's partials table must fail in the config check (before any
    launch), not after forward and loss have run"""
    import ctypes
    from harness import emu_lib
    from transformergrooveinfilling_amd import _lib
    lib = emu_lib()
    ok = _lib.make_config(1, 16, 32, 4, 16, 47)
    assert lib.cdll.gt_workspace_bytes(ctypes.byref(ok)) > 0
    bad = _lib.make_config(1, 16, 32, 4, 16, 48)
    assert lib.cdll.gt_workspace_bytes(ctypes.byref(bad)) == 0
    assert b"LayerNorm" in lib.cdll.gt_last_error()
    bad2 = _lib.make_config(1, 16, 32, 4, 16, 20, 20)
    assert lib.cdll.gt_workspace_bytes(ctypes.byref(bad2)) == 0
