// libgroove_hip.so -- C ABI (include/groove_hip.h) over the gfx950 kernels of the GrooveTransformer
// train / predict step.  Host side here only sequences launches on the caller's stream: no
// allocation, no synchronisation, no host reads of device data -> every entry point is
// hipGraph-capturable.
//
// Op order follows the third-party torch modules the reference's un-vendored submodule wires
// (SURVEY.md 3.2-3.4): encoder layer torch:nn/modules/transformer.py:951-956,961-982; decoder layer
// :1143-1153; MHA torch:nn/functional.py:5820-5850,6504-6642; module tree / parameter names from the
// reference's demo checkpoint (ref:demo/transformer_run_171tyqit_Epoch_1.Model).
#include <assert.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "gt_attn.h"
#include "gt_common.h"
#include "gt_curve.h"
#include "gt_gemm.h"
#include "gt_groove.h"
#include "gt_group.h"
#include "gt_misc.h"
#include "gt_seq_api.h"

// ------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
static int gt_fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return -1;
}
extern "C" const char* gt_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------ launch timing
GtProfile g_prof;
thread_local bool g_dispatch_named = false;     // GT_TRACE_DISPATCH (gt_common.h)
#ifndef GT_EMU
struct ProfRec { const char* label; double flops, bytes; hipEvent_t a, b; };
static std::vector<ProfRec> g_recs;
void gt_prof_events(hipEvent_t* start, hipEvent_t* stop) {
  ProfRec r{g_prof.label, g_prof.flops, g_prof.bytes, nullptr, nullptr};
  (void)hipEventCreate(&r.a);
  (void)hipEventCreate(&r.b);
  g_recs.push_back(r);
  *start = r.a; *stop = r.b;
  g_prof.label = "other"; g_prof.flops = 0; g_prof.bytes = 0;
}
#else
void gt_prof_events(hipEvent_t*, hipEvent_t*) {}
#endif
extern "C" int gt_profile_enable(int on) {
  g_prof.on = on != 0;
  g_prof.label = "other";
  return 0;
}
// Synchronises, then writes up to max_rows rows "label count total_ms total_flops total_bytes" (one per
// kernel class, '\n'-separated) into buf and clears the records.  Returns the number of classes.
extern "C" int gt_profile_report(char* buf, size_t buf_len, int max_rows) {
  int n = 0;
#ifndef GT_EMU
  struct Acc { std::string label; long count; double ms, flops, bytes; };
  std::vector<Acc> acc;
  for (auto& r : g_recs) {
    (void)hipEventSynchronize(r.b);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
    size_t i = 0;
    for (; i < acc.size(); ++i) if (acc[i].label == r.label) break;
    if (i == acc.size()) acc.push_back(Acc{r.label, 0, 0, 0, 0});
    acc[i].count++; acc[i].ms += ms; acc[i].flops += r.flops; acc[i].bytes += r.bytes;
  }
  g_recs.clear();
  std::string out;
  for (auto& a : acc) {
    if (n >= max_rows) break;
    char line[256];
    snprintf(line, sizeof(line), "%s %ld %.6f %.6e %.6e\n", a.label.c_str(), a.count, a.ms, a.flops, a.bytes);
    out += line;
    ++n;
  }
  if (buf && buf_len) { strncpy(buf, out.c_str(), buf_len - 1); buf[buf_len - 1] = 0; }
#else
  if (buf && buf_len) buf[0] = 0;
#endif
  return n;
}
extern "C" int gt_version(void) { return 4; }

static int check_cfg(const gt_config* c) {
  if (!c) return gt_fail("gt_config is NULL");
  if (c->batch <= 0) return gt_fail("batch must be > 0 (got %d)", c->batch);
  if (c->d_model <= 0 || c->d_model > GT_MAX_D) return gt_fail("d_model %d outside 1..%d", c->d_model, GT_MAX_D);
  if (c->n_heads <= 0 || c->d_model % c->n_heads != 0)   // torch:nn/functional.py:6415-6417
    return gt_fail("embed_dim %d not divisible by num_heads %d", c->d_model, c->n_heads);
  if (c->d_model % 2 != 0) return gt_fail("d_model %d must be even (sin/cos positional encoding)", c->d_model);
  if (c->dim_ff <= 0 || c->src_dim <= 0) return gt_fail("dim_ff / src_dim must be > 0");
  if (c->n_enc_layers <= 0 || c->n_enc_layers > 64 || c->n_dec_layers < 0 || c->n_dec_layers > 64)
    return gt_fail("layer counts out of range (enc %d, dec %d)", c->n_enc_layers, c->n_dec_layers);
  if (!(c->dropout >= 0.f && c->dropout < 1.f)) return gt_fail("dropout %f outside [0,1)", (double)c->dropout);
  if (c->flags & ~(GT_CFG_NO_QUAD | GT_CFG_NO_LN_XCHG)) return gt_fail("gt_config.flags %d has unknown bits", c->flags);
  if (c->precision < 0 || c->precision > 2) return gt_fail("precision %d unknown (0 = fp32, 1 = bf16 GEMM operands, 2 = ... and bf16 storage of the Linear outputs)", c->precision);
  if ((int64_t)c->batch * 32 * (c->dim_ff > 3 * c->d_model ? c->dim_ff : 3 * c->d_model) >= (1ll << 31))
    return gt_fail("batch %d too large for 32-bit element indices", c->batch);
  // every LayerNorm instance gets one row of the dgamma/dbeta partials table (LnJobs): refuse here, before any launch,
  // what backward could not finish
  const int n_ln = 2 * c->n_enc_layers + 3 * c->n_dec_layers + (c->n_dec_layers > 0 ? 2 : 1);
  if (n_ln > GT_LN_JOBS_MAX)
    return gt_fail("%d LayerNorm instances (enc %d, dec %d layers) exceed the %d the backward's partials table holds",
                   n_ln, c->n_enc_layers, c->n_dec_layers, GT_LN_JOBS_MAX);
  return 0;
}

// ------------------------------------------------------------------------------------ parameter layout
struct AttnP { int64_t in_w, in_b, out_w, out_b; };
struct LayerP { AttnP sa, xa; int64_t w1, b1, w2, b2, n1w, n1b, n2w, n2b, n3w, n3b; };
struct PEntry { int64_t off, size; int rows, cols; };
struct PLayout {
  int64_t in_w, in_b, encn_w, encn_b, din_w, din_b, decn_w, decn_b, out_w, out_b, total;
  std::vector<LayerP> enc, dec;
  std::vector<PEntry> entries;
};
static PLayout param_layout(const gt_config& c) {
  PLayout L;
  int64_t cur = 0;
  auto add = [&](int rows, int cols) {
    const int64_t size = (int64_t)rows * (cols ? cols : 1);
    const int64_t off = cur;
    L.entries.push_back(PEntry{off, size, rows, cols});
    cur += (size + 63) / 64 * 64;          // 256-byte aligned tensors: float4 loads, clean all-reduce buckets
    return off;
  };
  const int d = c.d_model, F = c.dim_ff;
  auto attn = [&](AttnP& a) { a.in_w = add(3 * d, d); a.in_b = add(3 * d, 0); a.out_w = add(d, d); a.out_b = add(d, 0); };
  L.in_w = add(d, c.src_dim); L.in_b = add(d, 0);
  L.enc.resize(c.n_enc_layers);
  for (auto& l : L.enc) {
    attn(l.sa);
    l.w1 = add(F, d); l.b1 = add(F, 0); l.w2 = add(d, F); l.b2 = add(d, 0);
    l.n1w = add(d, 0); l.n1b = add(d, 0); l.n2w = add(d, 0); l.n2b = add(d, 0);
  }
  L.encn_w = add(d, 0); L.encn_b = add(d, 0);
  L.dec.resize(c.n_dec_layers);
  if (c.n_dec_layers > 0) {
    L.din_w = add(d, GT_TGT); L.din_b = add(d, 0);
    for (auto& l : L.dec) {
      attn(l.sa); attn(l.xa);
      l.w1 = add(F, d); l.b1 = add(F, 0); l.w2 = add(d, F); l.b2 = add(d, 0);
      l.n1w = add(d, 0); l.n1b = add(d, 0); l.n2w = add(d, 0); l.n2b = add(d, 0); l.n3w = add(d, 0); l.n3b = add(d, 0);
    }
    L.decn_w = add(d, 0); L.decn_b = add(d, 0);
  }
  L.out_w = add(GT_TGT, d); L.out_b = add(GT_TGT, 0);
  L.total = cur;
  return L;
}

extern "C" int gt_param_count(const gt_config* cfg, int64_t* n_tensors, int64_t* n_floats) {
  if (check_cfg(cfg)) return -1;
  PLayout L = param_layout(*cfg);
  if (n_tensors) *n_tensors = (int64_t)L.entries.size();
  if (n_floats) *n_floats = L.total;
  return 0;
}
extern "C" int gt_param_layout(const gt_config* cfg, int64_t* offsets, int64_t* sizes, int32_t* rows, int32_t* cols) {
  if (check_cfg(cfg)) return -1;
  PLayout L = param_layout(*cfg);
  for (size_t i = 0; i < L.entries.size(); ++i) {
    if (offsets) offsets[i] = L.entries[i].off;
    if (sizes) sizes[i] = L.entries[i].size;
    if (rows) rows[i] = L.entries[i].rows;
    if (cols) cols[i] = L.entries[i].cols;
  }
  return 0;
}

// ------------------------------------------------------------------------------------ workspace layout
struct LayerW {
  int64_t qkv, P, ctx, xhat1, rstd1, x1;            // self-attention block
  int64_t qx, kvx, Px, ctxx, xhatx, rstdx, x2;      // decoder cross-attention block
  int64_t hact, xhat2, rstd2, xout;                 // FFN block (xhat2/rstd2 = the layer's LAST norm)
};
// One entry per region ws_layout() hands out: the single description of the workspace that gt_ws_find, sh_act and only16 answer from.
struct WRegion {
  const char* name;         // what gt_ws_find answers to (nullptr: private)
  int layer;                // global layer index (-1: one per workspace)
  int64_t off, n;           // in floats
  int64_t sh = -1;          // offset of its bf16 shadow (precision = 1, bf16_shadows()), for the activations whose producers write one
  bool only = false;        // level 2: stored in bf16 alone (the fp32 region stays allocated, unwritten)
};
struct WLayout {
  std::vector<WRegion> regions;
  int64_t x0, a0, enc_xhat, enc_rstd, memory, y0, b0, dec_xhat, dec_rstd, dec_final;
  std::vector<LayerW> layers;                        // encoder layers then decoder layers
  int64_t hvo_tmp, dlogits, loss_part, dctx, dmem, da0_dec, ln_part, ln_part_stride, total, stamps = 0;
  int64_t pack_f = -1, pack_b = -1, pack_stride = 0;   // fragment-ordered weight copies of the sequence-resident kernels (gt_seq.h)
  int64_t seq_dctx = -1;                               // hand-over buffer of their two-workgroups-per-sequence (SPLIT) backward phases
  int64_t seq_xchg = -1, seq_xchg_n = 0;               // pair-exchange region of their four-workgroups-per-sequence (QUAD) forward
  int64_t rowx = -1, rowx_n = 0;                       // row exchange of the LayerNorm-fused 64x64-tile Linears (gt_gemm64.h; d_model 256 / 512)
  int64_t seq_amask = -1, seq_amask_stride = 0;        // dropout keep bits of P, one word per (layer, sequence, head, query): their head_dim-2 attention
  // bf16 shadows (precision = 1, bf16_shadows()) of the encoder layers' four matrices and their transposes, [in_w | out_w | w1 | w2] per layer
  int64_t w16 = -1, w16t = -1, w16_stride = 0;
  int64_t kbits = -1, kbits_stride = 0;                // keep bits of the FFN activation, [layer][M / 32][F / 32][64] 16-bit words (gt_gemm32.h; round 6)
  int64_t wT = -1, wT_stride = 0;                      // precision = 1 without shadows: fp32 transposes of the encoder layers' matrices (dgrads as NT)
  struct TmpSet { int64_t dzA, dzAm, dzB, dzBm, dzC, dzCm, dhid, dqkv, dqkvx; };
  std::vector<TmpSet> set;                           // one per layer
};
// Every layer keeps its own backward temporaries, so ALL weight gradients of the step leave as one grouped dispatch per
// tile class at the end of backward instead of one per layer: fewer kernel boundaries (~4 us each: C2 0.333 -> 0.319 ms)
// and better-balanced launches (C4 bs512 11.0 -> 10.5 ms).
static bool seq_supported(const gt_config& c);
// bf16 SHADOWS of the GEMM operands (precision = 1): where the Linears of the encoder layers run on the big-tile kernel -- interior
// 128-tiles, at least GT_T128H_MIN of them -- and the tensors' producers are the kernels that can write a bf16 copy (LayerNorm passes of d_model 256 /
// 512, the MFMA attention kernels).
#ifndef GT_T128_BIG_MIN
#define GT_T128_BIG_MIN 192
#endif
// Level 1 = shadows BESIDE the fp32 tensors.  Measured (round 4, C5 bs 512, tools/rejected/bf16_shadows.md): the Linears' forward / dgrad
// GEMMs get 1.3-1.4x faster, but the shadows are ADDITIONAL bytes -- the producers (attention, LayerNorm passes, FFN epilogues) pay what
// the GEMMs gain, and the weight gradients are not bound by their operand fetch at all: 4.03-4.07 ms with, 4.04 ms without.
// gt_set_operand_shadows(0 / 1 / 2) / GT_BF16_SHADOWS select the level; results are bit-identical at every level.
// Level 2 (the default where the path applies): the tensors that are ONLY ever consumed as bf16-rounded GEMM operands -- ctx, hact, dhid,
// dqkv and the dropout-masked dz copies of the encoder layers -- are stored in bf16 ALONE: their producers write 2 bytes per element
// instead of 4 (+ 2), every consumer (Linear, dgrad, weight gradient, the FFN2 dgrad's zero test of hact) takes the bf16 tensor.  Outputs,
// losses and gradients are bit for bit those of level 0 / 1 (the fp32-source GEMMs round the same values at fragment assembly):
// C5 bs 512 4.06 -> 3.6 ms.  gt_ws_find names the bf16 tensors "<name>16"; the fp32 regions of those six stay allocated, unwritten.
static int bf16_shadow_level() { return (int)gt_switch(GT_SW_OPERAND_SHADOWS); }
// every change of the shadow level IN FORCE -- the one switch the workspace LAYOUT depends on -- bumps this counter: a host that caches workspaces
// compares it before it reuses one (StepEngine.slot re-makes the slot: offsets move with the level, and a workspace sized for another is too small or mis-read)
static int g_layout_epoch = 0;
extern "C" int gt_layout_epoch() { return g_layout_epoch; }
extern "C" int gt_set_operand_shadows(int level) {
  const int was = bf16_shadow_level();
  gt_switch_set(GT_SW_OPERAND_SHADOWS, level > 2 ? 2 : level);
  if (bf16_shadow_level() != was) ++g_layout_epoch;
  return 0;
}
// precision = 1 where the shadows do not apply: fp32 W^T copies of the encoder layers' matrices, so that the dgrads run in the NT form
// (results: the same products, summed in the NT kernel's k order)
static bool bf16_shadows(const gt_config& c);
static bool bf16_wt(const gt_config& c) {
  return c.precision >= 1 && c.n_enc_layers > 0 && c.d_model % 32 == 0 && c.dim_ff % 32 == 0 && !bf16_shadows(c);
}
static bool bf16_shadows(const gt_config& c) {
  const int on = bf16_shadow_level() > 0;
  const int64_t M = (int64_t)c.batch * 32;
  const int hd = c.n_heads > 0 ? c.d_model / c.n_heads : 0;
  const int nmin = c.d_model < c.dim_ff ? c.d_model : c.dim_ff;            // every Linear of a layer on the big-tile kernel (its epilogue writes hact16 / dhid16)
  return on && c.precision >= 1 && c.n_enc_layers > 0 && (c.d_model == 256 || c.d_model == 512) && c.dim_ff % 128 == 0 &&
         M % 128 == 0 && (hd == 16 || hd == 32 || hd == 64 || hd == 128) && (M / 128) * (nmin / 128) >= GT_T128H_MIN;
}
// precision = 2 (round 5): bf16 where the bytes are.  On top of precision 1's operand-only tensors (level 2 of the shadows: ctx, hact, dhid,
// dqkv, masked dz copies) every Linear OUTPUT of the encoder layers that torch.autocast(bfloat16) would hand on as bf16 is stored in bf16
// alone: qkv (read by the attention kernels: fp32 arithmetic on bf16-stored q / k / v), the out-proj / linear2 outputs ahead of their
// LayerNorm, the dgrad outputs ahead of a LayerNorm backward, and dctx (out-proj dgrad -> attention backward).  The residual stream, the
// LayerNorm statistics / xhat, softmax, loss, master weights and optimizer stay fp32.  Applies where the level-2 shadows apply and the
// heads are 64 or 128 wide (the LDS-staged attention kernels); elsewhere precision 2 runs as precision 1 (gt_precision_in_force).
static bool p2(const gt_config& c) {
  const int hd = c.n_heads > 0 ? c.d_model / c.n_heads : 0;
  return c.precision == 2 && bf16_shadows(c) && bf16_shadow_level() >= 2 && (hd == 64 || hd == 128);
}
extern "C" int gt_precision_in_force(const gt_config* cfg) {
  if (check_cfg(cfg)) return -1;
  return p2(*cfg) ? 2 : (cfg->precision ? 1 : 0);
}
static WLayout ws_layout(const gt_config& c) {
  WLayout W;
  int64_t cur = 0;
  const int nl = c.n_enc_layers + c.n_dec_layers;
  W.regions.reserve(40 + 34 * (size_t)nl);
  auto add = [&](const char* name, int layer, int64_t n) { int64_t o = cur; cur += (n + 63) / 64 * 64; W.regions.push_back(WRegion{name, layer, o, n}); return o; };
#define WS(s, f, layer, n) s.f = add(#f, layer, n)          // a public region: gt_ws_find answers to the field's name
  const int64_t M = (int64_t)c.batch * 32, d = c.d_model, F = c.dim_ff, BH = (int64_t)c.batch * c.n_heads;
  WS(W, x0, -1, M * d); WS(W, a0, -1, M * d);
  W.layers.resize(nl);
  for (int l = 0; l < nl; ++l) {
    LayerW& w = W.layers[l];
    WS(w, qkv, l, M * 3 * d); WS(w, P, l, BH * 1024); WS(w, ctx, l, M * d);
    WS(w, xhat1, l, M * d); WS(w, rstd1, l, M); WS(w, x1, l, M * d);
    if (l >= c.n_enc_layers) {
      WS(w, qx, l, M * d); WS(w, kvx, l, M * 2 * d); WS(w, Px, l, BH * 1024); WS(w, ctxx, l, M * d);
      WS(w, xhatx, l, M * d); WS(w, rstdx, l, M); WS(w, x2, l, M * d);
    } else {
      w.qx = w.kvx = w.Px = w.ctxx = w.xhatx = w.rstdx = w.x2 = -1;
    }
    WS(w, hact, l, M * F); WS(w, xhat2, l, M * d); WS(w, rstd2, l, M); WS(w, xout, l, M * d);
  }
  WS(W, enc_xhat, -1, M * d); WS(W, enc_rstd, -1, M); WS(W, memory, -1, M * d);
  if (c.n_dec_layers > 0) {
    WS(W, y0, -1, M * d); WS(W, b0, -1, M * d); W.dec_xhat = add(nullptr, -1, M * d); W.dec_rstd = add(nullptr, -1, M); WS(W, dec_final, -1, M * d);
    WS(W, dmem, -1, M * d); W.hvo_tmp = add(nullptr, -1, M * GT_TGT);
  } else {
    W.y0 = W.b0 = W.dec_xhat = W.dec_rstd = W.dec_final = W.dmem = W.hvo_tmp = -1;
  }
  WS(W, dlogits, -1, M * GT_TGT);
  W.loss_part = add(nullptr, -1, std::max<int64_t>(((M * GT_VOICES + 255) / 256) * 4, 8 * (int64_t)c.batch));   // loss_kernel's / the fused loss's workgroups x 4
  // dgamma/dbeta partials: one [row_tiles][2][d] block per LayerNorm instance (2 per encoder layer, 3 per decoder
  // layer, the final norms)
  W.ln_part_stride = ((M + 7) / 8) * 2 * d;
  W.ln_part = add(nullptr, -1, W.ln_part_stride * (2 * c.n_enc_layers + 3 * c.n_dec_layers + 2));
  WS(W, dctx, -1, M * d);
  W.da0_dec = c.n_dec_layers > 0 ? add(nullptr, -1, M * d) : -1;
  // Backward temporaries: one set per layer (the weight gradients read them at the end of backward)
  W.set.resize(nl);
  for (int k = 0; k < nl; ++k) {
    WLayout::TmpSet& t = W.set[k];
    WS(t, dzA, k, M * d); WS(t, dzAm, k, M * d); WS(t, dzB, k, M * d); WS(t, dzBm, k, M * d);
    WS(t, dhid, k, M * F); WS(t, dqkv, k, M * 3 * d);
    if (c.n_dec_layers > 0) { WS(t, dzC, k, M * d); WS(t, dzCm, k, M * d); WS(t, dqkvx, k, M * 3 * d); }
    else { t.dzC = t.dzCm = t.dqkvx = -1; }
  }
  if (seq_supported(c)) {
    W.pack_stride = (int64_t)4 * d * d + (int64_t)2 * d * F;
    WS(W, pack_f, -1, W.pack_stride * c.n_enc_layers); WS(W, pack_b, -1, W.pack_stride * c.n_enc_layers);
    W.seq_dctx = add(nullptr, -1, 2 * M * d);
    if (d == 128) { W.seq_xchg_n = 2 * gt_seq_xchg_floats(c.batch); WS(W, seq_xchg, -1, W.seq_xchg_n); }    // (two regions: the forward's, and backward phase 0's when fused behind it)
    if ((d == 32 || d == 64) && c.n_heads == 16) { W.seq_amask_stride = BH * 32; W.seq_amask = add("amask", -1, W.seq_amask_stride * c.n_enc_layers); }   // (behind everything else: no other offset moves)
  }
  if (!seq_supported(c) && (d == 256 || d == 512) && M % 64 == 0) { W.rowx_n = gt_rowx_floats(M, (int)d); WS(W, rowx, -1, W.rowx_n); }
  if (bf16_shadows(c)) {
    // the bf16 shadow of the region at fp32 offset `off` (half its floats; `with`: the shadow it shares); gt_ws_find names it "<name>16"
    auto sh = [&](int64_t off, bool only, int64_t with = -1) {
      size_t i = 0;
      while (i < W.regions.size() && (W.regions[i].off != off || W.regions[i].n <= 0)) ++i;
      assert(i < W.regions.size() && "shadow of an offset ws_layout did not hand out");
      const int64_t s = with >= 0 ? with : add(nullptr, -1, (W.regions[i].n + 1) / 2);
      W.regions[i].sh = s; W.regions[i].only = only;
      return s;
    };
    const bool only = bf16_shadow_level() >= 2;
    sh(W.x0, false);        // (round 5: the input layer's output -- layer 0's in-proj and its weight gradient then run with both operands in bf16 like every other layer's)
    for (int l = 0; l < c.n_enc_layers; ++l) {
      const LayerW& w = W.layers[l];
      sh(w.ctx, only); sh(w.x1, false); sh(w.hact, only);
      if (l + 1 < c.n_enc_layers) sh(w.xout, false);          // (the top layer's output comes from the two-norm pass, and feeds no big GEMM)
    }
    for (int k = 0; k < c.n_enc_layers; ++k) {        // (one set per layer: the encoder layers' are the first L)
      const WLayout::TmpSet& t = W.set[k];
      // dz / dzm share a shadow: the consumer takes the masked copy when there is dropout, else dz itself (tmp_set)
      // (dzAm / dzBm exist as tensors of their own only with dropout; without it the operand is dz itself, which stays fp32)
      const int64_t a = sh(t.dzA, false), b = sh(t.dzB, false);
      sh(t.dzAm, only, a); sh(t.dzBm, only, b);
      sh(t.dhid, only); sh(t.dqkv, only);
    }
    W.w16_stride = ((int64_t)4 * d * d + (int64_t)2 * d * F + 1) / 2;          // floats per layer
    W.w16 = add(nullptr, -1, W.w16_stride * c.n_enc_layers); W.w16t = add(nullptr, -1, W.w16_stride * c.n_enc_layers);
  } else if (bf16_wt(c)) {
    W.wT_stride = (int64_t)4 * d * d + (int64_t)2 * d * F;
    W.wT = add(nullptr, -1, W.wT_stride * c.n_enc_layers);
  }
  // (behind everything else: no other offset moves.  One bit per element of hact: M F / 32 floats per layer)
  if (!seq_supported(c) && F % 32 == 0) { W.kbits_stride = (M * F / 32 + 63) / 64 * 64; W.kbits = add(nullptr, -1, W.kbits_stride * nl); }
#ifdef GT_SEQ_STAMPS
  WS(W, stamps, -1, 2048 + 2 * 4 * 512);
#endif
#undef WS
  W.total = cur;
  return W;
}
extern "C" size_t gt_workspace_bytes(const gt_config* cfg) {
  if (check_cfg(cfg)) return 0;
  return (size_t)ws_layout(*cfg).total * sizeof(float);
}
// One-off preparation of a fresh workspace: zeroes the region whose protocol relies on it (the QUAD forward's pair exchange: every
// granule is zero between launches, the consumer re-zeroes what it has read).  Stream-ordered, capturable; a no-op for shapes without
// such a region.
static int launch_status(const char* what);
extern "C" int gt_workspace_init(const gt_config* cfg, float* ws, gt_stream_t stream) {
  if (check_cfg(cfg)) return -1;
  if (!ws) return gt_fail("gt_workspace_init: ws must not be NULL");
  const WLayout W = ws_layout(*cfg);
  if (W.seq_xchg >= 0) (void)hipMemsetAsync(ws + W.seq_xchg, 0, (size_t)W.seq_xchg_n * sizeof(float), (hipStream_t)stream);
  if (W.rowx >= 0) (void)hipMemsetAsync(ws + W.rowx, 0, (size_t)W.rowx_n * sizeof(float), (hipStream_t)stream);      // (tag 0 never matches: serials start at 1)
  return launch_status("gt_workspace_init");
}
// 0: no bf16 operand shadows for this configuration; 1: beside the fp32 tensors; 2: ctx / hact / dhid / dqkv / masked dz copies of the
// encoder layers stored in bf16 ALONE (gt_ws_find "<name>16")
extern "C" int gt_operand_shadow_level(const gt_config* cfg) {
  if (check_cfg(cfg)) return -1;
  return bf16_shadows(*cfg) ? bf16_shadow_level() : 0;
}
// The error word of whichever in-launch exchange region this shape has (offset in floats, -1: none).  rowx and seq_xchg are mutually
// exclusive (rowx requires !seq_supported), so the precedence does not matter.
static int64_t xchg_err_off(const WLayout& W) { return W.rowx >= 0 ? W.rowx : W.seq_xchg; }
static unsigned* xchg_err(const WLayout& W, const float* ws) {
  const int64_t eo = xchg_err_off(W);
  return eo >= 0 ? reinterpret_cast<unsigned*>(const_cast<float*>(ws) + eo) : nullptr;
}
// Answers from the table of ws_layout: every public region by its name (per-layer ones at `layer`), "<name>16" = its bf16 shadow (offset in
// floats, count = the floats it occupies: two bf16 per float).  Not regions of their own: "w16" / "w16t" (the weight shadows of encoder
// layer `layer`), "xchg_err", and precision 2's "qkv16" / "dctx16" (bf16 tensors in the first half of the fp32 tensor's region).
extern "C" int gt_ws_find(const gt_config* cfg, const char* name, int layer, int64_t* offset, int64_t* count) {
  if (check_cfg(cfg)) return -1;
  const gt_config& c = *cfg;
  const WLayout W = ws_layout(c);
  std::string n(name);
  if (n == "w16" || n == "w16t") {
    if (W.w16 < 0 || layer < 0 || layer >= c.n_enc_layers) return gt_fail("gt_ws_find: no weight shadows for this configuration / layer");
    *offset = (n == "w16" ? W.w16 : W.w16t) + W.w16_stride * layer; *count = W.w16_stride;
    return 0;
  }
  const bool want16 = n.size() > 2 && n.compare(n.size() - 2, 2, "16") == 0;
  if (want16) n.resize(n.size() - 2);
  const bool inplace16 = want16 && (n == "qkv" || n == "dctx") && p2(c);
  if (inplace16 && n == "qkv" && (layer < 0 || layer >= c.n_enc_layers)) return gt_fail("gt_ws_find: qkv16: layer %d is not an encoder layer", layer);
  int64_t off = -1, cnt = 0, sh = -1;
  bool other_layer = false;
  if (n == "xchg_err") { off = xchg_err_off(W); cnt = 2; }
  else for (const WRegion& r : W.regions) {
    if (r.name == nullptr || n != r.name) continue;
    if (r.layer < 0 || r.layer == layer) { off = r.off; cnt = r.n; sh = r.sh; break; }
    other_layer = true;
  }
  if (off < 0 && other_layer && (layer < 0 || layer >= (int)W.layers.size())) return gt_fail("gt_ws_find: layer %d out of range", layer);
  if (off < 0) return gt_fail("gt_ws_find: unknown or absent buffer '%s'", name);
  if (want16 && !inplace16) {
    if (sh < 0) return gt_fail("gt_ws_find: '%s' has no bf16 shadow in this configuration", name);
    off = sh;
  }
  *offset = off; *count = want16 ? (cnt + 1) / 2 : cnt;
  return 0;
}

// ------------------------------------------------------------------------------------ launch helpers
// The sequence-resident schedule of ONE call (seq_plan(), below the rules it wraps): an entry point asks once, and the forward, the
// backward, the bucket cut and the update of that call all read the same answers.  hc: the head-dim class of the kernels' instantiations.
struct SeqPlan { bool seq, split, quad, ride, fuse_b0; int hc; };
struct Ctx {
  gt_config c;
  SeqPlan plan;              // all false from make_ctx; forward, backward and the fused step fill it (seq_plan)
  PLayout P;
  WLayout W;
  int M, d, F, H, hd;
  const float* prm;
  float* grd;
  float* ws;
  const gt_step_state* st;
  bool drop;                 // train mode with p > 0
  hipStream_t s;
  WgradBatch* wb;            // weight gradients queue up here and leave as grouped dispatches
  LnJobs* ln;                // LayerNorm parameter-gradient partials to be summed at the end of backward
  mutable const char* refused;   // first bf16-only tensor that met a kernel which cannot take it (need16 writes, launch_status reports): dies with the call
};
// next partials block for a LayerNorm backward launched with `nwg` workgroups; registers the reduction job
static float* ln_job(const Ctx& x, int64_t gamma_off, int nwg) {
  if (!x.ln || x.ln->n >= GT_LN_JOBS_MAX) return nullptr;          // fall back to atomics
  float* part = x.ws + x.W.ln_part + x.W.ln_part_stride * x.ln->n;
  LnJob& j = x.ln->j[x.ln->n++];
  j.part = part; j.dgamma = x.grd + gamma_off; j.dbeta = x.grd + gamma_off + (x.d + 63) / 64 * 64; j.nwg = nwg;
  return part;
}
// the table entry of a workspace tensor that has a bf16 shadow (nullptr: it has none)
static const WRegion* shadowed(const Ctx& x, const float* p) {
  if (x.W.w16 < 0 || p == nullptr) return nullptr;            // (operand shadows and weight shadows come together: bf16_shadows())
  const int64_t off = p - x.ws;
  for (const WRegion& r : x.W.regions) if (r.sh >= 0 && r.off == off) return &r;
  return nullptr;
}
static uint16_t* sh_act(const Ctx& x, const float* p) {
  const WRegion* r = shadowed(x, p);
  return r ? reinterpret_cast<uint16_t*>(x.ws + r->sh) : nullptr;
}
// level 2: is this workspace tensor stored in bf16 alone (its fp32 region is not written)?
static bool only16(const Ctx& x, const float* p) {
  const WRegion* r = shadowed(x, p);
  return r && r->only;
}
// a consumer of a bf16-only tensor that could not take the bf16-source kernel would read an unwritten fp32 region: refuse loudly
static void need16(const Ctx& x, bool ok, const char* what) { if (!ok && x.refused == nullptr) x.refused = what; }
// where an encoder-layer weight matrix lies in a copy that keeps [in_w | out_w | w1 | w2] per layer, `stride` elements apart (-1: not one of them)
static int64_t enc_w_slot(const Ctx& x, const float* W, int64_t stride) {
  const int64_t off = W - x.prm, d = x.d, F = x.F;
  for (int l = 0; l < x.c.n_enc_layers; ++l) {
    const LayerP& p = x.P.enc[l];
    if (off == p.sa.in_w) return stride * l;
    if (off == p.sa.out_w) return stride * l + 3 * d * d;
    if (off == p.w1) return stride * l + 4 * d * d;
    if (off == p.w2) return stride * l + 4 * d * d + d * F;
  }
  return -1;
}
// fp32 transposed copy of an encoder-layer weight matrix (precision = 1 without shadows), or nullptr
static const float* wT_of(const Ctx& x, const float* W) {
  const int64_t slot = x.W.wT >= 0 ? enc_w_slot(x, W, x.W.wT_stride) : -1;
  return slot >= 0 ? x.ws + x.W.wT + slot : nullptr;
}
// bf16 shadow of an encoder-layer weight matrix (transposed: the copy that turns a dgrad into the NT form), or nullptr
static const uint16_t* sh_w(const Ctx& x, const float* W, bool transposed) {
  const int64_t slot = x.W.w16 >= 0 ? enc_w_slot(x, W, 2 * x.W.w16_stride) : -1;
  return slot >= 0 ? reinterpret_cast<const uint16_t*>(x.ws + (transposed ? x.W.w16t : x.W.w16)) + slot : nullptr;
}
struct Tmp { float *dzA, *dzAm, *dzB, *dzBm, *dzC, *dzCm, *dhid, *dqkv, *dqkvx; };
static Tmp tmp_set(const Ctx& x, int gl) {
  const WLayout::TmpSet& t = x.W.set[gl];
  float* ws = x.ws;
  Tmp r;
  r.dzA = ws + t.dzA; r.dzAm = x.drop ? ws + t.dzAm : r.dzA;
  r.dzB = ws + t.dzB; r.dzBm = x.drop ? ws + t.dzBm : r.dzB;
  r.dzC = t.dzC >= 0 ? ws + t.dzC : nullptr; r.dzCm = t.dzC >= 0 ? (x.drop ? ws + t.dzCm : r.dzC) : nullptr;
  r.dhid = ws + t.dhid; r.dqkv = ws + t.dqkv; r.dqkvx = t.dqkvx >= 0 ? ws + t.dqkvx : nullptr;
  return r;
}
static DropArgs mk_drop(const Ctx& x, int site) {
  DropArgs da;
  da.st = x.drop ? x.st : nullptr;
  da.site = (uint32_t)site;
  da.thr = x.drop ? (uint32_t)(x.c.dropout * 16777216.0f) : 0u;
  da.scale = x.drop ? 1.0f / (1.0f - x.c.dropout) : 1.0f;
  return da;
}
static DropArgs no_drop() { DropArgs da; da.st = nullptr; da.site = 0u; da.thr = 0u; da.scale = 1.0f; return da; }
static int lsite(int gl, int kind) { return GT_SITE_LAYER0 + 8 * gl + kind; }
static GemmArgs mk_gemm(const Ctx& x, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.B = B; g.C = C; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
  g.mask_scale = 1.0f;
  g.drop.scale = 1.0f;
  g.bf16 = x.c.precision ? 1 : 0;
  return g;
}
// y = x W^T + b  (forward "NT");  out16 (precision = 2): y stored in bf16 ALONE at out16 (row stride ldout), `out` not written
static void linear_fwd(const Ctx& x, const float* in, int ldin, const float* W, const float* b, float* out, int ldout,
                       int N, int K, uint16_t* out16 = nullptr) {
  GemmArgs g = mk_gemm(x, in, ldin, W, K, out16 ? nullptr : out, ldout, x.M, N, K);
  g.bias = b;
  if (ldin == K) { g.A16 = sh_act(x, in); g.B16 = sh_w(x, W, false); g.lda16 = g.ldb16 = K; }
  if (out16) { g.C16 = out16; g.ldc16 = ldout; need16(x, gemm_on_big_kernel<false, EPI_STORE>(g), "Linear with a bf16-only output (precision 2)"); }
  if (only16(x, in)) need16(x, g.A16 && g.B16 && gemm32h_ok(g, EPI_STORE), "Linear forward of a bf16-only tensor");
  gemm_launch<false, false, EPI_STORE>(g, x.s);
}
// dW (N_w x K_w) += dY^T X ; db += colsum(dY)       ("TN", split over tokens, fp32 atomics)
static void wgrad(const Ctx& x, const float* dY, int ldy, const float* X, int ldx, float* dW, float* db, int Nw, int Kw) {
  GemmArgs g = mk_gemm(x, dY, ldy, X, ldx, dW, Kw, Nw, Kw, x.M);
  g.dbias = db;
  if (ldy == Nw && ldx == Kw) { g.A16 = sh_act(x, dY); g.B16 = sh_act(x, X); g.lda16 = Nw; g.ldb16 = Kw; }     // bf16 shadows of dY / X (precision = 1)
  if (only16(x, dY) || only16(x, X)) {
    const long t128 = (long)(Nw / 128) * (Kw / 128);
    need16(x, x.wb != nullptr && g.A16 && (g.B16 || !only16(x, X)) && wgrad32_ok(g) && t128 * ((x.M + 511) / 512) >= GT_WGRAD_T128_MIN,
           "weight gradient of a bf16-only tensor");
  }
  if (x.wb) wgrad_queue(*x.wb, g, x.s);
  else gemm_launch<true, true, EPI_ATOMIC>(g, x.s);
}
extern "C" int gt_set_deterministic(int on) { return gt_switch_set_flag(GT_SW_DETERMINISTIC, on); }

// dX = dY W   ("NN")
// out16 (precision = 2): the result stored in bf16 ALONE at out16 (dense rows of N); dX is then not written
static void dgrad_store(const Ctx& x, const float* dY, int ldy, const float* W, int ldw, float* dX, int N, int K, int accumulate,
                        uint16_t* out16 = nullptr) {
  if (out16 != nullptr) {
    GemmArgs g = mk_gemm(x, dY, ldy, W, ldw, nullptr, N, x.M, N, K);
    if (ldy == K && ldw == N) { g.A16 = sh_act(x, dY); g.B16 = sh_w(x, W, true); g.lda16 = g.ldb16 = K; }
    g.C16 = out16; g.ldc16 = N;
    need16(x, !accumulate && gemm_on_big_kernel<true, EPI_STORE>(g) && (!only16(x, dY) || (g.A16 && g.B16)), "dgrad with a bf16-only output (precision 2)");
    gemm_launch<false, true, EPI_STORE>(g, x.s);
    return;
  }
  if (const float* wt = (ldw == N) ? wT_of(x, W) : nullptr) {      // dX = dY (W^T)^T: the NT form over the transposed copy
    GemmArgs g = mk_gemm(x, dY, ldy, wt, K, dX, N, x.M, N, K);
    g.accumulate = accumulate; g.as_dgrad = 1;
    gemm_launch<false, false, EPI_STORE>(g, x.s);
    return;
  }
  GemmArgs g = mk_gemm(x, dY, ldy, W, ldw, dX, N, x.M, N, K);
  g.accumulate = accumulate;
  if (ldy == K && ldw == N) { g.A16 = sh_act(x, dY); g.B16 = sh_w(x, W, true); g.lda16 = g.ldb16 = K; }      // (W^T: [N][K], k contiguous)
  if (only16(x, dY)) need16(x, g.A16 && g.B16 && gemm32h_ok(g, EPI_STORE), "dgrad of a bf16-only tensor");
  gemm_launch<false, true, EPI_STORE>(g, x.s);
}
// dz = LNbwd(dY W + res) with the LayerNorm whose (xhat, rstd, gamma) are given; dzm = dz * dropout mask
// Row-owning GEMM tiles fuse the LayerNorm into the producing linear -- but every workgroup then streams the WHOLE weight
// matrix.  Wide d_model at few tokens (d 512, M 2048: 128 workgroups x up to 3 MB at ~40 GB/s per CU) makes that the bound
// (23 TF measured); there the linear runs as an ordinary tiled GEMM and the norm as its own in-place row pass.
#ifndef GT_ROW_FUSE_MAX_D
#define GT_ROW_FUSE_MAX_D 64
#endif
#ifndef GT_ROW_FUSE_MIN_M
#define GT_ROW_FUSE_MIN_M 8192
#endif
// (bf16 operands: always the tiled GEMM + row pass -- the row-owning tiles exist in fp32 only)
// Round 3: at d_model 512 the row-owning tiles never pay -- 64 x 512 tiles on the one-deep 16x16x4 body run at 52 % (forward) / 65 %
// (backward) of the MFMA peak where the 128 x 128 ring GEMM + an HBM-bound row pass make 80 % + 25 us (C4 bs512: 9.28 -> 8.91 ms;
// d_model 256 at 8192 tokens keeps the fused tiles: 5.57 vs 5.66 ms)
#ifndef GT_ROW_FUSE_BIG_MAX_D
#define GT_ROW_FUSE_BIG_MAX_D 256
#endif
// LayerNorm inside the producing Linear / dgrad on 64x64 tiles with the in-launch row exchange (gt_gemm64.h): -1 = wherever it applies (d_model 256 /
// 512 outside the row-owning tiles, 3/4 .. 2 tiles of 64x64 per CU: the whole grid resident at once), 0 = off (GT_LN_XCHG=0 / gt_set_ln_exchange(0):
// the norm as a row pass of its own).  22 launches fewer per step at d_model 512.  Measured at 2048 tokens (round 5, A/B on one box, two rounds): C4 bs 64
// 1.488 / 1.492 -> 1.472 / 1.474 ms, C5 bf16 bs 64 0.944 / 0.936 -> 0.931 / 0.933, precision 2 0.929 / 0.932 -> 0.916 / 0.918 -- with the one-hop hand-off
// (tagged granules, coalesced); the three-hop "data, drain, ready word" form was neutral (1.494 vs 1.494, bf16 0.984 vs 0.968), a first form with
// per-row granules (16 scattered polls per lane) cost 13 us per launch (1.811 ms).  C3 (d_model 256, 8192 tokens): 5.20 ms on the row-owning tiles, 5.29
// on 64x64 tiles + row pass, 5.44 with the three-hop exchange, 5.06 with this one (row_fused below).
extern "C" int gt_set_ln_exchange(int on) { return gt_switch_set_flag(GT_SW_LN_XCHG, on); }
static int seq_cu_count();
static int xchg_cus();
// polling bound of an in-launch exchange: gt_set_xchg_spin_max's while positive, else the exchange's compiled default
static int xchg_spin_max(int dflt) { const long v = gt_switch(GT_SW_XCHG_SPIN_MAX); return v > 0 ? (int)v : dflt; }
// 0 = off, 1 = on where it applies (the default), 2 = forced (gt_set_ln_exchange(1) / GT_LN_XCHG=1: no lower bound on the tile count -- tests)
static int ln_xchg_mode() { const long v = gt_switch(GT_SW_LN_XCHG); return v < 0 ? 1 : v ? 2 : 0; }
static bool ln_xchg(const Ctx& x) { return ln_xchg_mode() != 0 && !(x.c.flags & GT_CFG_NO_LN_XCHG) && x.W.rowx >= 0; }
static void ln_xchg_args(const Ctx& x, GemmArgs& g) {
  g.rowx = reinterpret_cast<unsigned*>(x.ws + x.W.rowx);
  g.spin_max = xchg_spin_max(GT_ROWX_SPIN_MAX);
}
// which geometry the row exchange runs on for this (M, N): 64 = the 64x64 kernels of gt_gemm64.h, 128 = the big tile (round 6), 0 = none
static int ln_xchg_tile(const GemmArgs& g) {
  if (gemm64_ln_shape(g, xchg_cus(), ln_xchg_mode() == 2)) return 64;
  if (gt_switch(GT_SW_LN_XCHG128) && gemm32_ln_shape(g, xchg_cus())) return 128;     // (A/B switches)
  return (gt_switch(GT_SW_LN_XCHG32) && gemm_xln32_shape(g, xchg_cus())) ? 32 : 0;
}
// Which kernel takes the Linear / dgrad g with the LayerNorm (EPI_RES_LN) / its backward (EPI_RES_LNBWD) in its epilogue: the ONE statement of that rule
// (linear_res_ln and dgrad_lnbwd pick, then run).  H: bf16-source, both operand shadows; else fp32-source -- not for a bf16-ONLY input (in_only16).
enum LnXchgKind { LX_NONE, LX_128H, LX_128, LX_32, LX_64H, LX_64 };
static int ln_xchg_rows(LnXchgKind k) { return k == LX_NONE ? 0 : k == LX_32 ? 32 : k <= LX_128 ? 128 : 64; }
static LnXchgKind ln_xchg_pick(const GemmArgs& g, int epi, bool bkm, bool in_only16) {
  const int tile = ln_xchg_tile(g);
  const bool both16 = g.bf16 && g.A16 && g.B16;
  if (tile == 128) {
    if (!gemm32_ln_ok(g, epi)) return LX_NONE;
    if (both16 && gemm32h_ok(g, epi)) return LX_128H;
    return (!in_only16 && !both16 && gemm32_ok(g, epi, bkm)) ? LX_128 : LX_NONE;
  }
  if (tile == 32) return (!in_only16 && gemm_xln32_ok(g, epi == EPI_RES_LN ? EPI_RES_LN_X : EPI_RES_LNBWD_X)) ? LX_32 : LX_NONE;
  if (tile != 64) return LX_NONE;
  if (both16 && gemm64h_ok(g, epi)) return LX_64H;
  return (!in_only16 && !both16 && gemm64_ok(g, epi)) ? LX_64 : LX_NONE;
}
template <bool BKM, int EPI>
static void ln_xchg_run(const Ctx& x, const GemmArgs& g, LnXchgKind k) {
  switch (k) {
    case LX_128H: gemm64_trace("ln128 bf16-source", g, false, EPI); gemm32h_launch<false, EPI>(g, x.s); break;
    case LX_128:  gemm64_trace("ln128 fp32-source", g, BKM, EPI); gemm32_launch<BKM, EPI>(g, x.s); break;
    case LX_32: {
      // the generic kernel's 32x32 tiles (the d_model-256 YAMLs at 512 ... 2048 tokens): fp32 sources; precision 1 rounds them on their way into LDS
      constexpr int EPIX = EPI == EPI_RES_LN ? EPI_RES_LN_X : EPI_RES_LNBWD_X;
      GemmArgs f = g;
      f.k_chunk = (f.K + 63) / 64 * 64;
      gemm64_trace("ln32 fp32-source", f, BKM, EPI);
      if (f.bf16) gemm_launch_cfg<2, 2, 1, 1, 64, false, BKM, EPIX, 1>(f, 1, x.s);
      else        gemm_launch_cfg<2, 2, 1, 1, 64, false, BKM, EPIX>(f, 1, x.s);
      break;
    }
    case LX_64H:  gemm64h_launch<false, EPI>(g, x.s); break;
    case LX_64:   gemm64_launch<BKM, EPI>(g, x.s); break;
    case LX_NONE: break;
  }
}
// does the row exchange take this shape's d_model-wide Linears?  (the shape rule of gemm64_ln_shape for N = d_model)
static bool ln_xchg_rows(const Ctx& x) {
  if (!ln_xchg(x) || x.M % 64 != 0) return false;
  GemmArgs g{};
  g.M = x.M; g.N = x.d;
  return ln_xchg_tile(g) != 0;
}
// Round 5: where the row exchange applies the 64x64 ring tiles + the norm in their epilogue beat the row-owning tiles too (d_model 256 at 8192 tokens,
// C3: 5.20 ms with the row-owning tiles, 5.06 with 64x64 tiles + exchange -- 5.29 with 64x64 tiles and the norm as a row pass); GT_LN_XCHG=0
// keeps the row-owning tiles
static bool row_fused(const Ctx& x) {
  if (x.c.precision) return false;
  if (x.d <= GT_ROW_FUSE_MAX_D) return true;
  return x.M >= GT_ROW_FUSE_MIN_M && x.d <= GT_ROW_FUSE_BIG_MAX_D && !ln_xchg_rows(x);
}
static void ln_bwd(const Ctx& x, const float* dy, const float* res, const float* xhat, const float* rstd, int64_t gamma_off, float* dz,
                   float* dzm, int site, const uint16_t* dy16 = nullptr);
static int dgrad_lnbwd(const Ctx& x, const float* dY, int ldy, const float* W, int K, const float* res, const float* xhat,
                       const float* rstd, int64_t gamma_off, float* dz, float* dzm, int site) {
  if (!row_fused(x)) {
    if (ln_xchg(x) && x.ln && x.ln->n < GT_LN_JOBS_MAX) {
      // ONE launch: the dgrad on 64x64 tiles, the LayerNorm backward in its epilogue (row sums through the in-launch exchange)
      const float* wt = wT_of(x, W);                            // (precision 1 without shadows: the NT form over the fp32 transpose)
      GemmArgs g = wt ? mk_gemm(x, dY, ldy, wt, K, dz, x.d, x.M, x.d, K) : mk_gemm(x, dY, ldy, W, x.d, dz, x.d, x.M, x.d, K);
      if (!wt && ldy == K) { g.A16 = sh_act(x, dY); g.B16 = sh_w(x, W, true); g.lda16 = g.ldb16 = K; }
      g.as_dgrad = 1;
      g.res = res; g.ldres = x.d; g.xhat = xhat; g.rstd = rstd; g.gamma = x.prm + gamma_off;
      g.C2 = (x.drop && !only16(x, dzm)) ? dzm : nullptr;
      g.C16 = sh_act(x, x.drop ? dzm : dz); g.ldc16 = x.d;
      g.drop = mk_drop(x, site);
      float dummy; g.ln_part = &dummy;                          // (pick first: a registered job cannot be taken back)
      ln_xchg_args(x, g);
      const LnXchgKind k = ln_xchg_pick(g, EPI_RES_LNBWD, wt == nullptr, only16(x, dY));
      if (k != LX_NONE) {
        g.ln_part = ln_job(x, gamma_off, x.M / ln_xchg_rows(k));
        if (wt) ln_xchg_run<false, EPI_RES_LNBWD>(x, g, k);
        else    ln_xchg_run<true, EPI_RES_LNBWD>(x, g, k);
        return 0;
      }
    }
    // precision = 2: the dgrad output lives in bf16 alone -- in the region that receives the bf16 copy of the norm's result (in place)
    uint16_t* t16 = (p2(x.c) && (x.d == 256 || x.d == 512) && x.ln && x.ln->n < GT_LN_JOBS_MAX) ? sh_act(x, x.drop ? dzm : dz) : nullptr;
    dgrad_store(x, dY, ldy, W, x.d, dz, x.d, K, 0, t16);
    ln_bwd(x, dz, res, xhat, rstd, gamma_off, dz, dzm, site, t16);
    return 0;
  }
  GemmArgs g = mk_gemm(x, dY, ldy, W, x.d, dz, x.d, x.M, x.d, K);
  g.res = res; g.ldres = x.d;
  g.xhat = xhat; g.rstd = rstd; g.gamma = x.prm + gamma_off;
  g.dgamma = x.grd + gamma_off; g.dbeta = x.grd + gamma_off + (x.d + 63) / 64 * 64;   // bias tensor follows the weight
  g.C2 = x.drop ? dzm : nullptr;
  g.drop = mk_drop(x, site);
  const int bm = gemm_row_rows(g, true);
  g.ln_part = ln_job(x, gamma_off, (x.M + bm - 1) / bm);
  return gemm_launch_row<false, true, EPI_RES_LNBWD>(g, x.s);
}
// dz = LNbwd(dy (+ res)); dzm = dz * dropout mask.  Few tokens: 2 rows per wave (one wave per CU cannot hide its own load
// latency); many: 8 rows per wave, fewer partials to sum.
static void ln_bwd(const Ctx& x, const float* dy, const float* res, const float* xhat, const float* rstd, int64_t gamma_off, float* dz,
                   float* dzm, int site, const uint16_t* dy16) {
  const int rpw = x.M <= 4096 ? 2 : GT_LNB_ROWS;
  const int rows_per_block = 4 * rpw;
  const int nblk = (x.M + rows_per_block - 1) / rows_per_block;
  float* part = ln_job(x, gamma_off, nblk);
  gt_prof_tag("ln_bwd", 0, (res ? 16.0 : 12.0) * x.M * x.d);
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (part != nullptr && (x.d == 256 || x.d == 512) && al16(dy) && al16(xhat) && al16(dz) && (!res || al16(res)) && (!x.drop || al16(dzm))) {
    uint16_t* dzm16 = sh_act(x, x.drop ? dzm : dz);
    float* dzm32 = (x.drop && !only16(x, dzm)) ? dzm : (float*)nullptr;          // (level 2: the masked copy lives in bf16 alone)
    gt_dispatch("ln_bwd variant v4 M %d d %d rpw %d in16 %d", x.M, x.d, rpw, dy16 != nullptr);
    if (x.d == 512) gt_launch(ln_bwd_v4_kernel<2>, dim3(nblk), dim3(256), x.s, dy, res, xhat, rstd, x.prm + gamma_off, dz,
                              dzm32, mk_drop(x, site), part, x.M, rpw, dzm16, dy16);
    else gt_launch(ln_bwd_v4_kernel<1>, dim3(nblk), dim3(256), x.s, dy, res, xhat, rstd, x.prm + gamma_off, dz,
                   dzm32, mk_drop(x, site), part, x.M, rpw, dzm16, dy16);
    return;
  }
  need16(x, dy16 == nullptr, "LayerNorm backward of a bf16-only gradient (precision 2)");
  gt_dispatch("ln_bwd variant generic M %d d %d rpw %d in16 0", x.M, x.d, rpw);
  gt_launch(ln_bwd_kernel, dim3(nblk), dim3(256), x.s, dy, res, xhat, rstd,
            x.prm + gamma_off, dz, (x.drop && !only16(x, dzm)) ? dzm : (float*)nullptr, mk_drop(x, site), x.grd + gamma_off,
            x.grd + gamma_off + (x.d + 63) / 64 * 64, part, x.M, x.d, rpw, sh_act(x, x.drop ? dzm : dz));
}
// dz = LNbwd_inner(LNbwd_outer(dy)): the final encoder / decoder norm (outer) and the top layer's last norm (inner) sit back
// to back; one pass over the rows instead of two launches.  Falls back to two passes when the partials table is full.
static void ln_bwd2(const Ctx& x, const float* dy, const float* xhat_o, const float* rstd_o, int64_t gamma_o, float* mid,
                    const float* xhat_i, const float* rstd_i, int64_t gamma_i, float* dz, float* dzm, int site) {
  const int rpw = x.M <= 4096 ? 2 : GT_LNB_ROWS;
  const int nblk = (x.M + 4 * rpw - 1) / (4 * rpw);
  float* part_o = (x.ln && x.ln->n + 2 <= GT_LN_JOBS_MAX) ? ln_job(x, gamma_o, nblk) : nullptr;
  float* part_i = part_o ? ln_job(x, gamma_i, nblk) : nullptr;
  if (!part_o || !part_i) {
    ln_bwd(x, dy, nullptr, xhat_o, rstd_o, gamma_o, mid, nullptr, 0);
    ln_bwd(x, mid, nullptr, xhat_i, rstd_i, gamma_i, dz, dzm, site);
    return;
  }
  gt_prof_tag("ln_bwd", 0, 20.0 * x.M * x.d);
  gt_dispatch("ln_bwd variant two_norms M %d d %d rpw %d in16 0", x.M, x.d, rpw);
  gt_launch(ln_bwd2_kernel, dim3(nblk), dim3(256), x.s, dy, xhat_o, rstd_o, (const float*)(x.prm + gamma_o), part_o, xhat_i, rstd_i,
            (const float*)(x.prm + gamma_i), part_i, dz, (x.drop && !only16(x, dzm)) ? dzm : (float*)nullptr, mk_drop(x, site), x.M, x.d, rpw,
            sh_act(x, x.drop ? dzm : dz));
}
// second norm applied right after linear_res_ln's (the final encoder / decoder norm after the last layer)
struct SecondNorm { int64_t gamma_off; float* y; float* xhat; float* rstd; };
// The LayerNorm-forward row pass behind a Linear: n.y = LN_n(drop(in) + res) [; second->y = LN_second(n.y)]; in16 (precision 2): where the rows
// live in bf16 alone.  res == nullptr: a plain norm (the one after a row-fused first).  y16: bf16 copy of n.y (one norm only).
static void ln_fwd_rows(const Ctx& x, const float* in, const uint16_t* in16, const float* res, const DropArgs& da, const SecondNorm& n,
                        uint16_t* y16, const SecondNorm* second) {
  const int64_t bo = (x.d + 63) / 64 * 64;          // a norm's bias tensor follows its weight
  const float* gm = x.prm + n.gamma_off;
  gt_prof_tag("ln_fwd", 0, ((second ? 24.0 : res ? 16.0 : 12.0) - (in16 ? 2.0 : 0.0)) * x.M * x.d);
  gt_dispatch("ln_fwd variant %s M %d d %d in16 %d", second ? "two_norms" : "one_norm", x.M, x.d, in16 != nullptr);
  if (second) {
    const float* gm2 = x.prm + second->gamma_off;
    gt_launch(ln_fwd2_kernel, dim3((x.M + 3) / 4), dim3(256), x.s, in, res, da, gm, gm + bo, n.y, n.xhat, n.rstd, gm2, gm2 + bo,
              second->y, second->xhat, second->rstd, x.M, x.d, in16);
  } else {
    gt_launch(ln_fwd_kernel, dim3((x.M + 3) / 4), dim3(256), x.s, in, res, da, gm, gm + bo, n.y, n.xhat, n.rstd, x.M, x.d, x.d, x.d, x.d,
              y16, in16);
  }
}
// x_out = LN(drop(in W^T + b) + res)   [; second->y = LN_second(x_out)]
static int linear_res_ln(const Ctx& x, const float* in, int K, int64_t w_off, int64_t b_off, const float* res, int64_t gamma_off,
                         float* out, float* xhat, float* rstd, int site, const SecondNorm* second = nullptr) {
  GemmArgs g = mk_gemm(x, in, K, x.prm + w_off, K, out, x.d, x.M, x.d, K);
  g.bias = x.prm + b_off;
  const int64_t bo = (x.d + 63) / 64 * 64;          // a norm's bias tensor follows its weight
  if (!row_fused(x)) {
    g.A16 = sh_act(x, in); g.B16 = sh_w(x, x.prm + w_off, false); g.lda16 = g.ldb16 = K;
    if (only16(x, in)) need16(x, g.A16 && g.B16 && gemm32h_ok(g, EPI_STORE), "Linear (+ LayerNorm) of a bf16-only tensor");
    // precision = 2: the Linear output ahead of the norm lives in bf16 alone -- in the region that then receives the bf16 copy of the norm's
    // result (the row pass reads a row into registers before it writes any of it)
    uint16_t* t16 = p2(x.c) ? sh_act(x, out) : nullptr;
    // ONE launch: the Linear with dropout + residual + LayerNorm in its epilogue (row statistics through the in-launch exchange: 64x64 tiles at
    // a GPU's share of a data-parallel batch, the big tile from 8192 tokens at d_model 512 -- round 6)
    // (precision 2 fuses on the big tile only: the pre-norm output never leaves the registers -- rounded to bf16 there, round16: the numbers of
    //  the bf16-stored form without its round trip.  At 2048 tokens the stored form + row pass stays: measured 0.866 / 0.867 ms against
    //  0.870 / 0.870 fused (profiles/r06_ab_p2_fused_forward.txt))
    if ((t16 == nullptr || ln_xchg_tile(g) == 128) && !second && ln_xchg(x)) {
      GemmArgs f = g;
      f.res = res; f.ldres = x.d; f.gamma = x.prm + gamma_off; f.beta = x.prm + gamma_off + bo;
      f.aux = xhat; f.aux2 = rstd; f.drop = mk_drop(x, site);
      f.C16 = sh_act(x, out); f.ldc16 = x.d;
      f.round16 = t16 != nullptr;
      ln_xchg_args(x, f);
      const LnXchgKind k = ln_xchg_pick(f, EPI_RES_LN, false, only16(x, in));
      if (k != LX_NONE) { ln_xchg_run<false, EPI_RES_LN>(x, f, k); return 0; }
    }
    if (t16 != nullptr) {
      g.C = nullptr; g.C16 = t16; g.ldc16 = x.d;
      need16(x, gemm_on_big_kernel<false, EPI_STORE>(g), "Linear (+ LayerNorm) with a bf16-only output (precision 2)");
    }
    gemm_launch<false, false, EPI_STORE>(g, x.s);
    const SecondNorm first = {gamma_off, out, xhat, rstd};
    ln_fwd_rows(x, out, t16, res, mk_drop(x, site), first, sh_act(x, out), second);
    return 0;
  }
  g.res = res; g.ldres = x.d;
  g.gamma = x.prm + gamma_off; g.beta = x.prm + gamma_off + bo;
  g.aux = xhat; g.aux2 = rstd;
  g.drop = mk_drop(x, site);
  if (gemm_launch_row<false, false, EPI_RES_LN>(g, x.s)) return -1;
  // fused row tile for the first norm: the second one is its own pass
  if (second) ln_fwd_rows(x, out, nullptr, nullptr, no_drop(), *second, nullptr, nullptr);
  return 0;
}
// head dims served by the MFMA attention kernels (0: use the generic LDS/VALU kernels)
static int attn_mfma_hd(const Ctx& x) {
  const int hd = x.d / x.H;
  if (hd == 16 || hd == 32 || hd == 64 || hd == 128) return hd;
  return hd < 16 ? -16 : 0;                         // -16: the 16-wide kernels with zero-padded operands (head_dim 1..15)
}
// Attention backward with fewer (sequence, head) pairs than CUs and head_dim 64 / 128 (the reference's d_model-256 YAMLs: 2 heads of 128,
// batch 32 = 64 pairs): the LDS-staged kernel with four wave pairs per (sequence, head) -- each repeats the dP contraction of its tile from
// LDS and takes a quarter of the head's column tiles (gt_attn.h, CS).  10.5 -> 10.0 us per launch at 64 pairs: the stage is a latency
// floor (launch, cold operands, three barriers), not a parallelism problem -- the same split on the register-fragment kernels, forward
// and backward, was SLOWER (5.8 -> 8.4 / 10.5 -> 16.1 us: every wave repeats the contraction's loads; tools/rejected/README.md).
#ifndef GT_ATTN_CS_MAX_PAIRS
#define GT_ATTN_CS_MAX_PAIRS 256
#endif
static bool attn_col_split(const Ctx& x, int pairs) {
  const int hd = attn_mfma_hd(x);
  return (hd == 64 || hd == 128) && pairs < GT_ATTN_CS_MAX_PAIRS;
}
// in16 (precision = 2): q / k / v are bf16 tensors at the same ELEMENT offsets (the qkv buffer holds bf16 in its first half)
static void attention_fwd(const Ctx& x, const float* q, int ldq, const float* k, const float* v, int ldkv, float* P, float* ctx,
                          int causal, int site, bool in16 = false) {
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldk = ldkv; a.ldv = ldkv; a.P = P; a.ctx = ctx; a.ldc = x.d;
  a.H = x.H; a.hd = x.hd; a.scale = 1.0f / sqrtf((float)x.hd); a.causal = causal; a.drop = mk_drop(x, site);
  a.ctx16 = attn_mfma_hd(x) > 0 ? sh_act(x, ctx) : nullptr;
  if (only16(x, ctx)) { need16(x, a.ctx16 != nullptr, "attention output stored in bf16 alone"); if (a.ctx16) a.ctx = nullptr; }
  gt_prof_tag("attn_fwd", 4.0 * x.M * 32 * x.d, 4.0 * (4.0 * x.M * x.d + 1024.0 * x.c.batch * x.H));
  const dim3 grid(x.c.batch * x.H);
  if (in16) {
    a.q16 = reinterpret_cast<const uint16_t*>(q); a.k16 = a.q16 + (k - q); a.v16 = a.q16 + (v - q);
    a.q = a.k = a.v = nullptr;
    need16(x, ((ldq | ldkv) & 3) == 0 && (attn_mfma_hd(x) == 64 || attn_mfma_hd(x) == 128), "attention over bf16-stored q / k / v (precision 2)");
    gt_dispatch("attn_fwd kernel lds%d-bf16 pairs %u", attn_mfma_hd(x), grid.x);
    if (attn_mfma_hd(x) == 128) gt_launch(attn_fwd_lds_kernel<128, true>, grid, dim3(128), x.s, a);
    else gt_launch(attn_fwd_lds_kernel<64, true>, grid, dim3(128), x.s, a);
    return;
  }
  if (attn_mfma_hd(x) == 0) gt_dispatch("attn_fwd kernel generic pairs %u", grid.x);
  else gt_dispatch("attn_fwd kernel mfma%d%s pairs %u", attn_mfma_hd(x) < 0 ? 16 : attn_mfma_hd(x), attn_mfma_hd(x) < 0 ? "-padded" : "", grid.x);
  switch (attn_mfma_hd(x)) {
    case 16:  gt_launch(attn_fwd_mfma_kernel<16, false>, grid, dim3(128), x.s, a); break;
    case 32:  gt_launch(attn_fwd_mfma_kernel<32, false>, grid, dim3(128), x.s, a); break;
    case 64:  gt_launch(attn_fwd_mfma_kernel<64, false>, grid, dim3(128), x.s, a); break;
    case 128: gt_launch(attn_fwd_mfma_kernel<128, false>, grid, dim3(128), x.s, a); break;
    case -16: gt_launch(attn_fwd_mfma_kernel<16, true>, grid, dim3(128), x.s, a); break;
    default:  gt_launch(attn_fwd_kernel, grid, dim3(256), x.s, a);
  }
}
#ifndef GT_ATTN_BWD_LDS_MIN
#define GT_ATTN_BWD_LDS_MIN 1024       // (sequence, head) pairs from which attention backward stages its operands in LDS
#endif
static void attention_bwd(const Ctx& x, const float* q, int ldq, const float* k, const float* v, int ldkv, const float* P,
                          const float* dctx, float* dq, int lddq, float* dk, float* dv, int lddkv, int site, bool in16 = false) {
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldk = ldkv; a.ldv = ldkv; a.P = const_cast<float*>(P);
  a.H = x.H; a.hd = x.hd; a.scale = 1.0f / sqrtf((float)x.hd); a.drop = mk_drop(x, site);
  a.dctx = dctx; a.lddc = x.d; a.dq = dq; a.dk = dk; a.dv = dv; a.lddq = lddq; a.lddk = lddkv; a.lddv = lddkv;
  if (attn_mfma_hd(x) > 0 && dk == dq + x.d && dv == dq + 2 * x.d && lddq == 3 * x.d && lddkv == 3 * x.d) a.dqkv16 = sh_act(x, dq);
  if (only16(x, dq)) { need16(x, a.dqkv16 != nullptr, "attention gradients stored in bf16 alone"); if (a.dqkv16) { a.dq = nullptr; a.dk = nullptr; a.dv = nullptr; } }
  gt_prof_tag("attn_bwd", 10.0 * x.M * 32 * x.d, 4.0 * (7.0 * x.M * x.d + 1024.0 * x.c.batch * x.H));
  const dim3 grid(x.c.batch * x.H);
  // head_dim 64 with the chip full: the LDS-staged form (every operand byte requested once, 16 bytes at a time)
  const int lds_min = (int)gt_switch(GT_SW_ATTN_BWD_LDS_MIN, GT_ATTN_BWD_LDS_MIN);
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (in16) {                                        // precision = 2: q / k / v / dctx stored in bf16 alone, widened on their way into LDS
    a.q16 = reinterpret_cast<const uint16_t*>(q); a.k16 = a.q16 + (k - q); a.v16 = a.q16 + (v - q); a.dctx16 = reinterpret_cast<const uint16_t*>(dctx);
    a.q = a.k = a.v = nullptr; a.dctx = nullptr;
    need16(x, ((ldq | ldkv | lddq | lddkv | x.d) & 3) == 0 && (attn_mfma_hd(x) == 64 || attn_mfma_hd(x) == 128), "attention backward over bf16-stored operands (precision 2)");
    gt_dispatch("attn_bwd kernel lds%dx%d-bf16 pairs %u", attn_mfma_hd(x), (attn_mfma_hd(x) == 128 || (int)grid.x < GT_ATTN_CS_MAX_PAIRS) ? 4 : 1, grid.x);
    if (attn_mfma_hd(x) == 128) gt_launch(attn_bwd_lds_kernel<128, 4, true>, grid, dim3(512), x.s, a);
    else if ((int)grid.x < GT_ATTN_CS_MAX_PAIRS) gt_launch(attn_bwd_lds_kernel<64, 4, true>, grid, dim3(512), x.s, a);
    else gt_launch(attn_bwd_lds_kernel<64, 1, true>, grid, dim3(128), x.s, a);
    return;
  }
  const bool lds_ok = ((ldq | ldkv | lddq | lddkv | x.d) & 3) == 0 && al16(q) && al16(k) && al16(v) && al16(dctx) && al16(dq) && al16(dk) && al16(dv);
  if (attn_mfma_hd(x) == 64 && (int)grid.x >= lds_min && lds_ok) {
    gt_dispatch("attn_bwd kernel lds64x1 pairs %u", grid.x);
    gt_launch(attn_bwd_lds_kernel<64>, grid, dim3(128), x.s, a);
    return;
  }
  if (attn_col_split(x, (int)grid.x) && lds_ok) {     // few pairs, wide heads: LDS-staged operands, four wave pairs per pair
    gt_dispatch("attn_bwd kernel lds%dx4 pairs %u", attn_mfma_hd(x), grid.x);
    if (attn_mfma_hd(x) == 128) gt_launch(attn_bwd_lds_kernel<128, 4>, grid, dim3(512), x.s, a);
    else gt_launch(attn_bwd_lds_kernel<64, 4>, grid, dim3(512), x.s, a);
    return;
  }
  if (attn_mfma_hd(x) == 0) gt_dispatch("attn_bwd kernel generic pairs %u", grid.x);
  else gt_dispatch("attn_bwd kernel mfma%d%s pairs %u", attn_mfma_hd(x) < 0 ? 16 : attn_mfma_hd(x), attn_mfma_hd(x) < 0 ? "-padded" : "", grid.x);
  switch (attn_mfma_hd(x)) {
    case 16:  gt_launch(attn_bwd_mfma_kernel<16, false>, grid, dim3(128), x.s, a); break;
    case 32:  gt_launch(attn_bwd_mfma_kernel<32, false>, grid, dim3(128), x.s, a); break;
    case 64:  gt_launch(attn_bwd_mfma_kernel<64, false>, grid, dim3(128), x.s, a); break;
    case 128: gt_launch(attn_bwd_mfma_kernel<128, false>, grid, dim3(128), x.s, a); break;
    case -16: gt_launch(attn_bwd_mfma_kernel<16, true>, grid, dim3(128), x.s, a); break;
    default:  gt_launch(attn_bwd_kernel, grid, dim3(256), x.s, a);
  }
}

static int make_ctx(Ctx& x, const gt_config* cfg, const float* params, float* grads, float* ws, const gt_step_state* st,
                    int train, gt_stream_t stream) {
  if (check_cfg(cfg)) return -1;
  if (!params || !ws) return gt_fail("params / ws must not be NULL");
  x.c = *cfg;
  x.plan = SeqPlan{};
  x.P = param_layout(*cfg);
  x.W = ws_layout(*cfg);
  x.M = cfg->batch * 32; x.d = cfg->d_model; x.F = cfg->dim_ff; x.H = cfg->n_heads; x.hd = x.d / x.H;
  x.prm = params; x.grd = grads; x.ws = ws; x.st = st;
  x.drop = train && st != nullptr && cfg->dropout > 0.f;
  x.s = (hipStream_t)stream;
  x.wb = nullptr;
  x.ln = nullptr;
  x.refused = nullptr;
  return 0;
}
static int launch_status(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return gt_fail("%s: HIP launch error: %s", what, hipGetErrorString(e));
  return 0;
}
static int launch_status(const Ctx& x, const char* what) {      // ... of a call with a context: what need16 recorded comes first
  if (x.refused != nullptr) return gt_fail("%s: %s has no bf16-source kernel for this shape (gt_set_operand_shadows(1) keeps the fp32 copies)", what, x.refused);
  return launch_status(what);
}

// ------------------------------------------------------------------------------------ forward
// InputLayer: Linear -> ReLU -> + pe[t] -> dropout        
static void input_layer_fwd(const Ctx& x, const float* in, int S, int64_t w, int64_t b, const float* pe, float* a0, float* out,
                            int site) {
  GemmArgs g = mk_gemm(x, in, S, x.prm + w, S, out, x.d, x.M, x.d, S);
  g.bias = x.prm + b; g.aux = a0; g.pe = pe; g.drop = mk_drop(x, site);
  g.C16 = sh_act(x, out); g.ldc16 = x.d;           // (bf16 shadow of x0 where the encoder's operands have them: written by the generic kernel's EPI_RELU_PE epilogue)
  gemm_launch<false, false, EPI_RELU_PE>(g, x.s);
}
// FFN block + last norm of a layer:  xout = LN(xin + drop(W2 drop(relu(W1 xin + b1)) + b2))
// The two launches around the FFN activation, as their argument blocks: FFN1 (hact = drop(relu(xin W1^T + b1))) and the FFN2 dgrad
// (dhid = (dzm W2) * [hact != 0] / (1 - p)).  `ok`: false when a tensor stored in bf16 alone meets a kernel that cannot take it (need16).
static GemmArgs ffn1_args(const Ctx& x, const LayerP& p, const LayerW& w, const float* xin, int gl, bool* ok) {
  float* ws = x.ws;
  GemmArgs g = mk_gemm(x, xin, x.d, x.prm + p.w1, x.d, ws + w.hact, x.F, x.M, x.F, x.d);
  g.bias = x.prm + p.b1; g.drop = mk_drop(x, lsite(gl, GT_SITE_FFN));
  g.A16 = sh_act(x, xin); g.B16 = sh_w(x, x.prm + p.w1, false); g.lda16 = g.ldb16 = x.d;
  if (g.A16 && g.B16) { g.C16 = sh_act(x, ws + w.hact); g.ldc16 = x.F; }      // (written by the bf16-source kernel's epilogue only)
  *ok = true;
  if (only16(x, ws + w.hact)) { *ok = g.C16 && gemm32h_ok(g, EPI_RELU_DROP); if (g.C16) g.C = nullptr; }
  return g;
}
// (*nt: the product runs in its NT form on a transposed fp32 copy of W2 -- precision 1 without shadows)
static GemmArgs ffn2d_args(const Ctx& x, const LayerP& p, const LayerW& w, const Tmp& t, const float* dzm, bool* nt, bool* ok) {
  float* ws = x.ws;
  const float* w2t = wT_of(x, x.prm + p.w2);
  GemmArgs g = w2t ? mk_gemm(x, dzm, x.d, w2t, x.d, t.dhid, x.F, x.M, x.F, x.d) : mk_gemm(x, dzm, x.d, x.prm + p.w2, x.F, t.dhid, x.F, x.M, x.F, x.d);
  g.res = ws + w.hact; g.ldres = x.F;
  g.mask_scale = x.drop ? 1.0f / (1.0f - x.c.dropout) : 1.0f;
  *nt = w2t != nullptr; *ok = true;
  if (w2t) return g;
  g.A16 = sh_act(x, dzm); g.B16 = sh_w(x, x.prm + p.w2, true); g.lda16 = g.ldb16 = x.d;
  if (g.A16 && g.B16) { g.C16 = sh_act(x, t.dhid); g.ldc16 = x.F; }
  if (only16(x, ws + w.hact)) g.res16 = sh_act(x, ws + w.hact);
  if (only16(x, t.dhid) || only16(x, dzm) || g.res16) {
    *ok = g.C16 && gemm32h_ok(g, EPI_MASK_NZ);
    if (g.C16 && only16(x, t.dhid)) g.C = nullptr;
  }
  return g;
}
// Keep bits of layer gl's FFN activation (round 6): FFN1's epilogue leaves one bit per element of hact -- kept by the dropout AND positive --
// and the FFN2 dgrad reads those instead of hact itself (32 x / 16 x fewer bytes: C5 bs 512 3.15 -> 3.10 ms).  Only the ring-tile kernels
// write / read them (gemm32_store_epilogue), so BOTH launches must be on one: decided here, from the two argument blocks, for the
// forward and the backward alike.  GT_FFN_KBITS=0: off.
static uint16_t* ffn_kbits(const Ctx& x, const LayerP& p, const LayerW& w, const float* xin, int gl) {
  if (!gt_switch(GT_SW_FFN_KBITS) || x.W.kbits < 0 || x.M % 32 != 0) return nullptr;
  bool ok1, ok2, nt;
  const GemmArgs a = ffn1_args(x, p, w, xin, gl, &ok1);
  const Tmp t = tmp_set(x, gl);
  const GemmArgs b = ffn2d_args(x, p, w, t, t.dzAm, &nt, &ok2);
  if (!ok1 || !ok2 || !gemm_on_big_kernel<false, EPI_RELU_DROP>(a)) return nullptr;
  if (!(nt ? gemm_on_big_kernel<false, EPI_MASK_NZ>(b) : gemm_on_big_kernel<true, EPI_MASK_NZ>(b))) return nullptr;
  return reinterpret_cast<uint16_t*>(x.ws + x.W.kbits + x.W.kbits_stride * gl);
}
static int ffn_fwd(const Ctx& x, const LayerP& p, const LayerW& w, const float* xin, int64_t norm_w, int gl,
                   const SecondNorm* second = nullptr) {
  float* ws = x.ws;
  bool ok;
  GemmArgs g = ffn1_args(x, p, w, xin, gl, &ok);
  need16(x, ok, "FFN activation stored in bf16 alone");
  g.kbits = ffn_kbits(x, p, w, xin, gl);
  if (g.kbits) gemm64_trace("kbits write", g, false, EPI_RELU_DROP);
  gemm_launch<false, false, EPI_RELU_DROP>(g, x.s);
  return linear_res_ln(x, ws + w.hact, x.F, p.w2, p.b2, xin, norm_w, ws + w.xout, ws + w.xhat2, ws + w.rstd2,
                       lsite(gl, GT_SITE_DROPF), second);
}
static int self_attn_fwd(const Ctx& x, const LayerP& p, const LayerW& w, const float* xin, int causal, int gl) {
  float* ws = x.ws;
  const int d = x.d;
  const bool s16 = p2(x.c) && gl < x.c.n_enc_layers;          // precision = 2: qkv in bf16 alone (the first half of its buffer)
  linear_fwd(x, xin, d, x.prm + p.sa.in_w, x.prm + p.sa.in_b, ws + w.qkv, 3 * d, 3 * d, d, s16 ? reinterpret_cast<uint16_t*>(ws + w.qkv) : nullptr);
  attention_fwd(x, ws + w.qkv, 3 * d, ws + w.qkv + d, ws + w.qkv + 2 * d, 3 * d, ws + w.P, ws + w.ctx, causal,
                lsite(gl, GT_SITE_ATTN), s16);
  return linear_res_ln(x, ws + w.ctx, d, p.sa.out_w, p.sa.out_b, xin, p.n1w, ws + w.x1, ws + w.xhat1, ws + w.rstd1,
                       lsite(gl, GT_SITE_DROP1));
}

// ---- sequence-resident kernels (gt_seq.h): one workgroup per sequence walks the whole encoder -------------------------------
// GT_SW_SEQ: 0 = off (GT_SEQ=0 / gt_set_seq(0)), 1 = every supported shape (GT_SEQ=1 / gt_set_seq(1): tests), unset = by measurement (default):
// always at d_model <= 64 (C1 1.9x, ClosedHH YAML 1.15x over one kernel per op) and at d_model 128 (two workgroups per sequence
// while they fit the chip: bs 16 1.11x, 64 1.18x, 128 1.36x; one per sequence beyond: bs 192 1.53x); at the other widths of the
// 128 class a sequence's matmuls are bound by the fp32 MFMA rate of the ONE CU its workgroup runs on: from 64 sequences per GPU up.
extern "C" int gt_set_seq(int on) { return gt_switch_set_flag(GT_SW_SEQ, on); }
// SPLIT mode (d_model 128, and d_model 32 with dim_feedforward >= 256): 2 x batch workgroups of 16 token rows, one launch per layer
// and direction (+1).  Default (-1): when the pairs fit the chip once (2 x batch <= CUs) -- there a sequence per CU leaves most of
// the MFMA rate idle.
extern "C" int gt_set_seq_split(int on) { return gt_switch_set_flag(GT_SW_SEQ_SPLIT, on); }
// CUs of the CURRENT device (the caller's torch device; cached per device ordinal: a process may drive several GPUs)
static int seq_cu_count() {
#ifdef GT_EMU
  return 256;
#else
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cached[dev] == 0) {
    hipDeviceProp_t prop;
    cached[dev] = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
  }
  return cached[dev];
#endif
}
// CUs the in-launch exchanges may count on for CO-RESIDENCY (QUAD pair exchange, LayerNorm row exchange: every partner of a meeting must hold a CU
// at the same time).  multiProcessorCount does not see a CU mask: with HSA_CU_MASK / ROC_GLOBAL_CU_MASK in the environment the answer is "unknown",
// reported as 0 -- the exchange schedules are not chosen at all, instead of timing out into their fallback on the first step (one note on stderr).
static int xchg_cus() {
  static const bool masked = [] {
    const char* a = getenv("HSA_CU_MASK"); const char* b = getenv("ROC_GLOBAL_CU_MASK");
    const bool m = (a && a[0]) || (b && b[0]);
    if (m) fprintf(stderr, "[groove_hip] a CU mask is set (HSA_CU_MASK / ROC_GLOBAL_CU_MASK): the in-launch exchange schedules stay off\n");
    return m;
  }();
  return masked ? 0 : seq_cu_count();
}
static bool seq_split(const gt_config& c) {
  if (c.d_model != 128 && c.d_model != 32 && c.d_model != 64) return false;
  if (const long sw = gt_switch(GT_SW_SEQ_SPLIT); sw >= 0) return sw != 0;
  // d_model 32 / 64 by shape.  With 16 heads (head_dim 2 / 4) ALWAYS: these kernels alone have the vector-ALU attention, which the zero-padded MFMA
  // form of the whole-sequence kernels loses to at every F (round 6: d32 / H16 / F 64 0.222 -> 0.162 ms, F 128 0.232 -> 0.169; the ClosedHH YAML
  // and the reference CLI's default shape -- d64 / H16 / F 256: 0.370 -> 0.260 -- are the wide end of the same family).  Otherwise only where a
  // sequence's FFN is MFMA-issue-bound on its one CU, F >= 256 (round 2: ClosedHH 0.313 -> 0.290; round 6 at d_model 64: 4 heads 0.259 -> 0.232, 1 head
  // at F 512 0.352 -> 0.285): a narrow FFN is a latency chain that more launches only lengthen (testing YAML, F 16: 0.141 -> 0.160; d32 / H4 / F 128:
  // 0.147 -> 0.156)
  if (c.d_model <= 64 && c.dim_ff < 256 && c.n_heads != 16) return false;
  return 2 * c.batch <= seq_cu_count();
}
// Riders (gt_seq_wg.h): the SPLIT backward phases of the d_model-128 kernels carry the weight gradients on the CUs the sequence
// workgroups leave idle.  GT_SW_SEQ_RIDE: -1 = by shape (enough idle CUs that a phase's units get a rider each or nearly), 0 off, 1 on
// wherever the kernels support it (GT_SEQ_RIDE=0/1, gt_set_seq_ride).
extern "C" int gt_set_seq_ride(int on) { return gt_switch_set_flag(GT_SW_SEQ_RIDE, on); }
#ifndef GT_SEQ_RIDE_MIN_IDLE
#define GT_SEQ_RIDE_MIN_IDLE 96      /* batch <= 80: a phase's units find a rider each (bs 96, 64 idle CUs: 0.324 ms riding vs 0.270 grouped) */
#endif
#ifndef GT_SEQ_RIDE_LAST_PCT
#define GT_SEQ_RIDE_LAST_PCT 50
#endif
static bool seq_ride(const gt_config& c) {
  if (c.d_model != 128 || c.dim_ff % 16 != 0) return false;     // (seq_plan asks for a SPLIT schedule only)
  const int ride = (int)gt_switch(GT_SW_SEQ_RIDE), idle = seq_cu_count() - 2 * c.batch;
  if (ride >= 0) return ride != 0 && idle >= 1;
  return idle >= GT_SEQ_RIDE_MIN_IDLE;
}
// QUAD forward (gt_seq.h): four workgroups per sequence -- row halves x column partners that share the FFN through one pair exchange per
// layer -- while ALL of them fit the chip at once (one workgroup per CU: the partners spin on each other).  -1 = by shape, 0 / 1 forced
// (GT_SEQ_QUAD, gt_set_seq_quad; forcing it on still requires the grid to fit).
extern "C" int gt_set_seq_quad(int on) { return gt_switch_set_flag(GT_SW_SEQ_QUAD, on); }
static bool seq_quad(const gt_config& c) {
  if (c.d_model != 128 || c.dim_ff % 32 != 0 || 4 * c.batch > xchg_cus() || (c.flags & GT_CFG_NO_QUAD)) return false;     // (of a SPLIT schedule: seq_plan)
  return gt_switch(GT_SW_SEQ_QUAD) != 0;
}
// bound of the pair exchange's polling loop (0 / negative: the compiled default).  A test lowers it to see the time-out path -- error
// word, skipped update, host recovery -- without waiting seconds.
extern "C" int gt_set_xchg_spin_max(int polls) { return gt_switch_set(GT_SW_XCHG_SPIN_MAX, polls); }
static bool seq_supported(const gt_config& c) {
  const int hd = c.d_model / c.n_heads;
  return c.n_dec_layers == 0 && c.precision == 0 && c.d_model % 16 == 0 && c.d_model <= 128 && c.dim_ff % 16 == 0 &&
         c.dim_ff <= GT_SEQ_FMAX && c.src_dim <= 32 && (hd < 16 || hd == 16 || hd == 32 || hd == 64);
}
static bool use_seq(const gt_config& c) {
  const long sw = gt_switch(GT_SW_SEQ);
  if (sw < 0 && c.d_model > 64 && c.d_model != 128 && c.batch < 64) return false;   // (by measurement; 128 itself: the SPLIT kernels win from batch 16 up)
  return sw != 0 && seq_supported(c);
}
// The rules above, asked once for a call (a checked gt_config).  Nothing is kept between calls: the process-wide setters and the
// environment answer every time as they always did.
static SeqPlan seq_plan(const gt_config& c) {
  SeqPlan p{};
  p.seq = use_seq(c);
  if (!p.seq) return p;
  const int hd = c.d_model / c.n_heads;
  p.hc = hd < 16 ? 0 : hd;                        // head-dim class (one instantiation each: the attention bodies' registers differ 4x)
  p.split = seq_split(c);
  p.quad = p.split && seq_quad(c);                // four workgroups per sequence: column partners share the FFN
  p.ride = p.split && seq_ride(c);
  // the fused train step's last forward launch goes on into backward phase 0 (seq_fb_kernel): QUAD schedule, riders, head_dim 32
  p.fuse_b0 = p.quad && p.ride && hd == 32;
  return p;
}
// The instantiation a sequence-resident launch of this call's plan runs (gt_seq_kernel_id).  quad: four workgroups per sequence in THIS launch --
// every forward phase of a QUAD plan, of its backward phase 0 alone.  The same id goes to the launcher and into the trace line.
static SeqKernelId seq_kernel(const Ctx& x, bool quad, bool bwd) { return gt_seq_kernel_id(x.d, x.plan.hc, x.plan.split, quad, bwd); }
// The tail of a seq_fwd / seq_bwd trace line, printed from the id the launcher gets: " hc <class> exact <0/1> attn <form> loss <0/1>" at
// GT_TRACE_DISPATCH=2, nothing at 1 -- whoever reads the level-1 trace (its keys are checked one by one by the readers that exist) sees the lines it
// always saw.  attn: "mfma", or for class 0 "valu" / "mfma-pad" (gt_seq_valu_attn); "none" for the QUAD backward launch, whose phase has no attention.
struct SeqInst { char s[64]; };
static SeqInst seq_inst(const Ctx& x, const SeqKernelId& id, bool bwd, bool loss) {
  SeqInst t;
  t.s[0] = 0;
  if (gt_dispatch_level() >= 2) {
    const char* attn = (bwd && id.quad) ? "none" : id.hdc != 0 ? "mfma" : gt_seq_valu_attn(id.split, id.dp, x.hd, x.H) ? "valu" : "mfma-pad";
    snprintf(t.s, sizeof(t.s), " hc %d exact %d attn %s loss %d", id.hdc, (int)id.exact, attn, (int)loss);
  }
  return t;
}
// a launcher's -1: the id names no instantiation of gt_seq_inst.h (nothing seq_supported admits gets here)
static int seq_no_kernel(const char* what, const SeqKernelId& id) {
  return gt_fail("%s: no kernel <%d, %d, %d, %d, %d> is compiled (gt_seq_inst.h)", what, id.dp, id.hdc, (int)id.exact, (int)id.split, (int)id.quad);
}
// What a fused train step hands to its forward and takes back from it (train_step_impl; gt_forward passes none).
struct FwdStep {
  // in: the loss to take along in the launch that runs the output layer (y == nullptr: none), and GT_STEP_PACKS_CURRENT -- the
  // fragment-ordered weight copies in ws are the previous fused update's (seq_update_pack_kernel)
  const float* y; float penalty; float* stats; unsigned* ticket;
  bool packs_current;
  // out
  bool loss_done;            // the sequence-resident launch, or heads_fwd_kernel on the one-kernel-per-op path, computed the loss too
  bool b0_done;              // the last forward launch already ran backward phase 0 (seq_fb_kernel): the step's backward skips it
};
// flops of backward phase 0 of the SPLIT / QUAD schedule: the dgrads of the output layer and of the last layer's FFN2, FFN1, out-proj
static double seq_b0_flops(const Ctx& x) { return 2.0 * x.M * (27.0 * x.d + 2.0 * x.d * x.F + (double)x.d * x.d); }
// launches of one gt_train_step on the sequence-resident path (0: another path -- dozens to hundreds): pack, forward (phases), backward
// (phases), LayerNorm-parameter reduce, grouped weight gradients (one or two tile classes), optimizer.  Hosts use it to choose
// between replaying a captured graph and plain launches: below ~25 nodes the graph's per-node cost exceeds what it saves.
extern "C" int gt_step_launches(const gt_config* cfg) {
  if (check_cfg(cfg)) return -1;
  const SeqPlan sp = seq_plan(*cfg);
  if (!sp.seq) return 0;
  // (with GT_STEP_PACKS_CURRENT one less: no packing launch)
  if (!sp.split) return 7;
  // pack, L forward + L + 1 backward phases (QUAD at head_dim 32: the last forward launch runs backward phase 0 too), [grouped weight gradients x 2,] reduce / tail, update
  return 2 * cfg->n_enc_layers + 1 + (sp.ride ? 3 : 5) - (sp.fuse_b0 ? 1 : 0);
}
static SeqArgs mk_seq(const Ctx& x, const float* pe, const float* src, float* hvo) {
  SeqArgs a;
  memset(&a, 0, sizeof(a));
  a.prm = x.prm; a.ws = x.ws; a.pe = pe; a.xin = src; a.hvo = hvo;
  a.B = x.c.batch; a.S = x.c.src_dim; a.d = x.d; a.F = x.F; a.H = x.H; a.L = x.c.n_enc_layers; a.hd = x.hd;
  a.st = x.drop ? x.st : nullptr; a.thr = x.drop ? (uint32_t)(x.c.dropout * 16777216.0f) : 0u;
  a.dscale = x.drop ? 1.0f / (1.0f - x.c.dropout) : 1.0f;
  const LayerP& p = x.P.enc[0];
  a.p0 = SeqLayerP{p.sa.in_w, p.sa.in_b, p.sa.out_w, p.sa.out_b, p.w1, p.b1, p.w2, p.b2, p.n1w, p.n1b, p.n2w, p.n2b};
  a.pstride = x.c.n_enc_layers > 1 ? x.P.enc[1].sa.in_w - p.sa.in_w : x.P.encn_w - p.sa.in_w;   // (one layer: its span -- the update kernel's range test)
  const LayerW& w = x.W.layers[0];
  a.w0 = SeqLayerW{w.qkv, w.P, w.ctx, w.xhat1, w.rstd1, w.x1, w.hact, w.xhat2, w.rstd2, w.xout};
  a.wstride = x.c.n_enc_layers > 1 ? x.W.layers[1].qkv - w.qkv : 0;
  const WLayout::TmpSet& t = x.W.set[0];
  a.t0 = SeqTmp{t.dzA, t.dzAm, t.dzB, t.dzBm, t.dhid, t.dqkv};
  a.tstride = x.W.set.size() > 1 ? x.W.set[1].dzA - t.dzA : 0;
  a.in_w = x.P.in_w; a.in_b = x.P.in_b; a.encn_w = x.P.encn_w; a.encn_b = x.P.encn_b; a.out_w = x.P.out_w; a.out_b = x.P.out_b;
  a.x0 = x.W.x0; a.a0 = x.W.a0; a.memory = x.W.memory; a.enc_xhat = x.W.enc_xhat; a.enc_rstd = x.W.enc_rstd;
  a.dlogits = x.W.dlogits; a.da0 = x.W.dctx; a.ln_part = x.W.ln_part; a.ln_part_stride = x.W.ln_part_stride;
  a.stamps = x.W.stamps;
  a.pack_f = x.W.pack_f; a.pack_b = x.W.pack_b; a.kstride = x.W.pack_stride;
  a.dctx = x.W.seq_dctx; a.xchg = x.W.seq_xchg; a.xchg_b = x.W.seq_xchg >= 0 ? x.W.seq_xchg + gt_seq_xchg_floats(x.c.batch) : -1; a.fuse_b0 = 0; a.spin_max = xchg_spin_max(GT_XCHG_SPIN_MAX); a.amask = x.W.seq_amask; a.amask_stride = x.W.seq_amask_stride; a.phase = 0;
  a.loss_y = nullptr; a.loss_penalty = 0.f; a.loss_stats = nullptr; a.loss_part = nullptr; a.loss_ticket = nullptr;
  a.grd = nullptr; a.nseq = 0; a.wg_accumulate = 0; a.ride_last_k = x.M; a.out_early = 0; a.tail_phase = 0; a.tail_ksplit = 1; a.ln_nwg = 0; a.bump = nullptr;
  return a;
}
// the whole forward (input layer ... output heads) of every sequence: ONE launch
static int seq_forward(const Ctx& x, const float* pe, const float* src, float* hvo_out, FwdStep* st) {
  const SeqPlan& sp = x.plan;
  SeqArgs a = mk_seq(x, pe, src, hvo_out);
  if (st && st->y != nullptr) {                   // the fused step's loss rides in the launch that runs the output layer (one launch less)
    a.loss_y = st->y; a.loss_penalty = st->penalty; a.loss_stats = st->stats; a.loss_ticket = st->ticket;
    a.loss_part = x.ws + x.W.loss_part;
    st->loss_done = true;
  }
  const double fl = 2.0 * x.M * ((double)x.c.src_dim * x.d + x.c.n_enc_layers * (4.0 * x.d * x.d + 64.0 * x.d + 2.0 * x.d * x.F) + 27.0 * x.d);
  if (!(st && st->packs_current)) {   // fragment-ordered copies of this step's weights, for the forward and the backward kernel
    const int64_t frags = 2 * (int64_t)x.c.n_enc_layers * x.W.pack_stride / 256;
    gt_prof_tag("seq_pack", 0.0, 12.0 * x.c.n_enc_layers * x.W.pack_stride);
    gt_dispatch("seq_pack B %d d %d F %d L %d", x.c.batch, x.d, x.F, x.c.n_enc_layers);
    gt_seq_launch_pack(a, (unsigned)((frags + 3) / 4), x.s);
  }
  // fused train step on the QUAD schedule: the last phase's launch goes on into backward phase 0 (seq_fb_kernel)
  const bool fuse_b0 = sp.fuse_b0 && a.loss_y != nullptr;
  // (its dgrad products -- output layer, FFN2, FFN1, out-proj of the last layer -- are counted where they run)
  gt_prof_tag("seq_fwd", fl + (fuse_b0 ? seq_b0_flops(x) : 0.0), 4.0 * x.M * (x.c.src_dim + x.c.n_enc_layers * (9.0 * x.d + x.F) + 27.0));
  const SeqKernelId id = seq_kernel(x, sp.quad, false);          // (every forward launch of the call runs the same instantiation)
  if (sp.split) {
    // GT_SEQ_QUAD_PRO=1: input layer + in-proj(0) as a prologue launch of their own instead of four times over inside phase 0 --
    // measured neutral at the headline shape (0.2076 vs 0.2073 ms: one more launch for 17 k fewer cycles of phase 0), so off
    a.quad_pro = sp.quad ? (int)gt_switch(GT_SW_SEQ_QUAD_PRO) : 0;
    for (int p = a.quad_pro ? -1 : 0; p < x.c.n_enc_layers; ++p) {   // one launch per encoder layer (gt_seq.h, SPLIT) [+ QUAD's prologue]
      SeqArgs ap = a;
      ap.phase = p;
      if (p > (a.quad_pro ? -1 : 0)) gt_prof_tag("seq_fwd", 0.0, 0.0);          // (flops and bytes of the whole forward are on the first phase's tag)
      // (hc exact attn: the instantiation and the attention form; loss: this launch runs the output layer and takes the fused loss along)
      gt_dispatch("seq_fwd phase %d split 1 quad %d ride %d fuse_b0 %d B %d d %d F %d L %d%s", p, sp.quad, sp.ride,
                  fuse_b0 && p == x.c.n_enc_layers - 1, x.c.batch, x.d, x.F, x.c.n_enc_layers,
                  seq_inst(x, id, false, a.loss_y != nullptr && p == x.c.n_enc_layers - 1).s);
      if (fuse_b0 && p == x.c.n_enc_layers - 1) {
        ap.fuse_b0 = 1;
        gt_seq_launch_fb(ap, 4 * x.c.batch, x.s);
        st->b0_done = true;
      } else if (gt_seq_launch_fwd(ap, id, (sp.quad ? 4 : 2) * x.c.batch, x.s)) {
        return seq_no_kernel("seq_fwd", id);
      }
    }
    return 0;
  }
  gt_dispatch("seq_fwd phase 0 split 0 quad 0 ride 0 fuse_b0 0 B %d d %d F %d L %d%s", x.c.batch, x.d, x.F, x.c.n_enc_layers,
              seq_inst(x, id, false, a.loss_y != nullptr).s);
  return gt_seq_launch_fwd(a, id, x.c.batch, x.s) ? seq_no_kernel("seq_fwd", id) : 0;
}
// the whole backward chain of every sequence in ONE launch (SPLIT: one per phase).  The weight gradients (contractions over all
// sequences) and the LayerNorm parameter gradients ride in the phases and finish in the tail launch (sp.ride: nothing is left for the
// caller), or are queued here for the caller's grouped dispatch and reduce (backward_impl's finish()).
// phase: backward_impl's; cut_layer: first encoder layer of the upper gradient bucket (grad_split); b0_done: FwdStep's
static int seq_backward(const Ctx& x, const float* xin, int accumulate, int phase, int cut_layer, gt_step_state* bump_state, bool grads_zero,
                        bool b0_done) {
  const SeqPlan& sp = x.plan;
  const WLayout& W = x.W;
  const PLayout& P = x.P;
  const int L = x.c.n_enc_layers, B = x.c.batch, S = x.c.src_dim, d = x.d, M = x.M;
  float* ws = x.ws; float* grads = x.grd;
  // LayerNorm jobs in the order the kernel fills their partial blocks (one [2][d] row per sequence)
  const int nwg = sp.split ? 2 * B : B;                        // partial rows per LayerNorm instance: one per workgroup
  bool ok = ln_job(x, P.encn_w, nwg) != nullptr;
  for (int j = L - 1; j >= 0; --j) ok = ok && ln_job(x, P.enc[j].n2w, nwg) && ln_job(x, P.enc[j].n1w, nwg);
  if (!ok) return gt_fail("too many LayerNorm instances for the partials table");
  SeqArgs a = mk_seq(x, nullptr, xin, nullptr);
  // dgrad products (the four Linear dgrads = the forward's GEMM flops; attention backward (dP, dV, dQ, dK) = twice the forward's
  // QK^T + PV; the SPLIT mode's second copy of it is not counted) -- plus, with riders, the weight gradients these launches carry
  double fl = 2.0 * M * (L * (4.0 * d * d + 128.0 * d + 2.0 * d * x.F) + 27.0 * d);
  if (sp.ride) {
    // rider workgroups behind the 2 x batch sequence workgroups: as many as the busiest phase has units, at most the idle CUs
    a.grd = grads; a.nseq = 2 * B; a.wg_accumulate = (accumulate && !grads_zero) ? 1 : 0;
    const int per_layer = gt_seq_wg_tiles(d, x.F) + gt_seq_wg_tiles(x.F, d) + gt_seq_wg_tiles(d, d), win = gt_seq_wg_tiles(3 * d, d);
    const int lnu = (2 * d + 63) / 64;                            // LayerNorm column blocks per job
    const int idle = seq_cu_count() - a.nseq, busiest = per_layer + (L > 1 ? win : 0) + 2 * lnu + (L == 1 ? lnu : 0);
    const int R = idle < busiest ? (idle > 0 ? idle : 1) : busiest;
    // the last phase's sequence work is short (attention backward + in-proj dgrad of layer 0): its riders take only the first
    // GT_SEQ_RIDE_LAST_PCT % of the tokens of each tile, the tail launch -- the whole chip -- adds the rest
    a.ride_last_k = (int)((int64_t)M * GT_SEQ_RIDE_LAST_PCT / 100) / 64 * 64;
    fl += 2.0 * M * ((L - 1) * 3.0 * d * d + L * ((double)d * d + 2.0 * d * x.F))
          - 2.0 * (M - a.ride_last_k) * (per_layer + (L > 1 ? win : 0)) * 2048.0;
    if (b0_done) fl -= seq_b0_flops(x);                         // (phase 0 ran, and was counted, in the forward's last launch)
    gt_prof_tag("seq_bwd", fl, 4.0 * M * (L * (14.0 * d + 2.0 * x.F) + 27.0) + 4.0 * M * L * (8.0 * d + 2.0 * x.F));   // + the riders' operands, once
    // bucketed backward (data-parallel overlap): phase 1 = the launches up to the cut of grad_split, phase 2 = the rest + tail
    const int pcut = L - cut_layer + 1;                          // last backward phase of the first half (two buckets)
    const int p_lo = phase == 2 ? pcut + 1 : 0, p_hi = phase == 1 ? pcut : L;
    a.ln_nwg = nwg;
    for (int p = p_lo; p <= p_hi; ++p) {
      if (p == 0 && b0_done) continue;
      SeqArgs ap = a;
      ap.phase = p;
      if (p > p_lo && !(b0_done && p == 1)) gt_prof_tag("seq_bwd", 0.0, 0.0);
      // phase 0 has no riders: four workgroups per sequence there (column partners, gt_seq.h QUAD) while they fit the chip
      const bool quad = p == 0 && sp.quad;
      const SeqKernelId id = seq_kernel(x, quad, true);
      // (loss 0: no backward launch carries the loss -- the key is there so that both families read alike)
      gt_dispatch("seq_bwd phase %d split 1 quad %d ride 1 riders %d fuse_b0 %d B %d d %d F %d L %d%s", p, quad,
                  p == 0 ? 0 : R, b0_done, B, d, x.F, L, seq_inst(x, id, true, false).s);
      if (gt_seq_launch_bwd(ap, id, quad ? 2 * a.nseq : a.nseq + (p == 0 ? 0 : R), x.s)) return seq_no_kernel("seq_bwd", id);
    }
    if (phase == 1) {      // bucket 0 reaches to the END of the buffer: the output layer's gradient now, by a launch of its own
      a.phase = 0; a.tail_phase = 0; a.tail_ksplit = 2; a.bump = nullptr;
      gt_prof_tag("seq_tail", 2.0 * M * 27.0 * d, 4.0 * M * (27.0 + d));
      gt_dispatch("seq_tail kind out_early B %d d %d F %d L %d", B, d, x.F, L);
      gt_seq_launch_tail(a, (unsigned)(gt_seq_wg_tiles(GT_TGT, d) * 2), x.s);
      return 0;
    }
    a.out_early = phase == 2 ? 1 : 0;
    // the tail: the rest of the last phase's tiles, then in-proj of layer 0 + input layer (token range split in two: two partial
    // tiles adding onto zero commute, so this stays reproducible), the step-counter bump
    const int tiles = win + gt_seq_wg_tiles(d, S) + (a.out_early ? 0 : gt_seq_wg_tiles(GT_TGT, d));
    const int ks = M / 8 < 2 ? M / 8 : 2;
    a.phase = L + 1; a.tail_phase = L + 1; a.tail_ksplit = ks; a.bump = bump_state;
    const int nrest = a.ride_last_k < M ? per_layer + (L > 1 ? win : 0) : 0;
    gt_prof_tag("seq_tail", 2.0 * M * (3.0 * d * d + (a.out_early ? 0.0 : 27.0 * d) + (double)d * S) + 2.0 * (M - a.ride_last_k) * nrest * 2048.0,
                4.0 * M * (4.0 * d + S));
    gt_dispatch("seq_tail kind tail B %d d %d F %d L %d", B, d, x.F, L);
    gt_seq_launch_tail(a, (unsigned)(nrest + tiles * ks), x.s);
    return 0;
  }
  gt_prof_tag("seq_bwd", fl, 4.0 * M * (L * (14.0 * d + 2.0 * x.F) + 27.0));
  const SeqKernelId id = seq_kernel(x, false, true);           // (without riders no backward phase runs four workgroups per sequence)
  for (int p = 0; p <= (sp.split ? L : 0); ++p) {              // SPLIT: one launch per phase; else the one launch
    SeqArgs ap = a;
    ap.phase = p;
    if (p > 0) gt_prof_tag("seq_bwd", 0.0, 0.0);
    gt_dispatch("seq_bwd phase %d split %d quad 0 ride 0 riders 0 fuse_b0 0 B %d d %d F %d L %d%s", p, sp.split, B, d, x.F, L,
                seq_inst(x, id, true, false).s);
    if (gt_seq_launch_bwd(ap, id, nwg, x.s)) return seq_no_kernel("seq_bwd", id);
  }
  wgrad(x, ws + W.dlogits, GT_TGT, ws + W.memory, d, grads + P.out_w, grads + P.out_b, GT_TGT, d);
  for (int j = L - 1; j >= 0; --j) {
    const LayerP& p = P.enc[j];
    const LayerW& w = W.layers[j];
    const Tmp t = tmp_set(x, j);
    const float* lin = (j == 0) ? ws + W.x0 : ws + W.layers[j - 1].xout;
    wgrad(x, t.dzAm, d, ws + w.hact, x.F, grads + p.w2, grads + p.b2, d, x.F);
    wgrad(x, t.dhid, x.F, ws + w.x1, d, grads + p.w1, grads + p.b1, x.F, d);
    wgrad(x, t.dzBm, d, ws + w.ctx, d, grads + p.sa.out_w, grads + p.sa.out_b, d, d);
    wgrad(x, t.dqkv, 3 * d, lin, d, grads + p.sa.in_w, grads + p.sa.in_b, 3 * d, d);
  }
  wgrad(x, ws + W.dctx, d, xin, S, grads + P.in_w, grads + P.in_b, d, S);
  return 0;
}

static int encoder_fwd(const Ctx& x, const float* pe, const float* src) {
  float* ws = x.ws;
  // this step's copies of the encoder layers' weights: `sstride` elements of the copy per layer
  const int tiles = (4 * x.d * x.d + 2 * x.d * x.F) / 1024;
  const dim3 wgrid((unsigned)(tiles * x.c.n_enc_layers));
  auto wcopy_args = [&](int64_t sstride) {
    const LayerP& p0 = x.P.enc[0];
    WShadowArgs a;
    a.prm = x.prm; a.w16 = nullptr; a.w16t = nullptr;
    a.in_w = p0.sa.in_w; a.out_w = p0.sa.out_w; a.w1 = p0.w1; a.w2 = p0.w2;
    a.pstride = x.c.n_enc_layers > 1 ? x.P.enc[1].sa.in_w - p0.sa.in_w : 0; a.sstride = sstride;
    a.d = x.d; a.F = x.F; a.L = x.c.n_enc_layers;
    return a;
  };
  if (x.W.wT >= 0) {       // fp32 transposes: this step's dgrads run as NT products
    gt_prof_tag("weight_shadow", 0.0, 8.0 * x.c.n_enc_layers * tiles * 1024.0);
    gt_launch(weight_transpose_kernel, wgrid, dim3(256), x.s, wcopy_args(x.W.wT_stride), ws + x.W.wT);
  }
  if (x.W.w16 >= 0) {      // bf16 shadows (and their transposes) for this step's Linears and dgrads
    WShadowArgs a = wcopy_args(2 * x.W.w16_stride);
    a.w16 = reinterpret_cast<uint16_t*>(ws + x.W.w16); a.w16t = reinterpret_cast<uint16_t*>(ws + x.W.w16t);
    gt_prof_tag("weight_shadow", 0.0, 8.0 * x.c.n_enc_layers * tiles * 1024.0);
    gt_launch(weight_shadow_kernel, wgrid, dim3(256), x.s, a);
  }
  input_layer_fwd(x, src, x.c.src_dim, x.P.in_w, x.P.in_b, pe, ws + x.W.a0, ws + x.W.x0, GT_SITE_PE_ENC);
  const float* cur = ws + x.W.x0;
  for (int l = 0; l < x.c.n_enc_layers; ++l) {
    const LayerP& p = x.P.enc[l];
    const LayerW& w = x.W.layers[l];
    if (self_attn_fwd(x, p, w, cur, 0, l)) return gt_fail("d_model %d unsupported by the row-LayerNorm kernels", x.d);
    // the final encoder norm rides on the last layer's closing norm (one row pass for both)
    const SecondNorm fin = {x.P.encn_w, ws + x.W.memory, ws + x.W.enc_xhat, ws + x.W.enc_rstd};
    if (ffn_fwd(x, p, w, ws + w.x1, p.n2w, l, l == x.c.n_enc_layers - 1 ? &fin : nullptr)) return -1;
    cur = ws + w.xout;
  }
  return 0;
}
static int decoder_fwd(const Ctx& x, const float* pe, const float* tgt_in) {
  float* ws = x.ws;
  const int d = x.d, L = x.c.n_enc_layers;
  input_layer_fwd(x, tgt_in, GT_TGT, x.P.din_w, x.P.din_b, pe, ws + x.W.b0, ws + x.W.y0, GT_SITE_PE_DEC);
  const float* cur = ws + x.W.y0;
  for (int l = 0; l < x.c.n_dec_layers; ++l) {
    const LayerP& p = x.P.dec[l];
    const LayerW& w = x.W.layers[L + l];
    const int gl = L + l;
    if (self_attn_fwd(x, p, w, cur, 1, gl)) return -1;
    // cross attention: q from the decoder stream (W[0:d]), k,v from the encoder memory (W[d:3d])
    linear_fwd(x, ws + w.x1, d, x.prm + p.xa.in_w, x.prm + p.xa.in_b, ws + w.qx, d, d, d);
    linear_fwd(x, ws + x.W.memory, d, x.prm + p.xa.in_w + (int64_t)d * d, x.prm + p.xa.in_b + d, ws + w.kvx, 2 * d, 2 * d, d);
    attention_fwd(x, ws + w.qx, d, ws + w.kvx, ws + w.kvx + d, 2 * d, ws + w.Px, ws + w.ctxx, 0, lsite(gl, GT_SITE_XATTN));
    if (linear_res_ln(x, ws + w.ctxx, d, p.xa.out_w, p.xa.out_b, ws + w.x1, p.n2w, ws + w.x2, ws + w.xhatx, ws + w.rstdx,
                      lsite(gl, GT_SITE_DROP2))) return -1;
    const SecondNorm fin = {x.P.decn_w, ws + x.W.dec_final, ws + x.W.dec_xhat, ws + x.W.dec_rstd};
    if (ffn_fwd(x, p, w, ws + w.x2, p.n3w, gl, l == x.c.n_dec_layers - 1 ? &fin : nullptr)) return -1;
    cur = ws + w.xout;
  }
  return 0;
}
// ---- greedy decoding, one time step: every row-wise op of the decoder runs on row t of each sequence only (a GEMM with
// M = B and leading dimensions x 32 over the SAME workspace buffers decoder_fwd uses).  The K/V rows self-attention wrote
// at steps < t are the KV cache; cross-attention K/V (ws.kvx) is computed once per layer before the loop.
static void step_linear(const Ctx& x, int B, const float* in, int ldin, const float* W, const float* b, float* out, int ldout, int N, int K) {
  GemmArgs g = mk_gemm(x, in, 32 * ldin, W, K, out, 32 * ldout, B, N, K);
  g.bias = b;
  gemm_launch<false, false, EPI_STORE>(g, x.s);
}
// out_t = LN(in_t W^T + b + res_t)   (eval: no dropout)
static void step_linear_res_ln(const Ctx& x, int B, const float* in, int ldin, int K, int64_t w_off, int64_t b_off, const float* res,
                               int64_t gamma_off, float* out, float* xhat, float* rstd) {
  step_linear(x, B, in, ldin, x.prm + w_off, x.prm + b_off, out, x.d, x.d, K);
  gt_launch(ln_fwd_kernel, dim3((B + 3) / 4), dim3(256), x.s, (const float*)out, res, no_drop(), x.prm + gamma_off,
            x.prm + gamma_off + (x.d + 63) / 64 * 64, out, xhat, rstd, B, x.d, 32 * x.d, 32 * x.d, 32 * x.d, (uint16_t*)nullptr, (const uint16_t*)nullptr);
}
static void step_attention(const Ctx& x, int B, const float* q, int ldq, const float* k, const float* v, int ldkv, float* ctx, int nkeys) {
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldk = ldkv; a.ldv = ldkv; a.ctx = ctx; a.ldc = x.d;
  a.H = x.H; a.hd = x.hd; a.scale = 1.0f / sqrtf((float)x.hd); a.drop = no_drop();
  gt_launch(attn_decode_kernel, dim3(B * x.H), dim3(64), x.s, a, nkeys);
}
static void decoder_step(const Ctx& x, const float* pe, const float* tgt, int t, float* hvo_tmp) {
  float* ws = x.ws;
  const int d = x.d, F = x.F, L = x.c.n_enc_layers, B = x.c.batch;
  const size_t r = (size_t)t;                       // row offset multiplier: buffer + r * ld
  {   // InputLayerDecoder on tgt row t with pe[t]
    GemmArgs g = mk_gemm(x, tgt + r * GT_TGT, 32 * GT_TGT, x.prm + x.P.din_w, GT_TGT, ws + x.W.y0 + r * d, 32 * d, B, d, GT_TGT);
    g.bias = x.prm + x.P.din_b; g.aux = ws + x.W.b0; g.pe = pe + r * d; g.pe_fixed = 1; g.drop = no_drop();
    gemm_launch<false, false, EPI_RELU_PE>(g, x.s);
  }
  const float* cur = ws + x.W.y0;
  for (int l = 0; l < x.c.n_dec_layers; ++l) {
    const LayerP& p = x.P.dec[l];
    const LayerW& w = x.W.layers[L + l];
    // masked self-attention: q, k, v of row t; keys 0..t are in ws.qkv from the earlier steps
    step_linear(x, B, cur + r * d, d, x.prm + p.sa.in_w, x.prm + p.sa.in_b, ws + w.qkv + r * 3 * d, 3 * d, 3 * d, d);
    step_attention(x, B, ws + w.qkv + r * 3 * d, 3 * d, ws + w.qkv + d, ws + w.qkv + 2 * d, 3 * d, ws + w.ctx + r * d, t + 1);
    step_linear_res_ln(x, B, ws + w.ctx + r * d, d, d, p.sa.out_w, p.sa.out_b, cur + r * d, p.n1w, ws + w.x1 + r * d, ws + w.xhat1, ws + w.rstd1);
    // cross attention over the 32 memory positions
    step_linear(x, B, ws + w.x1 + r * d, d, x.prm + p.xa.in_w, x.prm + p.xa.in_b, ws + w.qx + r * d, d, d, d);
    step_attention(x, B, ws + w.qx + r * d, d, ws + w.kvx, ws + w.kvx + d, 2 * d, ws + w.ctxx + r * d, 32);
    step_linear_res_ln(x, B, ws + w.ctxx + r * d, d, d, p.xa.out_w, p.xa.out_b, ws + w.x1 + r * d, p.n2w, ws + w.x2 + r * d, ws + w.xhatx, ws + w.rstdx);
    {   // FFN
      GemmArgs g = mk_gemm(x, ws + w.x2 + r * d, 32 * d, x.prm + p.w1, d, ws + w.hact + r * F, 32 * F, B, F, d);
      g.bias = x.prm + p.b1; g.drop = no_drop();
      gemm_launch<false, false, EPI_RELU_DROP>(g, x.s);
    }
    step_linear_res_ln(x, B, ws + w.hact + r * F, F, F, p.w2, p.b2, ws + w.x2 + r * d, p.n3w, ws + w.xout + r * d, ws + w.xhat2, ws + w.rstd2);
    cur = ws + w.xout;
  }
  gt_launch(ln_fwd_kernel, dim3((B + 3) / 4), dim3(256), x.s, cur + r * d, (const float*)nullptr, no_drop(), x.prm + x.P.decn_w,
            x.prm + x.P.decn_b, ws + x.W.dec_final + r * d, ws + x.W.dec_xhat, ws + x.W.dec_rstd, B, d, 32 * d, 32 * d, 32 * d, (uint16_t*)nullptr, (const uint16_t*)nullptr);
  GemmArgs g = mk_gemm(x, ws + x.W.dec_final + r * d, 32 * d, x.prm + x.P.out_w, d, hvo_tmp + r * GT_TGT, 32 * GT_TGT, B, GT_TGT, d);
  g.bias = x.prm + x.P.out_b;
  gemm_launch<false, false, EPI_HEADS>(g, x.s);
}
static void output_layer_fwd(const Ctx& x, float* hvo_out, FwdStep* st = nullptr) {
  const float* fin = x.ws + (x.c.n_dec_layers > 0 ? x.W.dec_final : x.W.memory);
  if (heads_fwd_ok(x.M, x.d, x.d, fin, x.prm + x.P.out_w)) {
    // the fused train step hands the loss over as well (as to the sequence-resident launches): one launch for OutputLayer + loss
    HeadsLoss hl = {nullptr, 0.f, nullptr, nullptr, nullptr, nullptr};
    if (st && st->y != nullptr) {
      hl = HeadsLoss{st->y, st->penalty, st->stats, x.ws + x.W.loss_part, st->ticket, x.ws + x.W.dlogits};
      st->loss_done = true;
    }
    static const bool trace = [] { const char* e = getenv("GT_TRACE_HEADS"); return e && e[0] == '1'; }();     // (tests: which launches took the kernel)
    if (trace) fprintf(stderr, "[heads] M %d d %d precision %d loss %d\n", x.M, x.d, x.c.precision, hl.y != nullptr);
    gt_prof_tag("gemm_fwd_heads", 2.0 * x.M * GT_TGT * x.d, 4.0 * ((double)x.M * x.d + (double)GT_TGT * x.d + (double)x.M * GT_TGT));
    gt_dispatch("heads M %d d %d prec %d loss %d", x.M, x.d, x.c.precision, hl.y != nullptr);
    if (x.c.precision) gt_launch(heads_fwd_kernel<1>, dim3(x.M / 16), dim3(256), x.s, fin, (const float*)(x.prm + x.P.out_w), (const float*)(x.prm + x.P.out_b), hvo_out, x.M, x.d, hl);
    else               gt_launch(heads_fwd_kernel<0>, dim3(x.M / 16), dim3(256), x.s, fin, (const float*)(x.prm + x.P.out_w), (const float*)(x.prm + x.P.out_b), hvo_out, x.M, x.d, hl);
    return;
  }
  GemmArgs g = mk_gemm(x, fin, x.d, x.prm + x.P.out_w, x.d, hvo_out, GT_TGT, x.M, GT_TGT, x.d);
  g.bias = x.prm + x.P.out_b;
  gemm_launch<false, false, EPI_HEADS>(g, x.s);
}

// st: the hand-offs of a fused train step (FwdStep; nullptr: a plain forward -- no loss taken along, weights packed, no backward phase)
static int forward_impl(const Ctx& x, const float* pe, const float* xin, const float* tgt_in, float* hvo_out, FwdStep* st) {
  if (!pe || !xin || !hvo_out) return gt_fail("gt_forward: pe / x / hvo_out must not be NULL");
  if (x.c.n_dec_layers > 0 && !tgt_in) return gt_fail("gt_forward: encoder-decoder model needs tgt_in");
  if (x.plan.seq) {
    seq_forward(x, pe, xin, hvo_out, st);
    return launch_status(x, "gt_forward");
  }
  if (encoder_fwd(x, pe, xin)) return -1;
  if (x.c.n_dec_layers > 0 && decoder_fwd(x, pe, tgt_in)) return -1;
  output_layer_fwd(x, hvo_out, st);
  return launch_status(x, "gt_forward");
}
extern "C" int gt_forward(const gt_config* cfg, const float* params, const float* pe, const float* xin, const float* tgt_in,
                          float* hvo_out, float* ws, const gt_step_state* state, int train, gt_stream_t stream) {
  Ctx x;
  if (make_ctx(x, cfg, params, nullptr, ws, state, train, stream)) return -1;
  x.plan = seq_plan(x.c);
  return forward_impl(x, pe, xin, tgt_in, hvo_out, nullptr);
}

// ------------------------------------------------------------------------------------ loss
extern "C" int gt_loss(const gt_config* cfg, const float* hvo, const float* y, float hit_loss_penalty, float* stats, float* d_hvo,
                       gt_stream_t stream) {
  if (check_cfg(cfg)) return -1;
  if (!hvo || !y || !stats) return gt_fail("gt_loss: hvo / y / stats must not be NULL");
  const int M = cfg->batch * 32;
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(stats, 0, 8 * sizeof(float), s);
  gt_prof_tag("loss", 0, 12.0 * M * GT_TGT);
  gt_launch(loss_kernel<false, false>, dim3((M * GT_VOICES + 255) / 256), dim3(256), s, hvo, y, hit_loss_penalty, stats, d_hvo, M,
            (float*)nullptr, (unsigned*)nullptr);
  return launch_status("gt_loss");
}

// The loss with options (gt_misc.h loss_ex_kernel): one workgroup per sequence, the options baked into the launch (host struct, read here --
// as gt_optimizer_prepare's hyper-parameters are).  scratch = the ticket word, then GT_LOSSX_PART partials per sequence.
static int loss_opts_check(const char* what, const gt_loss_opts* lo) {
  if (!lo) return gt_fail("%s: lo must not be NULL", what);
  const auto bad = [](float a) { return !(a >= 0.f) || __builtin_isinf(a); };      // negative, NaN or Inf
  if (bad(lo->penalty_h) || bad(lo->penalty_vo))
    return gt_fail("%s: penalty_h %g / penalty_vo %g must be >= 0 and finite", what, (double)lo->penalty_h, (double)lo->penalty_vo);
  for (int c = 0; c < GT_VOICES; ++c) {
    if (bad(lo->pos_weight[c]) || lo->pos_weight[c] == 0.f) return gt_fail("%s: pos_weight[%d] = %g must be > 0 and finite", what, c, (double)lo->pos_weight[c]);
    if (bad(lo->voice_weight[c])) return gt_fail("%s: voice_weight[%d] = %g must be >= 0 and finite", what, c, (double)lo->voice_weight[c]);
  }
  for (int q = 0; q < 3; ++q)
    if (bad(lo->term_weight[q])) return gt_fail("%s: term_weight[%d] = %g must be >= 0 and finite", what, q, (double)lo->term_weight[q]);
  if (!(lo->focal_gamma >= 0.f && lo->focal_gamma <= 8.f)) return gt_fail("%s: focal_gamma %g outside [0, 8]", what, (double)lo->focal_gamma);
  return 0;
}
static void loss_ex_launch(const gt_config& c, const float* hvo, const float* y, const gt_loss_opts& lo, float* stats, float* voice_stats,
                           float* d_out, bool wrt_logits, float* scratch, hipStream_t s) {
  const int M = c.batch * 32;
  gt_prof_tag("loss_ex", 0, 12.0 * M * GT_TGT);
  unsigned* ticket = reinterpret_cast<unsigned*>(scratch);
  if (wrt_logits) gt_launch(loss_ex_kernel<true>, dim3(c.batch), dim3(GT_LOSSX_THREADS), s, hvo, y, lo, stats, voice_stats, d_out, M, scratch + 1, ticket);
  else            gt_launch(loss_ex_kernel<false>, dim3(c.batch), dim3(GT_LOSSX_THREADS), s, hvo, y, lo, stats, voice_stats, d_out, M, scratch + 1, ticket);
}
extern "C" int64_t gt_loss_scratch_floats(const gt_config* cfg) {
  if (check_cfg(cfg)) return 0;
  return (int64_t)cfg->batch * GT_LOSSX_PART + 1;
}
extern "C" int gt_loss_ex(const gt_config* cfg, const float* hvo, const float* y, const gt_loss_opts* lo, float* stats, float* voice_stats,
                          float* d_out, int wrt_logits, float* scratch, gt_stream_t stream) {
  if (check_cfg(cfg)) return -1;
  if (!hvo || !y || !stats || !scratch) return gt_fail("gt_loss_ex: hvo / y / stats / scratch must not be NULL");
  if (loss_opts_check("gt_loss_ex", lo)) return -1;
  loss_ex_launch(*cfg, hvo, y, *lo, stats, voice_stats, d_out, wrt_logits != 0, scratch, (hipStream_t)stream);
  return launch_status("gt_loss_ex");
}

// ------------------------------------------------------------------------------------ backward
// FFN block backward.  In: dz (grad of the pre-norm sum of the layer's last norm) and its dropout-masked
// copy dzm.  Out: dz_prev = LNbwd_prev(dhid W1 + dz) into (dzo, dzom) for the norm in front of the FFN.
static int ffn_bwd(const Ctx& x, const LayerP& p, const LayerW& w, const Tmp& t, const float* xin, const float* dz, const float* dzm,
                   const float* xhat_prev, const float* rstd_prev, int64_t gamma_prev, float* dzo, float* dzom, int site_prev) {
  float* ws = x.ws;
  wgrad(x, dzm, x.d, ws + w.hact, x.F, x.grd + p.w2, x.grd + p.b2, x.d, x.F);
  bool nt, ok;
  GemmArgs g = ffn2d_args(x, p, w, t, dzm, &nt, &ok);
  need16(x, ok, "FFN2 dgrad over bf16-only tensors");
  int gl = 0;                                                  // (the layer's index in the workspace: the keep bits are per layer)
  while (gl + 1 < (int)x.W.layers.size() && x.W.layers[gl].hact != w.hact) ++gl;
  if (dzm == tmp_set(x, gl).dzAm) g.kbits = ffn_kbits(x, p, w, xin, gl);       // (the set the forward's decision looked at -- always, today)
  if (g.kbits) gemm64_trace("kbits read", g, !nt, EPI_MASK_NZ);
  if (nt) gemm_launch<false, false, EPI_MASK_NZ>(g, x.s);
  else    gemm_launch<false, true, EPI_MASK_NZ>(g, x.s);
  wgrad(x, t.dhid, x.F, xin, x.d, x.grd + p.w1, x.grd + p.b1, x.F, x.d);
  return dgrad_lnbwd(x, t.dhid, x.F, x.prm + p.w1, x.F, dz, xhat_prev, rstd_prev, gamma_prev, dzo, dzom, site_prev);
}
// self-attention block backward.  In: dz1m (masked grad of the out-proj output).  Leaves dqkv in the set.
static void self_attn_bwd(const Ctx& x, const LayerP& p, const LayerW& w, const Tmp& t, const float* xin, const float* dz1m, int gl) {
  float* ws = x.ws;
  const int d = x.d;
  wgrad(x, dz1m, d, ws + w.ctx, d, x.grd + p.sa.out_w, x.grd + p.sa.out_b, d, d);
  const bool s16 = p2(x.c) && gl < x.c.n_enc_layers;          // precision = 2: dctx in bf16 alone (the first half of its buffer), like qkv
  dgrad_store(x, dz1m, d, x.prm + p.sa.out_w, d, ws + x.W.dctx, d, d, 0, s16 ? reinterpret_cast<uint16_t*>(ws + x.W.dctx) : nullptr);
  attention_bwd(x, ws + w.qkv, 3 * d, ws + w.qkv + d, ws + w.qkv + 2 * d, 3 * d, ws + w.P, ws + x.W.dctx, t.dqkv, 3 * d,
                t.dqkv + d, t.dqkv + 2 * d, 3 * d, lsite(gl, GT_SITE_ATTN), s16);
  wgrad(x, t.dqkv, 3 * d, xin, d, x.grd + p.sa.in_w, x.grd + p.sa.in_b, 3 * d, d);
}
// grad of the InputLayer: da = (dqkv Win + dz1) * dropmask * (a0 > 0) -> da_out; dW = da^T in; db = colsum(da)
static void input_layer_bwd(const Ctx& x, const LayerP& first, const Tmp& t, const float* dz1, const float* a0, const float* in, int S,
                            int64_t w, int64_t b, int site, float* da_out) {
  if (const float* wt = wT_of(x, x.prm + first.sa.in_w)) {
    GemmArgs g = mk_gemm(x, t.dqkv, 3 * x.d, wt, 3 * x.d, da_out, x.d, x.M, x.d, 3 * x.d);
    g.res = dz1; g.ldres = x.d; g.aux_in = a0; g.drop = mk_drop(x, site);
    gemm_launch<false, false, EPI_ADD_RELUMASK_DROP>(g, x.s);
    wgrad(x, da_out, x.d, in, S, x.grd + w, x.grd + b, x.d, S);
    return;
  }
  GemmArgs g = mk_gemm(x, t.dqkv, 3 * x.d, x.prm + first.sa.in_w, x.d, da_out, x.d, x.M, x.d, 3 * x.d);
  g.res = dz1; g.ldres = x.d; g.aux_in = a0; g.drop = mk_drop(x, site);
  g.A16 = sh_act(x, t.dqkv); g.B16 = sh_w(x, x.prm + first.sa.in_w, true); g.lda16 = g.ldb16 = 3 * x.d;
  if (only16(x, t.dqkv)) need16(x, g.A16 && g.B16 && gemm32h_ok(g, EPI_ADD_RELUMASK_DROP), "InputLayer dgrad of a bf16-only tensor");
  gemm_launch<false, true, EPI_ADD_RELUMASK_DROP>(g, x.s);
  wgrad(x, da_out, x.d, in, S, x.grd + w, x.grd + b, x.d, S);
}

// Gradient buckets for data-parallel overlap, in the order backward completes them.  Parameters are laid out
// [in | enc layers | enc norm | (dec in | dec layers | dec norm) | out] and backward walks that list from its end, so
// "everything from tensor X to the end" is final early: X = the decoder input layer of an encoder-decoder model, else
// encoder layer L/2.  split_layer: first encoder layer of the upper bucket (enc-dec: L, i.e. no encoder layer).
struct GradSplit { int nb; int split_layer; int64_t off[2], cnt[2]; };
static GradSplit grad_split(const gt_config& c, const PLayout& P, const SeqPlan& sp) {
  GradSplit g;
  g.nb = 1; g.split_layer = 0; g.off[0] = 0; g.cnt[0] = P.total; g.off[1] = g.cnt[1] = 0;
  int64_t cut = 0;
  if (c.n_dec_layers > 0) { cut = P.din_w; g.split_layer = c.n_enc_layers; }
  else if (c.n_enc_layers >= 2) { g.split_layer = c.n_enc_layers / 2; cut = P.enc[g.split_layer].sa.in_w; }
  // sequence-resident path: one bucket -- unless the weight gradients ride in the backward phases (gt_seq_wg.h): after phase p < L
  // everything from encoder layer L - p + 1 on is final; the cut is after phase min((L + 2) / 2, L - 1)
  if (sp.seq) {
    const int L = c.n_enc_layers;
    int pcut = (L + 2) / 2;                       // (the LAST phase's tiles are finished by the tail launch: the cut lies before it)
    if (pcut > L - 1) pcut = L - 1;
    if (pcut >= 1 && sp.ride) { g.split_layer = L - pcut + 1; cut = g.split_layer < L ? P.enc[g.split_layer].sa.in_w : P.encn_w; }
    else cut = 0;
  }
  if (cut > 0) {
    g.nb = 2; g.off[0] = cut; g.cnt[0] = P.total - cut; g.off[1] = 0; g.cnt[1] = cut;
  }
  return g;
}
extern "C" int gt_grad_buckets(const gt_config* cfg, int64_t* offsets, int64_t* counts) {
  if (check_cfg(cfg)) return -1;
  if (!offsets || !counts) return gt_fail("gt_grad_buckets: offsets / counts must not be NULL");
  const PLayout P = param_layout(*cfg);
  const GradSplit g = grad_split(*cfg, P, seq_plan(*cfg));
  for (int i = 0; i < 2; ++i) { offsets[i] = g.off[i]; counts[i] = g.cnt[i]; }
  return g.nb;
}

// d loss / d logits from d loss / d hvo -- unless ws.dlogits already holds it (d_hvo == nullptr: the fused loss kernel wrote it)
static void heads_bwd(const Ctx& x, const float* hvo, const float* d_hvo) {
  if (d_hvo == nullptr) return;
  gt_prof_tag("heads_bwd", 0, 12.0 * x.M * GT_TGT);
  gt_launch(heads_bwd_kernel, dim3((x.M * GT_TGT + 255) / 256), dim3(256), x.s, d_hvo, hvo, x.ws + x.W.dlogits, x.M * GT_TGT);
}
// The one-kernel-per-op backward.  phase: backward_impl's, of a two-bucket cut (else 0); cut_layer: first encoder layer of the upper bucket
// (grad_split).  Bucket 0 is the output layer with the decoder half (encoder-decoder) or with the encoder layers from cut_layer up; bucket 1
// the encoder layers below.  Weight gradients and LayerNorm partials queue up on x.wb / x.ln: the caller's finish() sends them.
static int op_backward(const Ctx& x, const float* xin, const float* tgt_in, const float* hvo, const float* d_hvo, int phase, int cut_layer) {
  const float* params = x.prm; float* grads = x.grd; float* ws = x.ws;
  const int L = x.c.n_enc_layers, Ld = x.c.n_dec_layers, d = x.d, M = x.M;
  const WLayout& W = x.W; const PLayout& P = x.P;
  if (phase != 2) {                                 // bucket 0 opens with the output layer, the final norm and the decoder half
    // OutputLayer: dlogits, dW_out, then d(final) fused with the final norm's backward
    heads_bwd(x, hvo, d_hvo);
    const float* fin = ws + (Ld > 0 ? W.dec_final : W.memory);
    wgrad(x, ws + W.dlogits, GT_TGT, fin, d, grads + P.out_w, grads + P.out_b, GT_TGT, d);
    // the final norm's backward and the top layer's closing norm's backward sit back to back: when the output-layer dgrad is
    // an ordinary tiled GEMM (row_fused false) both run as ONE row pass (ln_bwd2); with fused row tiles the first one is the
    // GEMM's epilogue and the second its own pass.  Either way (dzA, dzAm) of the top layer come out.
    const float* xh = ws + (Ld > 0 ? W.dec_xhat : W.enc_xhat);
    const float* rs = ws + (Ld > 0 ? W.dec_rstd : W.enc_rstd);
    const int64_t gfin = Ld > 0 ? P.decn_w : P.encn_w, gtop = Ld > 0 ? P.dec[Ld - 1].n3w : P.enc[L - 1].n2w;
    const int top = L + Ld - 1;                     // global index of the last layer
    const LayerW& wtop = W.layers[top];
    const Tmp ttop = tmp_set(x, top);
    if (!row_fused(x)) {
      dgrad_store(x, ws + W.dlogits, GT_TGT, params + P.out_w, d, ws + W.dctx, d, GT_TGT, 0);
      ln_bwd2(x, ws + W.dctx, xh, rs, gfin, ws + W.dctx, ws + wtop.xhat2, ws + wtop.rstd2, gtop, ttop.dzA, ttop.dzAm, lsite(top, GT_SITE_DROPF));
    } else {
      if (dgrad_lnbwd(x, ws + W.dlogits, GT_TGT, params + P.out_w, GT_TGT, nullptr, xh, rs, gfin, ws + W.dctx, nullptr, 0))
        return gt_fail("d_model %d unsupported by the row-LayerNorm kernels", d);
      ln_bwd(x, ws + W.dctx, nullptr, ws + wtop.xhat2, ws + wtop.rstd2, gtop, ttop.dzA, ttop.dzAm, lsite(top, GT_SITE_DROPF));
    }
    if (Ld > 0) {
      // (ws.dmem, the memory gradient, is the SUM of the decoder layers' cross-attention k / v dgrads: the first one processed stores, the
      //  others add.  Round 5: it used to be zeroed by a hipMemsetAsync here -- a memset NODE inside the step's captured graph -- and the
      //  encoder-decoder step then went non-finite intermittently when replays were separated by a host synchronisation (C3, and already
      //  the L1+1 model: 2 of 3 processes; never eagerly, never without the decoder): the only memset node of the fused step is gone.)
      for (int l = Ld - 1; l >= 0; --l) {
        const LayerP& p = P.dec[l];
        const int gl = L + l;
        const LayerW& w = W.layers[gl];
        const Tmp t = tmp_set(x, gl);
        const float* yin = (l == 0) ? ws + W.y0 : ws + W.layers[gl - 1].xout;
        // FFN (norm3's backward was done by the producer of dzA) -> dz2 = LNbwd_norm2(...) in (dzB, dzBm)
        if (ffn_bwd(x, p, w, t, ws + w.x2, t.dzA, t.dzAm, ws + w.xhatx, ws + w.rstdx, p.n2w, t.dzB, t.dzBm, lsite(gl, GT_SITE_DROP2))) return -1;
        // cross attention: q from the decoder stream, k/v from the encoder memory
        wgrad(x, t.dzBm, d, ws + w.ctxx, d, grads + p.xa.out_w, grads + p.xa.out_b, d, d);
        dgrad_store(x, t.dzBm, d, params + p.xa.out_w, d, ws + W.dctx, d, d, 0);
        float* dqx = t.dqkvx; float* dkvx = t.dqkvx + (int64_t)M * d;            // dq (M,d) then dkv (M,2d), both dense
        attention_bwd(x, ws + w.qx, d, ws + w.kvx, ws + w.kvx + d, 2 * d, ws + w.Px, ws + W.dctx, dqx, d, dkvx, dkvx + d, 2 * d,
                      lsite(gl, GT_SITE_XATTN));
        wgrad(x, dqx, d, ws + w.x1, d, grads + p.xa.in_w, grads + p.xa.in_b, d, d);
        wgrad(x, dkvx, 2 * d, ws + W.memory, d, grads + p.xa.in_w + (int64_t)d * d, grads + p.xa.in_b + d, 2 * d, d);
        dgrad_store(x, dkvx, 2 * d, params + p.xa.in_w + (int64_t)d * d, d, ws + W.dmem, d, 2 * d, l == Ld - 1 ? 0 : 1);
        // dz1 = LNbwd_norm1(dqx Wq + dz2) -> (dzC, dzCm) masked for the self-attn out-proj
        if (dgrad_lnbwd(x, dqx, d, params + p.xa.in_w, d, t.dzB, ws + w.xhat1, ws + w.rstd1, p.n1w, t.dzC, t.dzCm, lsite(gl, GT_SITE_DROP1)))
          return -1;
        self_attn_bwd(x, p, w, t, yin, t.dzCm, gl);
        if (l > 0) {
          const LayerW& wp = W.layers[gl - 1];
          const Tmp tn = tmp_set(x, gl - 1);
          if (dgrad_lnbwd(x, t.dqkv, 3 * d, params + p.sa.in_w, 3 * d, t.dzC, ws + wp.xhat2, ws + wp.rstd2, P.dec[l - 1].n3w, tn.dzA,
                          tn.dzAm, lsite(gl - 1, GT_SITE_DROPF)))
            return -1;
        } else {
          input_layer_bwd(x, p, t, t.dzC, ws + W.b0, tgt_in, GT_TGT, P.din_w, P.din_b, GT_SITE_PE_DEC, ws + W.da0_dec);
        }
      }
    }
  }
  if (Ld > 0) {
    if (phase == 1) return 0;                       // decoder half (bucket 0) done; ws.dmem holds the memory gradient
    // encoder final norm backward (input: accumulated dmem) and the last encoder layer's closing norm: one row pass
    const LayerW& w = W.layers[L - 1];
    const Tmp t = tmp_set(x, L - 1);
    ln_bwd2(x, ws + W.dmem, ws + W.enc_xhat, ws + W.enc_rstd, P.encn_w, ws + W.dctx, ws + w.xhat2, ws + w.rstd2, P.enc[L - 1].n2w,
            t.dzA, t.dzAm, lsite(L - 1, GT_SITE_DROPF));
  }
  // encoder layers hi .. lo: all of them, or (encoder-only, two buckets) those from cut_layer up, then those below.  The layers from the
  // cut up are final when the first half ends; (dzA, dzAm) of layer cut_layer - 1 are what it hands to the second
  const int hi = (Ld == 0 && phase == 2) ? cut_layer - 1 : L - 1, lo = (Ld == 0 && phase == 1) ? cut_layer : 0;
  for (int l = hi; l >= lo; --l) {
    const LayerP& p = P.enc[l];
    const LayerW& w = W.layers[l];
    const Tmp t = tmp_set(x, l);
    const float* lin = (l == 0) ? ws + W.x0 : ws + W.layers[l - 1].xout;
    if (ffn_bwd(x, p, w, t, ws + w.x1, t.dzA, t.dzAm, ws + w.xhat1, ws + w.rstd1, p.n1w, t.dzB, t.dzBm, lsite(l, GT_SITE_DROP1))) return -1;
    self_attn_bwd(x, p, w, t, lin, t.dzBm, l);
    if (l > 0) {
      const LayerW& wp = W.layers[l - 1];
      const Tmp tn = tmp_set(x, l - 1);
      if (dgrad_lnbwd(x, t.dqkv, 3 * d, params + p.sa.in_w, 3 * d, t.dzB, ws + wp.xhat2, ws + wp.rstd2, P.enc[l - 1].n2w, tn.dzA, tn.dzAm,
                      lsite(l - 1, GT_SITE_DROPF)))
        return -1;
    } else {
      input_layer_bwd(x, p, t, t.dzB, ws + W.a0, xin, x.c.src_dim, P.in_w, P.in_b, GT_SITE_PE_ENC, ws + W.dctx);
    }
  }
  return 0;
}
// phase 0: the whole backward; 1: only until bucket 0 of grad_split() is final; 2: the rest (after a phase-1 call on the
// same workspace -- the hand-over temporaries live there).  b0_done: the caller's forward ran backward phase 0 already (FwdStep).
// x: the caller's context with its plan, by value -- the queues of this call hang off the copy.
static int backward_impl(Ctx x, const float* xin, const float* tgt_in, const float* hvo, const float* d_hvo, int accumulate, int phase,
                         gt_step_state* bump_state, bool grads_zero, bool b0_done) {
  if (!x.grd || !xin) return gt_fail("gt_backward: grads / x must not be NULL");
  const int d = x.d;
  if (x.c.n_dec_layers > 0 && !tgt_in) return gt_fail("gt_backward: encoder-decoder model needs tgt_in");
  const WLayout& W = x.W; const PLayout& P = x.P;
  if (!accumulate) (void)hipMemsetAsync(x.grd, 0, (size_t)P.total * sizeof(float), x.s);
  // Weight gradients are queued and leave as ONE grouped dispatch per tile class at the end of the (phase of) backward
  // (finish()); every layer keeps its own temporaries (W.set) for that.
  WgradBatch wbatch;
  x.wb = &wbatch;
  LnJobs lnjobs;
  lnjobs.n = 0; lnjobs.N = d; lnjobs.bump = nullptr;
  lnjobs.err = xchg_err(x.W, x.ws);
  x.ln = &lnjobs;
  const GradSplit cut = grad_split(x.c, P, x.plan);
  if (cut.nb < 2) {                                 // nothing to split: phase 1 does everything, phase 2 nothing
    if (phase == 2) return 0;
    phase = 0;
  }
  // end of a phase: the queued weight gradients leave, the LayerNorm parameter-gradient partials queued so far are summed
  auto finish = [&]() -> int {
    if (!wbatch.empty()) wgrad_flush(wbatch, x.s);  // one grouped dispatch per tile class
    if (lnjobs.n > 0) {                             // LayerNorm dgamma/dbeta: one launch, fixed order
      lnjobs.bump = bump_state;
      gt_prof_tag("ln_param_reduce", 0, 4.0 * lnjobs.n * W.ln_part_stride);
      gt_dispatch("ln_param_reduce jobs %d d %d", lnjobs.n, d);
      gt_launch(ln_param_reduce_kernel, dim3((2 * d + 63) / 64, lnjobs.n), dim3(1024), x.s, lnjobs);
    }
    return launch_status(x, "gt_backward");
  };

  if (x.plan.seq) {
    // ---- sequence-resident path (gt_seq.h): the whole backward chain of every sequence in ONE launch; the weight gradients
    // (contractions over all sequences) and the LayerNorm parameter gradients leave as the grouped dispatch / the reduce -- or,
    // with riders, have left in the phases and the tail launch
    heads_bwd(x, hvo, d_hvo);
    if (seq_backward(x, xin, accumulate, phase, cut.split_layer, bump_state, grads_zero, b0_done)) return -1;
    return x.plan.ride ? launch_status(x, "gt_backward") : finish();
  }
  // ---- one kernel per op
  if (op_backward(x, xin, tgt_in, hvo, d_hvo, phase, cut.split_layer)) return -1;
  return finish();
}

// Measurement aid: the weight-gradient units of backward phase `phase` (gt_seq_wg.h) as a launch of their own, token range split
// `ksplit` ways, adding into grads -- operands are whatever the last backward left in ws.  tools/wg_unit_bench.py times it.
extern "C" int gt_debug_seq_wg_phase(const gt_config* cfg, const float* params, float* grads, const float* xin, float* ws, int phase,
                                     int ksplit, gt_stream_t stream) {
  Ctx x;
  if (make_ctx(x, cfg, params, grads, ws, nullptr, 0, stream)) return -1;
  if (!seq_supported(*cfg) || cfg->d_model != 128) return gt_fail("gt_debug_seq_wg_phase: d_model 128 sequence-resident shapes only");
  const int L = cfg->n_enc_layers, d = x.d;
  if (phase < 0 || phase > L + 1 || ksplit < 1) return gt_fail("gt_debug_seq_wg_phase: phase / ksplit out of range");
  SeqArgs a = mk_seq(x, nullptr, xin, nullptr);
  a.grd = grads; a.nseq = 0; a.wg_accumulate = 1; a.phase = phase; a.tail_phase = phase; a.tail_ksplit = ksplit; a.ln_nwg = 0; a.bump = nullptr;
  if (phase == 0 || phase > L) return gt_fail("gt_debug_seq_wg_phase: phases 1..L carry riders");
  const int per_layer = gt_seq_wg_tiles(d, x.F) + gt_seq_wg_tiles(x.F, d) + gt_seq_wg_tiles(d, d), win = gt_seq_wg_tiles(3 * d, d);
  const int tiles = per_layer + (phase >= 2 ? win : 0);
  gt_prof_tag("seq_tail", 0.0, 0.0);
  gt_seq_launch_tail(a, (unsigned)(tiles * ksplit), x.s);
  return launch_status(x, "gt_debug_seq_wg_phase");
}

extern "C" int gt_backward(const gt_config* cfg, const float* params, float* grads, const float* xin, const float* tgt_in,
                           const float* hvo, const float* d_hvo, float* ws, const gt_step_state* state, int train, int accumulate,
                           gt_stream_t stream) {
  if (!hvo || !d_hvo) return gt_fail("gt_backward: hvo / d_hvo must not be NULL");
  Ctx x;
  if (make_ctx(x, cfg, params, grads, ws, state, train, stream)) return -1;
  x.plan = seq_plan(x.c);
  return backward_impl(std::move(x), xin, tgt_in, hvo, d_hvo, accumulate, 0, nullptr, false, false);    // (a forward of its own ran no backward phase)
}

// ------------------------------------------------------------------------------------ optimizer
// step_advanced: the caller's previous launch already advanced step / opt_step (fused train step, see LnJobs::bump)
// err / guard: the fail-safe of the in-launch exchanges (gt_misc.h, sgd_kernel) -- only callers that hold the configuration's WHOLE flat buffers
// and its workspace pass them (gt_train_step, gt_optimizer_step_ws); the public gt_optimizer_step is a plain update of n elements
static int optimizer_step_impl(int algo, float* params, float* grads, float* m, float* v, int64_t n, gt_step_state* state,
                               int zero_grads, gt_stream_t stream, int step_advanced, unsigned* err = nullptr, int guard = 0) {
  if (!params || !grads || !state || n <= 0) return gt_fail("gt_optimizer_step: params / grads / state must not be NULL");
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((n + 1023) / 1024);
  if (algo == 0) {
    gt_prof_tag("optimizer", 0, 12.0 * n);
    gt_dispatch("update kind plain algo 0 n %lld", (long long)n);
    gt_launch(sgd_kernel, dim3(blocks), dim3(256), s, params, grads, n, (const gt_step_state*)state, zero_grads, (const unsigned*)err, guard);
  } else if (algo == 1) {
    if (!m || !v) return gt_fail("gt_optimizer_step: adam needs m and v");
    gt_prof_tag("optimizer", 0, 28.0 * n);
    gt_dispatch("update kind plain algo 1 n %lld", (long long)n);
    gt_launch(adam_kernel, dim3(blocks), dim3(256), s, params, grads, m, v, n, (const gt_step_state*)state, zero_grads, step_advanced, (const unsigned*)err, guard);
  } else {
    return gt_fail("optimizer algo %d unknown (0 = sgd, 1 = adam)", algo);
  }
  if (!step_advanced) gt_launch(step_inc_kernel, dim3(1), dim3(64), s, state, err, guard ? (const float*)(grads + n - 1) : (const float*)nullptr);
  return launch_status("gt_optimizer_step");
}
extern "C" int gt_optimizer_step(int algo, float* params, float* grads, float* m, float* v, int64_t n, gt_step_state* state,
                                 int zero_grads, gt_stream_t stream) {
  return optimizer_step_impl(algo, params, grads, m, v, n, state, zero_grads, stream, 0);
}
// The folded update of the sequence-resident path: the optimizer step over the WHOLE flat buffers of x (params = x.prm, x.grd) that also
// writes the NEXT step's fragment-ordered weights into ws (its caller may then pass GT_STEP_PACKS_CURRENT and the packing launch at the
// head of the step disappears).  step_advanced: as optimizer_step_impl's.  pe / xin / hvo_out: what the caller's step ran on, or NULL.
static int seq_update_pack(const Ctx& x, int algo, float* params, float* m, float* v, const float* pe, const float* xin, float* hvo_out,
                           gt_step_state* state, int step_advanced) {
  if (algo != 0 && algo != 1) return gt_fail("optimizer algo %d unknown (0 = sgd, 1 = adam)", algo);
  if (algo == 1 && (!m || !v)) return gt_fail("gt_optimizer_step: adam needs m and v");
  const SeqArgs a = mk_seq(x, pe, xin, hvo_out);
  gt_prof_tag("optimizer", 0, (algo ? 28.0 : 12.0) * x.P.total + 8.0 * x.c.n_enc_layers * x.W.pack_stride);
  gt_dispatch("update kind folded_pack algo %d n %lld", algo, (long long)x.P.total);
  gt_seq_launch_update_pack(a, algo, params, x.grd, m, v, x.P.total, state, step_advanced, x.s);
  return 0;
}

// gt_optimizer_step for a caller that steps with gt_train_step(skip_update = 1..3) (data-parallel: all-reduce in between): on the
// sequence-resident path the update also writes the next step's fragment-ordered weight copies into ws, so that step may pass
// GT_STEP_PACKS_CURRENT; elsewhere (or with zero_grads == 0) it is gt_optimizer_step.
extern "C" int gt_optimizer_step_ws(const gt_config* cfg, int algo, float* params, float* grads, float* m, float* v, float* ws,
                                    gt_step_state* state, int zero_grads, gt_stream_t stream) {
  if (check_cfg(cfg)) return -1;
  PLayout P = param_layout(*cfg);
  if (!use_seq(*cfg) || !zero_grads || !ws) {
    unsigned* err = ws ? xchg_err(ws_layout(*cfg), ws) : nullptr;
    return optimizer_step_impl(algo, params, grads, m, v, P.total, state, zero_grads, stream, 0, err, 1);
  }
  if (!params || !grads || !state) return gt_fail("gt_optimizer_step: params / grads / state must not be NULL");
  Ctx x;
  if (make_ctx(x, cfg, params, grads, ws, state, 1, stream)) return -1;
  if (seq_update_pack(x, algo, params, m, v, nullptr, nullptr, nullptr, state, 0)) return -1;
  gt_launch(step_inc_kernel, dim3(1), dim3(64), (hipStream_t)stream, state, xchg_err(x.W, ws),
            (const float*)(grads + P.total - 1));
  return launch_status(x, "gt_optimizer_step_ws");
}
// ------------------------------------------------------------------------------------ fused train step
// Where a fused step's loss comes from.  gt_train_step (by_opts false): the hit penalty -- the loss may ride in the forward's last launch,
// which may then run on into backward phase 0 (FwdStep).  gt_train_step_loss (include/groove_hip.h): the loss as a launch of its own -- none
// is handed over, so the forward runs exactly as gt_forward's and loss_ex_kernel writes d loss / d logits into ws.dlogits.
struct StepLoss { bool by_opts; float penalty; const gt_loss_opts* lo; float* voice_stats; float* scratch; };
// The one body of gt_train_step / gt_train_step_loss (`who`: the entry point, for its error messages).  One context and one plan for
// the whole call; what the forward hands to the backward travels in `fs`, on this frame.
static int train_step_impl(const char* who, const gt_config* cfg, int algo, float* params, float* grads, float* m, float* v,
                           const float* pe, const float* xin, const float* y, const StepLoss& loss, float* hvo_out, float* stats,
                           float* tgt_scratch, float* ws, gt_step_state* state, int skip_update, gt_stream_t stream) {
  if (check_cfg(cfg)) return -1;
  if (!y || !state) return gt_fail("%s: y / state must not be NULL", who);
  if (skip_update < 0 || skip_update > 7) return gt_fail("%s: skip_update %d outside 0..7", who, skip_update);
  const bool packs_current = (skip_update & GT_STEP_PACKS_CURRENT) != 0;
  skip_update &= 3;
  const float* tgt_in = nullptr;
  if (cfg->n_dec_layers > 0) {
    if (!tgt_scratch) return gt_fail("%s: encoder-decoder model needs tgt_scratch", who);
    tgt_in = tgt_scratch;
  }
  Ctx x;
  if (make_ctx(x, cfg, params, grads, ws, state, 1, stream)) return -1;
  x.plan = seq_plan(x.c);
  if (skip_update == 3)                             // second half of a bucketed backward (tgt_scratch still holds the shifted y)
    return backward_impl(std::move(x), xin, tgt_in, hvo_out, nullptr, 1, 2, nullptr, false, false);
  // everything is checked before the first launch
  if (!stats || !hvo_out || (loss.by_opts && !loss.scratch))
    return gt_fail("%s: hvo_out / stats%s must not be NULL", who, loss.by_opts ? " / loss_scratch" : "");
  if (loss.by_opts && loss_opts_check(who, loss.lo)) return -1;
  const int M = x.M;
  if (tgt_in) gt_launch(shift_right_kernel, dim3((M * GT_TGT + 255) / 256), dim3(256), x.s, y, tgt_scratch, M * GT_TGT);
  // the launch that runs the output layer computes the loss as well where it can (one launch less): the sequence-resident launches
  // always, one kernel per op where the OutputLayer runs on heads_fwd_kernel -- fs.loss_done says whether it did
  unsigned* ticket = reinterpret_cast<unsigned*>(&state->pad2[0]);
  FwdStep fs = {nullptr, 0.f, nullptr, nullptr, packs_current, false, false};
  if (!loss.by_opts) { fs.y = y; fs.penalty = loss.penalty; fs.stats = stats; fs.ticket = ticket; }
  if (forward_impl(x, pe, xin, tgt_in, hvo_out, &fs)) return -1;
  if (loss.by_opts) {
    loss_ex_launch(x.c, hvo_out, y, *loss.lo, stats, loss.voice_stats, ws + x.W.dlogits, true, loss.scratch, x.s);
  } else if (!fs.loss_done) {
    // loss + head-activation backward in one kernel: d loss / d logits straight into ws.dlogits; workgroup partials are
    // combined by the last-arriving workgroup (ticket in the step state), so there is no memset node and the stats are
    // bitwise reproducible.  grads: zero on entry (precondition), re-zeroed by the optimizer kernel.
    gt_prof_tag("loss", 0, 12.0 * M * GT_TGT);
    gt_launch(loss_kernel<true, true>, dim3((M * GT_VOICES + 255) / 256), dim3(256), x.s, (const float*)hvo_out, y, loss.penalty, stats,
              ws + x.W.dlogits, M, ws + x.W.loss_part, ticket);
  }
  // whole step: the last launch of backward (the LayerNorm partials reduce -- every model has LayerNorms) also advances the
  // step counters, and the optimizer is told so: one launch less than update + step_inc
  if (backward_impl(x, xin, tgt_in, hvo_out, nullptr, 1, skip_update == 2 ? 1 : 0, skip_update == 0 ? state : nullptr, true, fs.b0_done))
    return -1;
  if (skip_update) return 0;
  // the update that ends a whole step: the last launch of backward advanced the step counters already
  if (!x.plan.seq) return optimizer_step_impl(algo, params, grads, m, v, x.P.total, state, 1, stream, 1, xchg_err(x.W, ws), 1) ? -1 : 0;
  if (seq_update_pack(x, algo, params, m, v, pe, xin, hvo_out, state, 1)) return -1;
  return launch_status(x, who);
}
extern "C" int gt_train_step(const gt_config* cfg, int algo, float* params, float* grads, float* m, float* v, const float* pe,
                             const float* xin, const float* y, float hit_loss_penalty, float* hvo_out, float* stats,
                             float* tgt_scratch, float* ws, gt_step_state* state, int skip_update, gt_stream_t stream) {
  const StepLoss loss = {false, hit_loss_penalty, nullptr, nullptr, nullptr};
  return train_step_impl("gt_train_step", cfg, algo, params, grads, m, v, pe, xin, y, loss, hvo_out, stats, tgt_scratch, ws, state,
                         skip_update, stream);
}
extern "C" int gt_train_step_loss(const gt_config* cfg, int algo, float* params, float* grads, float* m, float* v, const float* pe,
                                  const float* xin, const float* y, const gt_loss_opts* lo, float* voice_stats, float* loss_scratch,
                                  float* hvo_out, float* stats, float* tgt_scratch, float* ws, gt_step_state* state, int skip_update,
                                  gt_stream_t stream) {
  const StepLoss loss = {true, 0.f, lo, voice_stats, loss_scratch};
  return train_step_impl("gt_train_step_loss", cfg, algo, params, grads, m, v, pe, xin, y, loss, hvo_out, stats, tgt_scratch, ws, state,
                         skip_update, stream);
}

// ------------------------------------------------------------------------------------ data-parallel guard element
// grads[n_floats - 1] = (error word of this workspace's in-launch exchange region set ? 1 : 0): what a data-parallel host enqueues between the
// backward and the gradient all-reduce, so that the flag rides the collective and every rank's update kernel skips together.  One tiny launch
// (a no-op for shapes without such a region).
__global__ __launch_bounds__(64) void dp_guard_kernel(float* guard, const unsigned* err) { if (threadIdx.x == 0) *guard = (*err != 0u) ? 1.0f : 0.0f; }
extern "C" int gt_dp_guard(const gt_config* cfg, float* grads, const float* ws, gt_stream_t stream) {
  if (check_cfg(cfg)) return -1;
  if (!grads || !ws) return gt_fail("gt_dp_guard: grads / ws must not be NULL");
  const unsigned* err = xchg_err(ws_layout(*cfg), ws);
  if (!err) return 0;
  const PLayout P = param_layout(*cfg);
  gt_launch(dp_guard_kernel, dim3(1), dim3(64), (hipStream_t)stream, grads + P.total - 1, err);
  return launch_status("gt_dp_guard");
}

// ------------------------------------------------------------------------------------ global-norm gradient clipping
// Two launches over the whole flat gradient buffer but its guard element (gt_misc.h grad_norm_kernel / grad_scale_kernel), one workgroup
// per GT_CLIP_CHUNK floats.  scratch = one partial per workgroup, then the ticket word; left all-zero by every call.
extern "C" int64_t gt_clip_grad_norm_scratch_floats(const gt_config* cfg) {
  if (check_cfg(cfg)) return 0;
  return gt_clip_wgs(param_layout(*cfg).total) + 1;
}
extern "C" int gt_clip_grad_norm(const gt_config* cfg, float* grads, const gt_step_state* state, float max_norm, float* out, float* scratch,
                                 gt_stream_t stream) {
  if (check_cfg(cfg)) return -1;
  if (!grads || !state || !out || !scratch) return gt_fail("gt_clip_grad_norm: grads / state / out / scratch must not be NULL");
  if (!(max_norm > 0.f)) return gt_fail("gt_clip_grad_norm: max_norm %g must be > 0 (+inf: measure only)", (double)max_norm);
  const int64_t n = param_layout(*cfg).total, nwg = gt_clip_wgs(n);
  hipStream_t s = (hipStream_t)stream;
  gt_prof_tag("clip_norm", 2.0 * (n - 1), 4.0 * (n - 1));
  gt_launch(grad_norm_kernel, dim3((unsigned)nwg), dim3(256), s, (const float*)grads, n, state, max_norm, out, scratch,
            reinterpret_cast<unsigned*>(scratch + nwg));
  gt_prof_tag("clip_scale", 1.0 * (n - 1), 8.0 * (n - 1));
  gt_launch(grad_scale_kernel, dim3((unsigned)nwg), dim3(256), s, grads, n, (const float*)out);
  return launch_status("gt_clip_grad_norm");
}

// ------------------------------------------------------------------------------------ optimizer extras: the pass before the update
// SGD momentum / Nesterov / weight decay, Adam's L2 weight decay and AdamW as ONE launch (gt_misc.h opt_prepare_kernel) that rewrites the
// gradient buffer (AdamW: the parameter buffer) in front of the unchanged update.  The hyper-parameters are read from the host struct here
// and baked into the launch, as gt_clip_grad_norm's max_norm is; lr and grad_scale are read on the device.  ws != NULL: the predicate of
// gt_optimizer_step_ws (error word, guard element); ws == NULL: plain, like gt_optimizer_step.  Never touches step / opt_step.
extern "C" int gt_optimizer_prepare(const gt_config* cfg, int algo, float* params, float* grads, float* mbuf, const float* ws,
                                    const gt_step_state* state, const gt_opt_hparams* hp, gt_stream_t stream) {
  if (check_cfg(cfg)) return -1;
  if (!params || !grads || !state || !hp) return gt_fail("gt_optimizer_prepare: params / grads / state / hp must not be NULL");
  if (algo != 0 && algo != 1) return gt_fail("optimizer algo %d unknown (0 = sgd, 1 = adam)", algo);
  if (!(hp->weight_decay >= 0.f) || !(hp->momentum >= 0.f))
    return gt_fail("gt_optimizer_prepare: weight_decay %g / momentum %g must be >= 0", (double)hp->weight_decay, (double)hp->momentum);
  if (algo == 1 && hp->momentum != 0.f) return gt_fail("gt_optimizer_prepare: momentum belongs to sgd (algo 0), not to adam");
  if (algo == 0 && hp->decoupled) return gt_fail("gt_optimizer_prepare: decoupled weight decay (AdamW) belongs to adam (algo 1), not to sgd");
  if (hp->nesterov && hp->momentum == 0.f) return gt_fail("gt_optimizer_prepare: nesterov needs a momentum > 0");
  if (hp->momentum != 0.f && !mbuf) return gt_fail("gt_optimizer_prepare: momentum needs mbuf");
  if (hp->weight_decay == 0.f && hp->momentum == 0.f) return 0;      // nothing to do: no launch
  const int64_t n = param_layout(*cfg).total, nwg = gt_prep_wgs(n);
  if (nwg <= 0) return 0;
  const OptPrep h{hp->weight_decay, hp->momentum, hp->nesterov ? 1 : 0, algo == 0 ? 0 : (hp->decoupled ? 2 : 1)};
  const unsigned* err = ws ? xchg_err(ws_layout(*cfg), ws) : nullptr;
  const double bytes = h.mode == 2 ? 8.0 : 8.0 + (h.wd != 0.f ? 4.0 : 0.0) + (h.mom != 0.f ? 8.0 : 0.0);
  gt_prof_tag("opt_prepare", (h.mode == 2 ? 1.0 : 6.0) * (n - 1), bytes * (n - 1));
  gt_launch(opt_prepare_kernel, dim3((unsigned)nwg), dim3(256), (hipStream_t)stream, params, grads, mbuf, n, state, h, err, ws ? 1 : 0);
  return launch_status("gt_optimizer_prepare");
}

// ------------------------------------------------------------------------------------ test aid: hold CUs
// nblocks workgroups that each pin 96 KB of LDS (no 136 KB sequence workgroup fits beside one) and spin for `usec` microseconds of the
// 100 MHz constant clock: a second stream's kernel (an RCCL collective, an evaluation predict) holding CUs while a four-workgroups-per-
// sequence launch is in flight (tests/test_hip_api.py: the step must come out right, or the engine must say that it did not).
__global__ __launch_bounds__(64) void occupy_cus_kernel(int usec, unsigned* sink) {
  __shared__ unsigned hold[24 * 1024];
  hold[threadIdx.x] = threadIdx.x;
  __syncthreads();
#ifndef GT_EMU
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)usec * 100ull) __builtin_amdgcn_s_sleep(32);
#endif
  if (hold[(threadIdx.x + 1) & 63] == 0xFFFFFFFFu && sink) *sink = 1u;      // (keeps the array alive)
}
extern "C" int gt_debug_occupy_cus(int nblocks, int usec, gt_stream_t stream) {
  if (nblocks <= 0 || usec < 0) return gt_fail("gt_debug_occupy_cus: nblocks %d / usec %d", nblocks, usec);
  gt_launch(occupy_cus_kernel, dim3(nblocks), dim3(64), (hipStream_t)stream, usec, (unsigned*)nullptr);
  return launch_status("gt_debug_occupy_cus");
}

// ------------------------------------------------------------------------------------ evaluation metrics / input gather
extern "C" int64_t gt_voice_metrics_scratch_floats(int64_t n_rows) {
  return n_rows <= 0 ? 0 : ((n_rows + GT_VM_ROWS - 1) / GT_VM_ROWS) * GT_TGT;
}
extern "C" int gt_voice_metrics(const float* hvo_pred, const float* hvo_gt, int64_t n_rows, float* out30, float* scratch,
                                gt_stream_t stream) {
  if (!hvo_pred || !hvo_gt || !out30 || !scratch) return gt_fail("gt_voice_metrics: pointers must not be NULL");
  if (n_rows <= 0 || n_rows >= (1ll << 31)) return gt_fail("gt_voice_metrics: n_rows %lld out of range", (long long)n_rows);
  const int M = (int)n_rows, nwg = (M + GT_VM_ROWS - 1) / GT_VM_ROWS;
  hipStream_t s = (hipStream_t)stream;
  gt_launch(voice_metrics_partial_kernel, dim3(nwg), dim3(256), s, hvo_pred, hvo_gt, scratch, M);
  gt_launch(voice_metrics_final_kernel, dim3(1), dim3(64), s, (const float*)scratch, out30, nwg, M);
  return launch_status("gt_voice_metrics");
}
// Threshold curves (gt_curve.h): the counting pass as two launches, the choice as a pure host function.  The grid is read from the host
// array here and baked into the launch, as gt_predict_voices' thresholds are.
extern "C" int64_t gt_hit_curve_scratch_words(int64_t n_rows, int32_t n_thres) {
  if (n_rows <= 0 || n_rows >= (1ll << 31) || n_thres < 1 || n_thres > GT_CURVE_MAX_THRES) return 0;
  return (int64_t)gt_curve_wgs(n_rows) * GT_CURVE_CLASSES * (n_thres + 1);
}
extern "C" int gt_hit_curve(const float* prob, int32_t prob_stride, const float* hvo_gt, int64_t n_rows, const float* thres, int32_t n_thres,
                            uint64_t* counts, uint32_t* scratch, gt_stream_t stream) {
  if (!prob || !hvo_gt || !thres || !counts || !scratch) return gt_fail("gt_hit_curve: pointers must not be NULL");
  if (n_rows <= 0 || n_rows >= (1ll << 31)) return gt_fail("gt_hit_curve: n_rows %lld out of range", (long long)n_rows);
  if (prob_stride != GT_VOICES && prob_stride != GT_TGT)
    return gt_fail("gt_hit_curve: prob_stride %d (9 = a prob_out buffer, 27 = the hit columns of an HVO buffer)", (int)prob_stride);
  if (const char* e = gt_curve_grid_error(thres, n_thres)) return gt_fail("gt_hit_curve: %s (n_thres %d)", e, (int)n_thres);
  CurveGrid g;
  for (int k = 0; k <= GT_CURVE_PAD; ++k) g.t[k] = k < n_thres ? thres[k] : __builtin_inff();
  const int nb = n_thres + 1, keys = GT_CURVE_CLASSES * nb, nwg = gt_curve_wgs(n_rows);
  hipStream_t s = (hipStream_t)stream;
  gt_prof_tag("hit_curve", 0.0, (double)n_rows * GT_VOICES * 8.0);
  gt_launch(hit_curve_partial_kernel, dim3(nwg), dim3(GT_CURVE_THREADS), s, prob, (int)prob_stride, hvo_gt, n_rows, g, nb, (unsigned*)scratch);
  gt_prof_tag("hit_curve_sum", 0.0, (double)nwg * keys * 4.0 + keys * 16.0);
  gt_launch(hit_curve_sum_kernel, dim3((keys + GT_CURVE_THREADS - 1) / GT_CURVE_THREADS), dim3(GT_CURVE_THREADS), s, (const unsigned*)scratch, nwg,
            keys, counts);
  return launch_status("gt_hit_curve");
}
// Per-group evaluation counts (gt_group.h): two launches; the accumulator variant (4 / 16 / 64 groups of LDS) follows n_groups.
extern "C" int64_t gt_group_metrics_scratch_words(int64_t n_seq, int32_t n_groups) {
  if (n_seq <= 0 || n_seq >= (1ll << 26) || n_groups < 1 || n_groups > GT_GM_MAX_GROUPS) return 0;
  return (int64_t)gt_gm_wgs(n_seq, n_groups) * GT_GM_ACC_WORDS(n_groups);
}
extern "C" int gt_group_metrics(const float* hvo_pred, const float* hvo_gt, const int32_t* group, const uint32_t* cells, int64_t n_seq,
                                int32_t n_groups, uint64_t* acc, uint32_t* seq_out, uint64_t* scratch, gt_stream_t stream) {
  if (!hvo_pred || !hvo_gt || !acc || !scratch) return gt_fail("gt_group_metrics: hvo_pred / hvo_gt / acc / scratch must not be NULL");
  if (n_seq <= 0 || n_seq >= (1ll << 26)) return gt_fail("gt_group_metrics: n_seq %lld out of range", (long long)n_seq);
  if (n_groups < 1 || n_groups > GT_GM_MAX_GROUPS)
    return gt_fail("gt_group_metrics: n_groups %d outside 1..%d", (int)n_groups, GT_GM_MAX_GROUPS);
  const int nwg = gt_gm_wgs(n_seq, n_groups), words = GT_GM_ACC_WORDS(n_groups), variant = gt_gm_variant(n_groups);
  hipStream_t s = (hipStream_t)stream;
  gt_prof_tag("group_metrics", 0.0, (double)n_seq * (2.0 * 32 * GT_TGT * 4.0 + (group ? 4.0 : 0.0) + (cells ? 4.0 * GT_VOICES : 0.0) +
                                                     (seq_out ? 16.0 : 0.0)) + (double)nwg * words * 8.0);
  auto* kern = variant == 4 ? group_metrics_partial_kernel<4> : variant == 16 ? group_metrics_partial_kernel<16>
                                                                              : group_metrics_partial_kernel<GT_GM_MAX_GROUPS>;
  gt_launch(kern, dim3(nwg), dim3(GT_GM_THREADS), s, hvo_pred, hvo_gt, group, cells, n_seq, (int)n_groups, scratch, seq_out);
  gt_prof_tag("group_metrics_sum", 0.0, (double)nwg * words * 8.0 + words * 16.0);
  gt_launch(group_metrics_sum_kernel, dim3((words + GT_GM_SUM_WORDS - 1) / GT_GM_SUM_WORDS), dim3(GT_GM_THREADS), s, (const uint64_t*)scratch,
            nwg, words, acc);
  return launch_status("gt_group_metrics");
}
// Groove descriptors and rhythmic distances per sequence (gt_groove.h): one launch, every output word stored by one thread.
extern "C" int gt_groove_features(const float* hvo_a, const float* hvo_b, int64_t n_seq, uint64_t* feat_a, uint64_t* feat_b, uint64_t* pair,
                                  gt_stream_t stream) {
  if (!hvo_a || !feat_a) return gt_fail("gt_groove_features: hvo_a / feat_a must not be NULL");
  if (n_seq <= 0 || n_seq >= (1ll << 26)) return gt_fail("gt_groove_features: n_seq %lld out of range", (long long)n_seq);
  if (!hvo_b && (feat_b || pair)) return gt_fail("gt_groove_features: feat_b / pair need hvo_b");
  if (((uintptr_t)hvo_a | (uintptr_t)hvo_b) & 15u) return gt_fail("gt_groove_features: hvo_a / hvo_b must be 16-byte aligned");
  if (((uintptr_t)feat_a | (uintptr_t)feat_b | (uintptr_t)pair) & 7u) return gt_fail("gt_groove_features: feat_a / feat_b / pair must be 8-byte aligned");
  const bool has_b = hvo_b && (feat_b || pair);
  gt_prof_tag("groove_features", 0.0, (double)n_seq * ((has_b ? 2.0 : 1.0) * 32 * GT_TGT * 4.0 +
                                                       8.0 * (GT_GF_WORDS * (feat_b ? 2.0 : 1.0) + (pair ? GT_GF_PAIR_WORDS : 0.0))));
  gt_launch(groove_features_kernel, dim3(gt_gf_wgs(n_seq)), dim3(GT_GF_THREADS), (hipStream_t)stream, hvo_a, hvo_b, n_seq, feat_a, feat_b, pair);
  return launch_status("gt_groove_features");
}
extern "C" int gt_hit_thresholds(const uint64_t* counts_host, const float* thres, int32_t n_thres, const gt_threshold_rule* rule,
                                 float* thres_out, int32_t* index_out, float* scores_out) {
  if (!counts_host || !thres || !rule || !thres_out || !index_out || !scores_out) return gt_fail("gt_hit_thresholds: pointers must not be NULL");
  if (const char* e = gt_curve_grid_error(thres, n_thres)) return gt_fail("gt_hit_thresholds: %s (n_thres %d)", e, (int)n_thres);
  if (rule->criterion != 0 && rule->criterion != 1) return gt_fail("gt_hit_thresholds: criterion %d (0 = F-beta, 1 = density)", (int)rule->criterion);
  if (rule->criterion == 0 && (!(rule->beta > 0.f) || __builtin_isinf(rule->beta)))
    return gt_fail("gt_hit_thresholds: beta %g must be > 0 and finite", (double)rule->beta);
  if (!(rule->fallback >= 0.f && rule->fallback <= 1.f)) return gt_fail("gt_hit_thresholds: fallback %g outside [0, 1]", (double)rule->fallback);
  const double b2 = (double)rule->beta * (double)rule->beta;
  const bool beta_ok = rule->beta > 0.f && !__builtin_isinf(rule->beta);      // (criterion 1 does not need one: its F-beta column is then 0)
  for (int c = 0; c < GT_VOICES; ++c) {
    uint64_t tp = 0, fp = 0, P = 0;
    const int k = gt_curve_choose(counts_host + (size_t)c * 2 * (n_thres + 1), n_thres, rule->criterion, b2, &tp, &fp, &P);
    float* sc = scores_out + 4 * c;
    index_out[c] = k;
    if (k < 0) {
      thres_out[c] = rule->fallback;
      sc[0] = sc[1] = sc[2] = sc[3] = 0.f;
      continue;
    }
    thres_out[c] = thres[k];
    sc[0] = tp + fp ? (float)((double)tp / (double)(tp + fp)) : 0.f;
    sc[1] = (float)((double)tp / (double)P);
    sc[2] = beta_ok ? (float)gt_curve_fbeta(b2, tp, P - tp, fp) : 0.f;
    sc[3] = (float)((double)(tp + fp) / (double)P);
  }
  return 0;
}
extern "C" int gt_gather_batch(const float* xs, const float* ys, const int64_t* idx, int64_t n_seq, int32_t batch, int32_t src_dim,
                               float* x, float* y, gt_stream_t stream) {
  if (!xs || !ys || !idx || !x || !y) return gt_fail("gt_gather_batch: pointers must not be NULL");
  if (batch <= 0 || src_dim <= 0 || n_seq <= 0) return gt_fail("gt_gather_batch: batch / src_dim / n_seq must be > 0");
  const int64_t n4 = (int64_t)batch * (32 * src_dim / 4 + 32 * GT_TGT / 4);
  gt_launch(gather_batch_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), (hipStream_t)stream, xs, ys, idx, x, y, (int)batch,
            (int)src_dim, n_seq);
  return launch_status("gt_gather_batch");
}
// The gather that also draws the infilling pair (gt_misc.h gather_infill_kernel).  The options are read from the host struct here and
// baked into the launch, as gt_optimizer_prepare's hyper-parameters are; seed and step are read on the device.
extern "C" int gt_gather_infill(const float* hvo_set, const int64_t* idx, int64_t n_seq, int32_t batch, const gt_infill_opts* io,
                                const gt_step_state* state, float* x, float* y, int32_t* removed, gt_stream_t stream) {
  if (!hvo_set || !idx || !io || !state || !x || !y) return gt_fail("gt_gather_infill: hvo_set / idx / io / state / x / y must not be NULL");
  if (batch <= 0 || n_seq <= 0) return gt_fail("gt_gather_infill: batch / n_seq must be > 0");
  if (io->voice_mask == 0 || (io->voice_mask & ~((1 << GT_VOICES) - 1)))
    return gt_fail("gt_gather_infill: voice_mask 0x%x must name at least one of the %d voices and no other bit", (unsigned)io->voice_mask, GT_VOICES);
  if (io->min_remove < 1 || io->max_remove < io->min_remove || io->max_remove > GT_VOICES)
    return gt_fail("gt_gather_infill: need 1 <= min_remove (%d) <= max_remove (%d) <= %d", (int)io->min_remove, (int)io->max_remove, GT_VOICES);
  InfillArgs a{io->voice_mask, io->min_remove, io->max_remove, {}};
  bool any = false;
  for (int k = 0; k <= io->max_remove - io->min_remove; ++k) {
    if (io->count_weight[k] < 0 || io->count_weight[k] > 1024)
      return gt_fail("gt_gather_infill: count_weight[%d] = %d outside 0..1024", k, (int)io->count_weight[k]);
    a.weight[k] = io->count_weight[k];
    any = any || io->count_weight[k] != 0;
  }
  if (!any) return gt_fail("gt_gather_infill: every count_weight of the sizes %d..%d is 0", (int)io->min_remove, (int)io->max_remove);
  gt_prof_tag("gather_infill", 0.0, (double)batch * (3.0 * 32 * GT_TGT * 4.0 + 12.0));
  gt_launch(gather_infill_kernel, dim3((unsigned)((batch + GT_GI_SEQ - 1) / GT_GI_SEQ)), dim3(GT_GI_THREADS), (hipStream_t)stream, hvo_set, idx,
            x, y, (int*)removed, (int)batch, n_seq, a, state);
  return launch_status("gt_gather_infill");
}
extern "C" int gt_infill_merge(const float* hvo_pred, const float* hvo_in, const int32_t* removed, int64_t n_seq, int32_t mode, float* hvo_out,
                               gt_stream_t stream) {
  if (!hvo_pred || !hvo_in || !hvo_out) return gt_fail("gt_infill_merge: hvo_pred / hvo_in / hvo_out must not be NULL");
  if (n_seq <= 0 || n_seq >= (1ll << 26)) return gt_fail("gt_infill_merge: n_seq %lld out of range", (long long)n_seq);
  if (mode != 0 && mode != 1) return gt_fail("gt_infill_merge: mode %d (0 = the reference's sum, 1 = the input's hits win whole)", (int)mode);
  const int64_t cells = n_seq * 32 * GT_VOICES;
  gt_prof_tag("infill_merge", 0.0, (double)n_seq * (3.0 * 32 * GT_TGT * 4.0 + (removed ? 4.0 : 0.0)));
  gt_launch(infill_merge_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), (hipStream_t)stream, hvo_pred, hvo_in, (const int*)removed,
            hvo_out, cells, (int)mode);
  return launch_status("gt_infill_merge");
}
// The gather that draws the event-level pair (gt_misc.h gather_infill_events_kernel): options from the host struct, baked into the launch;
// seed and step are read on the device.
extern "C" int gt_gather_infill_events(const float* hvo_set, const int64_t* idx, int64_t n_seq, int32_t batch, const gt_infill_event_opts* eo,
                                       const gt_step_state* state, float* x, float* y, uint32_t* cells, gt_stream_t stream) {
  if (!hvo_set || !idx || !eo || !state || !x || !y)
    return gt_fail("gt_gather_infill_events: hvo_set / idx / eo / state / x / y must not be NULL");
  if (batch <= 0 || n_seq <= 0) return gt_fail("gt_gather_infill_events: batch / n_seq must be > 0");
  if (eo->voice_mask == 0 || (eo->voice_mask & ~((1 << GT_VOICES) - 1)))
    return gt_fail("gt_gather_infill_events: voice_mask 0x%x must name at least one of the %d voices and no other bit", (unsigned)eo->voice_mask,
                   GT_VOICES);
  if (eo->ratio_lo < 0 || eo->ratio_hi > 65536 || eo->ratio_lo > eo->ratio_hi)
    return gt_fail("gt_gather_infill_events: need 0 <= ratio_lo (%d) <= ratio_hi (%d) <= 65536", (int)eo->ratio_lo, (int)eo->ratio_hi);
  const InfillEventArgs a{eo->voice_mask, (uint32_t)eo->ratio_lo, (uint32_t)(eo->ratio_hi - eo->ratio_lo + 1)};
  gt_prof_tag("gather_infill_events", 0.0, (double)batch * (3.0 * 32 * GT_TGT * 4.0 + 8.0 + 4.0 * GT_VOICES));
  gt_launch(gather_infill_events_kernel, dim3((unsigned)((batch + GT_GE_SEQ - 1) / GT_GE_SEQ)), dim3(GT_GE_THREADS), (hipStream_t)stream, hvo_set,
            idx, x, y, cells, (int)batch, n_seq, a, state);
  return launch_status("gt_gather_infill_events");
}
extern "C" int gt_infill_merge_cells(const float* hvo_pred, const float* hvo_in, const uint32_t* cells, int64_t n_seq, int32_t mode,
                                     float* hvo_out, gt_stream_t stream) {
  if (!hvo_pred || !hvo_in || !hvo_out) return gt_fail("gt_infill_merge_cells: hvo_pred / hvo_in / hvo_out must not be NULL");
  if (n_seq <= 0 || n_seq >= (1ll << 26)) return gt_fail("gt_infill_merge_cells: n_seq %lld out of range", (long long)n_seq);
  if (mode != 0 && mode != 1)
    return gt_fail("gt_infill_merge_cells: mode %d (0 = the reference's sum, 1 = the input's hits win whole)", (int)mode);
  if (!cells) return gt_infill_merge(hvo_pred, hvo_in, nullptr, n_seq, mode, hvo_out, stream);      // (the same launch: nothing is masked)
  const int64_t n_cells = n_seq * 32 * GT_VOICES;
  gt_prof_tag("infill_merge_cells", 0.0, (double)n_seq * (3.0 * 32 * GT_TGT * 4.0 + 4.0 * GT_VOICES));
  gt_launch(infill_merge_cells_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), (hipStream_t)stream, hvo_pred, hvo_in, cells, hvo_out,
            n_cells, (int)mode);
  return launch_status("gt_infill_merge_cells");
}

// ------------------------------------------------------------------------------------ predict
// vs != nullptr (gt_predict_voices): the per-voice head kernel decides and writes prob_out; thres / use_thres are then unused
static int predict_impl(const gt_config* cfg, const float* params, const float* pe, const float* xin, float* hvo_out, float thres,
                        int use_thres, uint32_t seed, float* tgt_scratch, float* ws, gt_stream_t stream, uint32_t idx0 = 0u,
                        const gt_voice_sampling* vs = nullptr, float* prob_out = nullptr);
extern "C" int gt_predict(const gt_config* cfg, const float* params, const float* pe, const float* xin, float* hvo_out, float thres,
                          int use_thres, float* tgt_scratch, float* ws, gt_stream_t stream) {
  return predict_impl(cfg, params, pe, xin, hvo_out, thres, use_thres != 0, 0u, tgt_scratch, ws, stream);
}
// model.predict(src, use_pd=True): hits sampled from the predicted probabilities (see predict_head_kernel); the encoder-decoder's
// greedy decode feeds the SAMPLED hits back, step by step
extern "C" int gt_predict_pd(const gt_config* cfg, const float* params, const float* pe, const float* xin, float* hvo_out, uint32_t seed,
                             float* tgt_scratch, float* ws, gt_stream_t stream) {
  return predict_impl(cfg, params, pe, xin, hvo_out, 0.5f, 2, seed, tgt_scratch, ws, stream);
}
// ... for a chunk of a larger set: first_seq = index of the chunk's first sequence inside the set.  The uniform of element (row, column)
// is hashed from its index in the WHOLE set, so the samples do not depend on how the set is cut into calls.
extern "C" int gt_predict_pd_at(const gt_config* cfg, const float* params, const float* pe, const float* xin, float* hvo_out, uint32_t seed,
                                int64_t first_seq, float* tgt_scratch, float* ws, gt_stream_t stream) {
  if (first_seq < 0) return gt_fail("gt_predict_pd_at: first_seq must be >= 0");
  return predict_impl(cfg, params, pe, xin, hvo_out, 0.5f, 2, seed, tgt_scratch, ws, stream, (uint32_t)((uint64_t)first_seq * 32u * GT_TGT));
}
static int predict_impl(const gt_config* cfg, const float* params, const float* pe, const float* xin, float* hvo_out, float thres,
                        int use_thres, uint32_t seed, float* tgt_scratch, float* ws, gt_stream_t stream, uint32_t idx0,
                        const gt_voice_sampling* vs, float* prob_out) {
  Ctx x;
  if (make_ctx(x, cfg, params, nullptr, ws, nullptr, 0, stream)) return -1;
  if (!pe || !xin || !hvo_out) return gt_fail("gt_predict: pe / x / hvo_out must not be NULL");
  const int M = x.M, B = cfg->batch;
  VoiceHeadArgs va{};
  if (vs) {
    for (int c = 0; c < GT_VOICES; ++c) va.thres[c] = vs->thres[c];
    va.temperature = vs->temperature;
    va.mode = vs->mode;
  }
  if (encoder_fwd(x, pe, xin)) return -1;
  if (cfg->n_dec_layers == 0) {
    output_layer_fwd(x, hvo_out);
    if (vs)
      gt_launch(predict_voices_head_kernel, dim3((M * GT_TGT + 255) / 256), dim3(256), x.s, (const float*)hvo_out, hvo_out, (float*)nullptr,
                prob_out, va, -1, B, seed, idx0);
    else
      gt_launch(predict_head_kernel, dim3((M * GT_TGT + 255) / 256), dim3(256), x.s, (const float*)hvo_out, hvo_out, (float*)nullptr,
                thres, use_thres, -1, B, seed, idx0);
    return launch_status(x, vs ? "gt_predict_voices" : "gt_predict");
  }
  if (!tgt_scratch) return gt_fail("gt_predict: encoder-decoder model needs tgt_scratch");
  // greedy decode: tgt row 0 = zeros, row t+1 = thresholded step t.  The encoder memory and every layer's cross-attention
  // K/V are computed once; step t then touches only row t of each sequence (decoder_step; the self-attention K/V rows of
  // the earlier steps are the cache).
  float* tmp = ws + x.W.hvo_tmp;
  (void)hipMemsetAsync(tgt_scratch, 0, (size_t)M * GT_TGT * sizeof(float), x.s);
  const int d = x.d, L = cfg->n_enc_layers;
  for (int l = 0; l < cfg->n_dec_layers; ++l) {
    const LayerP& p = x.P.dec[l];
    const LayerW& w = x.W.layers[L + l];
    linear_fwd(x, ws + x.W.memory, d, x.prm + p.xa.in_w + (int64_t)d * d, x.prm + p.xa.in_b + d, ws + w.kvx, 2 * d, 2 * d, d);
  }
  for (int t = 0; t < 32; ++t) {
    decoder_step(x, pe, tgt_scratch, t, tmp);
    if (vs)
      gt_launch(predict_voices_head_kernel, dim3((B * GT_TGT + 255) / 256), dim3(256), x.s, (const float*)tmp, hvo_out, tgt_scratch,
                prob_out, va, t, B, seed, idx0);
    else
      gt_launch(predict_head_kernel, dim3((B * GT_TGT + 255) / 256), dim3(256), x.s, (const float*)tmp, hvo_out, tgt_scratch, thres,
                use_thres, t, B, seed, idx0);
  }
  return launch_status(x, vs ? "gt_predict_voices" : "gt_predict");
}

// ---- per-voice controls: thresholds, temperature, hit caps, velocity / offset mask (include/groove_hip.h, gt_voice_sampling) ----
static int voice_sampling_check(const char* what, const gt_voice_sampling* vs) {
  if (!vs) return gt_fail("%s: vs must not be NULL", what);
  for (int c = 0; c < GT_VOICES; ++c) {
    if (!(vs->thres[c] >= 0.f && vs->thres[c] <= 1.f)) return gt_fail("%s: thres[%d] = %g outside [0, 1]", what, c, (double)vs->thres[c]);
    if (vs->max_count[c] < 0 || vs->max_count[c] > 32) return gt_fail("%s: max_count[%d] = %d outside 0..32", what, c, (int)vs->max_count[c]);
  }
  if (!(vs->temperature > 0.f) || __builtin_isinf(vs->temperature)) return gt_fail("%s: temperature %g must be > 0 and finite", what, (double)vs->temperature);
  if (vs->mode != 0 && vs->mode != 1) return gt_fail("%s: mode %d (0 = threshold, 1 = sampled)", what, (int)vs->mode);
  return 0;
}
// the cap / mask pass over n_seq sequences; launches nothing when it would change nothing
static void voice_select_launch(float* hvo, const float* prob, const gt_voice_sampling* vs, int n_seq, hipStream_t s) {
  VoiceSelectArgs va{};
  bool capped = false;
  for (int c = 0; c < GT_VOICES; ++c) {
    va.max_count[c] = vs->max_count[c];
    capped = capped || vs->max_count[c] < 32;
  }
  va.mask_vo = vs->mask_vo ? 1 : 0;
  if (!capped && !va.mask_vo) return;
  gt_prof_tag("voice_select", 0.0, (double)n_seq * 32 * 4.0 * (GT_TGT + GT_VOICES + (va.mask_vo ? GT_TGT : GT_VOICES)));
  gt_launch(voice_select_kernel, dim3((unsigned)((n_seq + GT_VS_SEQ - 1) / GT_VS_SEQ)), dim3(GT_VS_THREADS), s, hvo, prob, va, n_seq);
}
extern "C" int gt_voice_select(float* hvo, const float* prob, const gt_voice_sampling* vs, int64_t n_seq, gt_stream_t stream) {
  if (!hvo || !prob) return gt_fail("gt_voice_select: hvo / prob must not be NULL");
  if (voice_sampling_check("gt_voice_select", vs)) return -1;
  if (n_seq <= 0 || n_seq >= (1ll << 26)) return gt_fail("gt_voice_select: n_seq %lld out of range", (long long)n_seq);
  voice_select_launch(hvo, prob, vs, (int)n_seq, (hipStream_t)stream);
  return launch_status("gt_voice_select");
}
extern "C" int gt_predict_voices(const gt_config* cfg, const float* params, const float* pe, const float* xin, float* hvo_out,
                                 const gt_voice_sampling* vs, uint32_t seed, int64_t first_seq, float* prob_out, float* tgt_scratch,
                                 float* ws, gt_stream_t stream) {
  if (voice_sampling_check("gt_predict_voices", vs)) return -1;
  if (!prob_out) return gt_fail("gt_predict_voices: prob_out must not be NULL");
  if (first_seq < 0) return gt_fail("gt_predict_voices: first_seq must be >= 0");
  if (cfg && cfg->n_dec_layers > 0 && !tgt_scratch) return gt_fail("gt_predict_voices: encoder-decoder model needs tgt_scratch");
  if (predict_impl(cfg, params, pe, xin, hvo_out, 0.5f, 1, seed, tgt_scratch, ws, stream, (uint32_t)((uint64_t)first_seq * 32u * GT_TGT), vs,
                   prob_out))
    return -1;
  voice_select_launch(hvo_out, prob_out, vs, cfg->batch, (hipStream_t)stream);
  return launch_status("gt_predict_voices");
}

