// The run-time switches of the host code: ONE table, one resolution rule, one accessor.
//   gt_switch(id)   the setter's value while it is set, else the environment variable's -- read once per process, at the switch's first use --
//                   else the default.
// A setter (include/groove_hip_debug.h) is one gt_switch_set into its row; a negative argument means "unset" for every one of them.  The rules
// of groove_hip.hip / gt_gemm.h / gt_gemm64.h ask gt_switch and nothing else: no rule has a global or a getenv of its own.  Not here, because
// they are read live on purpose (a test switches them inside a running process): GT_TRACE_DISPATCH, GT_TRACE_GEMM64, GT_TRACE_HEADS, GT_EMU_DRY.
#pragma once
#include <limits.h>
#include <stdlib.h>

// how a row's environment text becomes its value
enum GtSwitchText {
  GT_SW_NO_ENV,     // setter only
  GT_SW_NOT0,       // 0 if the text begins with '0', else 1
  GT_SW_IS1,        // 1 if the text begins with '1', else 0
  GT_SW_LEVEL,      // one digit '0' .. '2'; any other text counts as unset
  GT_SW_LONG        // atol; the empty text counts as unset
};
constexpr long GT_SW_UNSET = LONG_MIN;
constexpr long GT_SW_BY_RULE = -1;       // default of the rows whose rule decides by shape / by its own macro while nothing is set
enum GtSwitch {
  GT_SW_SEQ, GT_SW_SEQ_SPLIT, GT_SW_SEQ_RIDE, GT_SW_SEQ_QUAD, GT_SW_LN_XCHG, GT_SW_LN_XCHG128, GT_SW_LN_XCHG32, GT_SW_FFN_KBITS, GT_SW_SEQ_QUAD_PRO,
  GT_SW_ATTN_BWD_LDS_MIN, GT_SW_DETERMINISTIC, GT_SW_OPERAND_SHADOWS, GT_SW_XCHG_SPIN_MAX, GT_SW_WGRAD128_MIN_CHUNK, GT_SW_WGRAD128H_MIN_CHUNK,
  GT_SW_T64R_MIN, GT_SW_T64R_MAX, GT_SW_T64H_MAX, GT_SW_LN128_MIN, GT_SW_LN32_MIN, GT_SW_COUNT
};
struct GtSwitchRow { GtSwitch id; const char* env; GtSwitchText text; long dflt; };
// (GT_SW_BY_RULE rows: the asking rule passes its default -- a shape rule's "by shape", a threshold's -D macro -- to gt_switch's second argument)
inline constexpr GtSwitchRow gt_switch_rows[GT_SW_COUNT] = {
  // id                        environment                 text          default              setter; values
  {GT_SW_SEQ,                  "GT_SEQ",                   GT_SW_NOT0,   GT_SW_BY_RULE},   // gt_set_seq; 0 off, 1 every supported shape, unset: by measurement
  {GT_SW_SEQ_SPLIT,            "GT_SEQ_SPLIT",             GT_SW_NOT0,   GT_SW_BY_RULE},   // gt_set_seq_split; 0 / 1, unset: by shape
  {GT_SW_SEQ_RIDE,             "GT_SEQ_RIDE",              GT_SW_NOT0,   GT_SW_BY_RULE},   // gt_set_seq_ride; 0 / 1, unset: by shape
  {GT_SW_SEQ_QUAD,             "GT_SEQ_QUAD",              GT_SW_NOT0,   GT_SW_BY_RULE},   // gt_set_seq_quad; 0 / 1, unset: by shape
  {GT_SW_LN_XCHG,              "GT_LN_XCHG",               GT_SW_NOT0,   GT_SW_BY_RULE},   // gt_set_ln_exchange; 0 off, 1 forced, unset: where it applies
  {GT_SW_LN_XCHG128,           "GT_LN_XCHG128",            GT_SW_NOT0,   1},               // (A/B) the row exchange on the big tile
  {GT_SW_LN_XCHG32,            "GT_LN_XCHG32",             GT_SW_NOT0,   1},               // (A/B) the row exchange on 32x32 tiles
  {GT_SW_FFN_KBITS,            "GT_FFN_KBITS",             GT_SW_NOT0,   1},               // (A/B) keep bits of the FFN activation
  {GT_SW_SEQ_QUAD_PRO,         "GT_SEQ_QUAD_PRO",          GT_SW_IS1,    0},               // (A/B) QUAD forward's prologue launch
  {GT_SW_ATTN_BWD_LDS_MIN,     "GT_ATTN_BWD_LDS_MIN",      GT_SW_LONG,   GT_SW_BY_RULE},   // default: the macro of that name
  {GT_SW_DETERMINISTIC,        "GT_DETERMINISTIC",         GT_SW_IS1,    0},               // gt_set_deterministic; 0 / 1
  {GT_SW_OPERAND_SHADOWS,      "GT_BF16_SHADOWS",          GT_SW_LEVEL,  2},               // gt_set_operand_shadows; 0 .. 2
  {GT_SW_XCHG_SPIN_MAX,        nullptr,                    GT_SW_NO_ENV, 0},               // gt_set_xchg_spin_max; <= 0: the exchange's compiled bound
  {GT_SW_WGRAD128_MIN_CHUNK,   "GT_WGRAD128_MIN_CHUNK",    GT_SW_LONG,   GT_SW_BY_RULE},   // default: the macro of that name (and so below)
  {GT_SW_WGRAD128H_MIN_CHUNK,  "GT_WGRAD128H_MIN_CHUNK",   GT_SW_LONG,   GT_SW_BY_RULE},
  {GT_SW_T64R_MIN,             "GT_T64R_MIN",              GT_SW_LONG,   GT_SW_BY_RULE},
  {GT_SW_T64R_MAX,             "GT_T64R_MAX",              GT_SW_LONG,   GT_SW_BY_RULE},
  {GT_SW_T64H_MAX,             "GT_T64H_MAX",              GT_SW_LONG,   GT_SW_BY_RULE},
  {GT_SW_LN128_MIN,            "GT_LN128_MIN",             GT_SW_LONG,   GT_SW_BY_RULE},
  {GT_SW_LN32_MIN,             "GT_LN32_MIN",              GT_SW_LONG,   GT_SW_BY_RULE},   // default: half the CUs (tests lower it: the emulator runs small shapes)
};
constexpr bool gt_switch_rows_in_order(int i = 0) { return i == GT_SW_COUNT || (gt_switch_rows[i].id == i && gt_switch_rows_in_order(i + 1)); }
static_assert(gt_switch_rows_in_order(), "gt_switch_rows: row i must describe GtSwitch i");

struct GtSwitchState { long set = GT_SW_UNSET, env = GT_SW_UNSET; bool env_read = false; };
inline GtSwitchState& gt_switch_state(GtSwitch id) { static GtSwitchState st[GT_SW_COUNT]; return st[id]; }
inline long gt_switch_text(GtSwitchText how, const char* e) {
  if (!e || how == GT_SW_NO_ENV) return GT_SW_UNSET;
  if (how == GT_SW_NOT0) return e[0] != '0';
  if (how == GT_SW_IS1) return e[0] == '1';
  if (how == GT_SW_LEVEL) return (e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : GT_SW_UNSET;
  return e[0] ? atol(e) : GT_SW_UNSET;
}
inline long gt_switch(GtSwitch id, long dflt) {
  GtSwitchState& s = gt_switch_state(id);
  if (s.set != GT_SW_UNSET) return s.set;
  if (!s.env_read) { s.env_read = true; s.env = gt_switch_text(gt_switch_rows[id].text, gt_switch_rows[id].env ? getenv(gt_switch_rows[id].env) : nullptr); }
  return s.env != GT_SW_UNSET ? s.env : dflt;
}
inline long gt_switch(GtSwitch id) { return gt_switch(id, gt_switch_rows[id].dflt); }
// the body of every setter: v < 0 = unset; _flag: any other non-zero argument = 1
inline int gt_switch_set(GtSwitch id, long v) { gt_switch_state(id).set = v < 0 ? GT_SW_UNSET : v; return 0; }
inline int gt_switch_set_flag(GtSwitch id, int on) { return gt_switch_set(id, on < 0 ? -1 : on != 0); }
