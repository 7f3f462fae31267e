/* groove_hip_debug.h -- the PROCESS-WIDE run-time switches and the test / measurement aids of libgroove_hip.so.  Not part of the contract
 * (groove_hip.h): a host that trains or predicts needs none of them -- the library's defaults are the measured schedules, and the per-caller
 * switches are gt_config.flags.  Tests, benchmarks and A/B measurements use these.  Every gt_set_* is one write into its row of the switch
 * table (csrc/gt_switches.h): the setter's value holds while it is set, a NEGATIVE argument unsets it -- the environment variable of the row
 * (read once per process), else the default, answers again. */
#ifndef GROOVE_HIP_DEBUG_H
#define GROOVE_HIP_DEBUG_H
#include "groove_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Sequence-resident kernels (csrc/gt_seq.h): for encoder-only fp32 models with d_model <= 128 (% 16), dim_feedforward <= 512
 * (% 16), src_dim <= 32 and head_dim 16 / 32 / 64 or below 16, ONE workgroup per sequence runs the whole forward (and one the
 * whole backward) in a single launch -- or, in the SPLIT mode below, two workgroups per sequence and one launch per layer and
 * direction; gt_step_launches() gives the launch count of a train step.  Default (neither this call nor env GT_SEQ): d_model <= 64
 * and d_model == 128 always, the other widths of the 128 class from batch 64 up.  on = 1 forces them wherever supported, on = 0
 * switches them off (env GT_SEQ=1 / GT_SEQ=0 do the same), -1 = default.  Same results as the one-kernel-per-op path to fp32 rounding. */
int gt_set_seq(int on);
/* Two workgroups per sequence (16 token rows each) and one launch per layer and direction for the sequence-resident kernels at
 * d_model 128 or 32: -1 = default (when 2 x batch workgroups fit the CUs once; d_model 32 only with dim_feedforward >= 256), 0 = off,
 * 1 = on (env GT_SEQ_SPLIT=0/1 does the same).  Same results bit for bit: the split is over token rows. */
int gt_set_seq_split(int on);
/* FOUR workgroups per sequence in the forward of the SPLIT mode at d_model 128 (csrc/gt_seq.h, QUAD): the two workgroups of a 16-row
 * half are column partners that each compute half of dim_feedforward and swap their partial FFN2 results through one in-launch pair
 * exchange per layer (8-byte tagged granules, agent-scope stores / loads) -- the forward then fills 4 x batch CUs instead of 2 x batch.
 * -1 = default (whenever 4 x batch workgroups fit the CUs at once and dim_feedforward % 32 == 0), 0 = off, 1 = on under the same
 * condition (env GT_SEQ_QUAD=0/1).  Results agree with the SPLIT mode to fp32 rounding (the FFN2 contraction is summed as two halves);
 * bitwise repeatable run to run.  Needs gt_workspace_init on the workspace. */
int gt_set_seq_quad(int on);
/* Polls of an in-launch exchange (groove_hip.h, "xchg_err") before a workgroup gives its partner up (<= 0: the default, 2^22 = seconds;
 * tests lower it to see the time-out path). */
int gt_set_xchg_spin_max(int polls);
/* LayerNorm inside the producing Linear / dgrad (csrc/gt_gemm64.h, round 5): at d_model 256 / 512, where the 64 x 64-tile kernels apply and
 * the whole grid is resident at once (a GPU's share of a data-parallel batch: 2048 tokens), the N / 64 workgroups of a row block exchange
 * their row partials inside the launch (tagged 8-byte granules, agent-scope stores / polling loads; "rowx" workspace region, zeroed once
 * by gt_workspace_init) and each normalises its own tile -- no row pass of its own.  -1 = default (on where it applies: 3/4 .. 2 tiles of 64 x 64 per CU), 0 = off (env GT_LN_XCHG=0): the norm as a
 * row pass of its own; 1-1.5 % of the step at 2048 tokens (csrc/groove_hip.hip, ln_xchg).  Same
 * bounded-spin / error-word / skipped-update contract as the pair exchange ("xchg_err" names the word of whichever a shape has). */
int gt_set_ln_exchange(int on);
/* Test aid: nblocks workgroups that each pin 96 KB of LDS (no sequence workgroup fits beside one) for `usec` microseconds -- a second
 * stream holding CUs while a four-workgroups-per-sequence launch is in flight. */
int gt_debug_occupy_cus(int nblocks, int usec, gt_stream_t stream);
/* gt_config.precision = 1 (BASELINE configs[4]) at d_model 256 / 512 with every Linear of a layer on the big-tile kernel: bf16 copies of
 * the GEMM operands.  The producers of every activation / gradient a Linear, dgrad or weight gradient of an encoder layer consumes write
 * it in bf16 (8 tensors per layer), a per-step kernel writes bf16 copies of the layers' weights and of their transposes, and the GEMMs
 * stage those (csrc/gt_gemm32.h gemm32h_kernel: half the bytes per flop).  level 1: the copies sit BESIDE the fp32 tensors; level 2 (the
 * default): the tensors nothing but a GEMM reads -- ctx, hact, dhid, dqkv, the dropout-masked dz copies -- are stored in bf16 ALONE (the
 * reference's torch autograd keeps the same intermediates, in fp32: nothing of its interface sees them).  0: off.  -1: the environment
 * (GT_BF16_SHADOWS=0/1/2) or the default.  Outputs, losses and gradients are bit-identical at every level.  Changes gt_workspace_bytes and
 * which gt_ws_find names are live: set it before sizing a workspace (gt_layout_epoch, gt_operand_shadow_level: groove_hip.h). */
int gt_set_operand_shadows(int level);
/* Weight gradients as RIDER workgroups (csrc/gt_seq_wg.h): in the SPLIT mode at d_model 128 the backward phases' launches carry, on
 * the CUs their 2 x batch sequence workgroups leave idle, the weight gradients whose operands the earlier phases completed; one
 * workgroup owns a 32 x 64 gradient tile over ALL tokens (no atomics: bitwise reproducible), and a tail launch does what cannot ride
 * (layer 0's in-proj, the input layer), the LayerNorm parameter gradients and the step-counter bump.  -1 = default (when at least 64
 * CUs are idle beside the sequence workgroups), 0 = off (the grouped dispatch at the end of backward), 1 = on wherever supported
 * (env GT_SEQ_RIDE=0/1 does the same).  Same results to fp32 rounding (another summation order over the tokens). */
int gt_set_seq_ride(int on);
/* Measurement aid (tools/wg_unit_bench.py): the rider units of backward phase `phase` as a launch of their own (token range split
 * `ksplit` ways), ADDING into grads; operands = what the last backward on this workspace left there. */
int gt_debug_seq_wg_phase(const gt_config* cfg, const float* params, float* grads, const float* x, float* ws, int phase, int ksplit,
                          gt_stream_t stream);
/* Bitwise-reproducible weight gradients: each output tile of a weight gradient is owned by ONE workgroup that walks all tokens
 * (no split over the token dimension), so the fp32 atomic adds have a single contributor per element.  Everything else of the
 * step is reproducible already (fixed-order reductions).  Off by default: the small shapes lose their token parallelism
 * (env GT_DETERMINISTIC=1 does the same; -1 = that, or off). */
int gt_set_deterministic(int on);

#ifdef __cplusplus
}
#endif
#endif /* GROOVE_HIP_DEBUG_H */
