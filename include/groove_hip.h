/* groove_hip.h -- C ABI of libgroove_hip.so: the MI355X (gfx950) hot path of the GrooveTransformer
 * train / predict step.
 *
 * The reference has no FFI: its hot path sits behind a *Python module API* supplied by the
 * un-vendored submodule `BaseGrooveTransformers` (ref:train.py:12 `initialize_model, calculate_loss,
 * train_loop`; ref:evaluator.py:173 `model.predict`).  Each entry point below names the reference
 * interface it replaces; INTEGRATION.md shows the ctypes stub a maintainer of the reference adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch caching allocator); the library
 *     never allocates, frees or synchronises; every call enqueues on the given hipStream_t and is
 *     hipGraph-capturable (no host reads of device data, no host-dependent launch parameters
 *     except the gt_config);
 *   - return value 0 = ok, <0 = error; gt_last_error() gives the message (thread-local);
 *   - activations are row-major (M, features), M = batch*32 rows, row m = b*32 + t -- the layout
 *     the reference's DataLoader hands over ((B,32,S) / (B,32,27) contiguous fp32,
 *     ref:dataset.py:263-264,355-356);
 *   - HVO tensors are (M,27) = [hits(9) | velocities(9) | offsets(9)] (ref:utils.py:38-47,
 *     ref:evaluator.py:173-177);
 *   - parameters live in ONE flat fp32 buffer in state-dict order (names = the demo checkpoint's keys,
 *     ref:demo/transformer_run_171tyqit_Epoch_1.Model); gt_param_layout() gives each tensor's offset.
 *     Gradients use the same layout in a second flat buffer (one RCCL all-reduce, one fused update).
 */
#ifndef GROOVE_HIP_H
#define GROOVE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* gt_stream_t;   /* a hipStream_t (ihipStream_t*), passed opaquely so C callers need no HIP headers */

#define GT_T 32          /* max_len, hard-coded by the reference: ref:train.py:128 */
#define GT_TGT 27        /* embedding_size_tgt: ref:train.py:132 */
#define GT_VOICES 9
#define GT_MAX_D 512     /* largest d_model in the reference's sweeps: ref:configs/InfillingClosedHH_sweep.yaml */

/* params["model"] of ref:train.py:115-134 */
typedef struct gt_config {
  int32_t batch;          /* sequences in this call (B) */
  int32_t src_dim;        /* embedding_size_src: 16 (MSO) or 27 (symbolic), ref:train.py:129-131 */
  int32_t d_model;
  int32_t n_heads;
  int32_t dim_ff;
  int32_t n_enc_layers;
  int32_t n_dec_layers;   /* 0 = encoder_only (ref:train.py:125-127) */
  float dropout;
  int32_t precision;      /* 0 = fp32 everywhere (the parity path).  1 = BASELINE configs[4]: the operands of every Linear's
                           * forward / dgrad / wgrad GEMM are rounded to bf16 (round-to-nearest-even) on their way into the
                           * matrix cores (v_mfma_f32_16x16x32_bf16, fp32 accumulate); master weights, activations in HBM,
                           * attention core, LayerNorm, softmax, loss and optimizer stay fp32.  Bias gradients are column sums
                           * of the bf16-rounded output gradient.
                           * 2 = bf16 where the bytes are (round 5): on top of 1, the Linear OUTPUTS of the encoder layers that
                           * torch.autocast(bfloat16) hands on as bf16 are stored in bf16 alone -- qkv (the attention kernels then do
                           * fp32 arithmetic on bf16-stored q / k / v), the out-proj / linear2 outputs ahead of their LayerNorm, the
                           * dgrad outputs ahead of a LayerNorm backward, dctx.  Residual stream, LayerNorm statistics, softmax, loss,
                           * master weights and optimizer stay fp32.  In force where the bf16 operand shadows apply at level 2 and
                           * the heads are 64 / 128 wide (gt_precision_in_force); elsewhere it runs as precision 1. */
  int32_t flags;          /* per-CALLER schedule switches (round 6; 0 = the library's defaults).  They select among schedules that give the same
                           * numbers, never change the workspace layout, and -- unlike gt_set_seq_quad / gt_set_ln_exchange, which are
                           * process-wide -- bind only the calls made with this gt_config: two engines in one process can differ.
                           * GT_CFG_NO_QUAD: no four-workgroups-per-sequence schedule (no in-launch pair exchange);
                           * GT_CFG_NO_LN_XCHG: no LayerNorm inside the Linears (no in-launch row exchange). */
} gt_config;
#define GT_CFG_NO_QUAD 1
#define GT_CFG_NO_LN_XCHG 2

/* device-resident per-step state, so that a captured hipGraph replays with fresh dropout masks,
 * Adam bias correction and learning rate without host-side kernel-argument changes */
typedef struct gt_step_state {
  uint32_t seed_lo, seed_hi;   /* dropout RNG seed */
  uint32_t step;               /* dropout stream id; incremented by gt_optimizer_step (a host may overwrite it) */
  uint32_t opt_step;           /* optimizer updates applied so far (Adam t-1); incremented by gt_optimizer_step */
  float lr;                    /* ref:train.py:136 learning_rate */
  float grad_scale;            /* 1/world_size for data-parallel averaging, else 1 */
  float beta1, beta2, eps;     /* Adam (torch defaults 0.9 / 0.999 / 1e-8) */
  float pad2[3];               /* [0],[1]: ticket words of the loss / optimizer reductions (must start as 0) */
} gt_step_state;

/* ---- dropout RNG (shared with oracle/numpy_groove.py) ------------------------------------------
 * fmix32 = murmur3 finaliser.  key(site) = fmix32((fmix32((seed_lo ^ fmix32(step)) ^ site*0x9E3779B9)
 * ^ seed_hi) + 0x7F4A7C15);  r(idx) = fmix32((idx*0x9E3779B1) ^ key);  keep iff (r>>8) >= p*2^24;
 * kept values are scaled by 1/(1-p).  idx = flat element index of the dropped tensor
 * ((M,d) / (M,F): m*cols+c; attention probabilities: ((b*H+h)*32+i)*32+j).  Sites: */
#define GT_SITE_PE_ENC 0
#define GT_SITE_PE_DEC 1
#define GT_SITE_LAYER0 16   /* site = 16 + 8*global_layer + kind; decoder layers follow the encoder's */
#define GT_SITE_ATTN 0      /* self-attention probabilities */
#define GT_SITE_DROP1 1     /* dropout1 after self-attn out-proj */
#define GT_SITE_FFN 2       /* dropout inside the FFN */
#define GT_SITE_DROPF 3     /* dropout on the FFN output (encoder dropout2 / decoder dropout3) */
#define GT_SITE_XATTN 4     /* decoder cross-attention probabilities */
#define GT_SITE_DROP2 5     /* decoder dropout2 after cross-attn out-proj */

const char* gt_last_error(void);
int gt_version(void);

/* Parameter layout in the flat buffer.  n_tensors / n_floats may be NULL.
 * Replaces: model.state_dict() ordering of the reference's nn.Module (ckpt key order). */
int gt_param_count(const gt_config* cfg, int64_t* n_tensors, int64_t* n_floats);
/* offsets[i], sizes[i] in floats; rows[i], cols[i] the 2-D shape (cols = 0 for vectors). */
int gt_param_layout(const gt_config* cfg, int64_t* offsets, int64_t* sizes, int32_t* rows, int32_t* cols);

/* Bytes of scratch the forward/backward of this config needs (saved activations + temporaries). */
size_t gt_workspace_bytes(const gt_config* cfg);
/* Call ONCE on a freshly allocated workspace, before its first use (stream-ordered; the library itself never allocates): zeroes the
 * pair-exchange region of the four-workgroups-per-sequence forward (gt_set_seq_quad), whose granules are zero between launches by
 * protocol.  A no-op for configs without such a region.  No counterpart in the reference (torch owns its activations there). */
int gt_workspace_init(const gt_config* cfg, float* ws, gt_stream_t stream);
/* Test/debug: locate a named saved activation inside the workspace (offset & count in floats).
 * names: every public region of ws_layout (groove_hip.hip) by the name it is recorded under; "<name>16" for its bf16 shadow where it has one;
 * "w16" / "w16t" (weight shadows of one encoder layer); "xchg_err".  layer = global layer index (decoder layers follow the
 * encoder's), ignored for the regions a workspace has once. */
int gt_ws_find(const gt_config* cfg, const char* name, int layer, int64_t* offset, int64_t* count);

/* Replaces GrooveTransformer(Encoder).forward(src[, tgt]) (ref:train.py:195-215 via train_loop;
 * module tree pinned by the demo checkpoint).  x (M,src_dim); tgt_in (M,27) teacher-forcing input
 * or NULL when n_dec_layers==0; pe (32,d_model) the registered positional-encoding buffer;
 * hvo_out (M,27) = [h logits | sigmoid v | 0.5 tanh o].  state==NULL or train==0 -> eval mode
 * (no dropout).  Saved activations for gt_backward are left in ws. */
int gt_forward(const gt_config* cfg, const float* params, const float* pe, const float* x,
               const float* tgt_in, float* hvo_out, float* ws, const gt_step_state* state, int train,
               gt_stream_t stream);

/* Replaces calculate_loss(pred, y, bce_fn, mse_fn, hit_loss_penalty) (ref:train.py:201-203,213;
 * bce/mse: ref:train.py:176-179; penalty: ref:train.py:55-58).  stats (8 floats, zeroed by the
 * call): [0] loss, [1] hit accuracy, [2] unused (perplexity = exp(stats[3]) on the host), [3] bce,
 * [4] mse_v, [5] mse_o.  d_hvo (M,27) or NULL: d loss / d (h,v,o). */
int gt_loss(const gt_config* cfg, const float* hvo, const float* y, float hit_loss_penalty,
            float* stats, float* d_hvo, gt_stream_t stream);

/* Replaces loss.backward() for the same module.  d_hvo (M,27) = grad w.r.t. forward's outputs.
 * grads: flat buffer, same layout as params; zeroed first unless accumulate != 0. */
int gt_backward(const gt_config* cfg, const float* params, float* grads, const float* x,
                const float* tgt_in, const float* hvo, const float* d_hvo, float* ws,
                const gt_step_state* state, int train, int accumulate, gt_stream_t stream);

/* Replaces optimizer.step() of torch.optim.SGD(lr, momentum=0) (ckpt: optimizer param_groups) /
 * torch.optim.Adam(lr) (ref:train.py:40-42).  algo 0 = sgd, 1 = adam (m, v: flat moment buffers).
 * Reads lr/grad_scale/betas from *state and increments state->step / opt_step.  zero_grads != 0 also
 * zeroes the consumed gradient buffer (what opt.zero_grad() does before the next batch).
 * PLAIN: every one of the n elements is updated, for any n (a sub-range, an unpadded buffer); no error word and no guard
 * element are looked at -- the fail-safe of the in-launch exchanges belongs to gt_train_step / gt_optimizer_step_ws, which
 * know the configuration and its workspace. */
int gt_optimizer_step(int algo, float* params, float* grads, float* m, float* v, int64_t n,
                      gt_step_state* state, int zero_grads, gt_stream_t stream);

/* gt_optimizer_step for the data-parallel step sequence (gt_train_step(skip_update = 1..3), all-reduce, update): with the
 * configuration and its workspace at hand the update on the sequence-resident path also writes the next step's fragment-ordered
 * weight copies (see GT_STEP_PACKS_CURRENT below).  The buffers are the WHOLE flat buffers of the configuration (gt_param_count
 * n_floats elements).  This entry point -- like the update inside gt_train_step -- carries the fail-safe of the in-launch exchanges:
 * with the workspace's error word set ("xchg_err"), or with a non-zero GUARD element grads[n_floats - 1] (padding behind the 27-float
 * output bias; gt_dp_guard writes it, the gradient all-reduce sums it), NOTHING is applied: parameters and moments stay, consumed
 * gradients are cleared (zero_grads), state->step advances (the batch was consumed: fresh dropout masks) but state->opt_step (Adam's t)
 * does not, and word 1 of the "xchg_err" header counts the skipped update.  The guard element itself is neither updated nor cleared. */
int gt_optimizer_step_ws(const gt_config* cfg, int algo, float* params, float* grads, float* m, float* v, float* ws,
                         gt_step_state* state, int zero_grads, gt_stream_t stream);

/* Gradient buckets for overlapping the data-parallel all-reduce with backward (no reference counterpart: the
 * reference is single-device).  Writes up to two [offset, offset+count) ranges of the flat gradient buffer in the order
 * backward completes them and returns their number: 2 when the model splits (encoder-decoder: decoder half first;
 * encoder-only with >= 2 layers: upper half of the layers first; sequence-resident path: only while the weight gradients ride in
 * the SPLIT backward phases -- gt_set_seq_ride -- where everything from encoder layer L - p + 1 on is final after phase p), else 1
 * (the whole buffer). */
int gt_grad_buckets(const gt_config* cfg, int64_t* offsets, int64_t* counts);

/* One whole train step of train_loop's batch body (ref:train.py:195-215): [shift y for the decoder]
 * forward, loss, backward, optimizer update.  tgt_scratch (M,27) is only used when n_dec_layers>0.
 * skip_update: 0 = the whole step; 1 = no optimizer update (data-parallel: all-reduce grads, then gt_optimizer_step);
 * 2 = as 1 but backward stops as soon as bucket 0 of gt_grad_buckets() is final; 3 = ONLY the rest of that backward
 * (same buffers, directly after a skip_update=2 call) -- the caller all-reduces bucket 0 while 3 runs.
 * PRECONDITION: grads is all zeros on entry (zero it once after allocation; the update this call -- or the
 * caller's gt_optimizer_step(zero_grads=1) -- leaves it zeroed again, so no per-step memset is enqueued).
 * skip_update | GT_STEP_PACKS_CURRENT: on the sequence-resident path (gt_step_launches() > 0) a whole step (skip_update 0) ends with an
 * update that also writes the NEXT step's fragment-ordered weight copies into ws; a caller that knows the previous call on this ws was
 * such a step and that nobody has written params since may set this bit, and the packing launch at the head of the step is skipped.
 * Ignored on the other paths. */
#define GT_STEP_PACKS_CURRENT 4
int gt_train_step(const gt_config* cfg, int algo, float* params, float* grads, float* m, float* v,
                  const float* pe, const float* x, const float* y, float hit_loss_penalty,
                  float* hvo_out, float* stats, float* tgt_scratch, float* ws, gt_step_state* state,
                  int skip_update, gt_stream_t stream);

/* The loss controls beyond the one hit_loss_penalty (no counterpart in ref:train.py:55-58,176-179, whose calculate_loss has that float
 * alone): separate penalties for the hit term and for the velocity / offset terms, torch.nn.BCEWithLogitsLoss(pos_weight) per voice, a
 * weight per voice and per term, focal modulation of the hit term.  lo is HOST memory, read when the call is enqueued (a captured graph
 * keeps the values).  Per element (row m, voice c), in fp32, with p = sigmoid(h), sp = log1pf(expf(-|h|)):
 *   pen_h = (yh == 1) ? 1 : penalty_h;  pen_vo = (yh == 1) ? 1 : penalty_vo
 *   bce0  = max(h,0) - h yh + sp + (pos_weight[c] - 1) yh (sp + max(-h,0))        (torch's formula; pos_weight 1 adds an exact zero)
 *   f     = 1 for focal_gamma == 0 (no powf), else powf(q, focal_gamma), q = yh sigmoid(-h) + (1 - yh) p  (= 1 - p_t, no cancellation)
 *   bce   = voice_weight[c] pen_h f bce0;  mv = voice_weight[c] pen_vo (v - yv)^2;  mo = voice_weight[c] pen_vo (o - yo)^2
 * stats (8 floats): [3] [4] [5] the means over the M rows of the voice sums of bce / mv / mo, [0] = (tw[0] [3] + tw[1] [4]) + tw[2] [5],
 * [1] hit accuracy, [2] [6] [7] = 0.  voice_stats (36 floats, or NULL): [0..9) [9..18) [18..27) each voice's share of [3] [4] [5],
 * [27..36) the hit accuracy per voice.  d_out (M,27), or NULL: the gradient of stats[0] w.r.t. the activated outputs (wrt_logits = 0), or
 * already multiplied by the head activations' derivative (wrt_logits = 1: what backward's workspace "dlogits" holds); finite for every
 * finite input; where q == 0 the focal term and its gradient are 0.  With every option neutral and penalty_vo = penalty_h, d_out is
 * bit for bit gt_loss's.
 * One workgroup per sequence; no float atomics: the per-voice sums over a sequence's 32 rows, then over the workgroups in the last arriver,
 * run in a fixed order that depends on the batch alone -- stats and voice_stats are bitwise repeatable.  scratch: gt_loss_scratch_floats
 * floats (the ticket word, then 36 partials per sequence); zero once, left zero by every call.  Needs no workspace and no step state.
 * Rejected before any launch: lo / hvo / y / stats / scratch NULL, any NaN or Inf in lo, a pos_weight <= 0, a negative voice_weight,
 * term_weight or penalty, a focal_gamma outside [0, 8].  No host sync, no allocation; capturable. */
typedef struct gt_loss_opts {
  float penalty_h;                 /* weight of the hit term where y_h != 1 (gt_loss's hit_loss_penalty) */
  float penalty_vo;                /* weight of the velocity and offset terms where y_h != 1 */
  float pos_weight[GT_VOICES];     /* BCEWithLogitsLoss(pos_weight): > 0, finite */
  float voice_weight[GT_VOICES];   /* multiplies all three terms of a voice: >= 0, finite */
  float focal_gamma;               /* 0 = plain BCE; 0 <= gamma <= 8 */
  float term_weight[3];            /* loss = tw[0] bce + tw[1] mse_v + tw[2] mse_o: >= 0, finite */
} gt_loss_opts;
int64_t gt_loss_scratch_floats(const gt_config* cfg);
int gt_loss_ex(const gt_config* cfg, const float* hvo, const float* y, const gt_loss_opts* lo, float* stats, float* voice_stats,
               float* d_out, int wrt_logits, float* scratch, gt_stream_t stream);
/* gt_train_step with that loss as a launch of its own: [shift y for the decoder,] gt_forward(train = 1) WITHOUT the loss hand-off (the
 * sequence-resident forward does not run on into backward phase 0), gt_loss_ex(wrt_logits = 1) into the workspace's "dlogits", the
 * unchanged backward, and for skip_update 0 the unchanged update (sequence-resident path: the folded update + pack).  skip_update 0..3
 * and GT_STEP_PACKS_CURRENT mean what they mean for gt_train_step (3 runs the rest of the backward alone: lo is not read).  The same
 * precondition on grads, the same fail-safe of the in-launch exchanges (it lives in the update).  One launch more than gt_train_step -- two
 * where gt_train_step's last forward launch runs on into backward phase 0; gt_step_launches itself is unchanged.  With neutral options the results agree with gt_train_step to fp32
 * rounding (the loss sums run in another order). */
int gt_train_step_loss(const gt_config* cfg, int algo, float* params, float* grads, float* m, float* v,
                       const float* pe, const float* x, const float* y, const gt_loss_opts* lo, float* voice_stats,
                       float* loss_scratch, float* hvo_out, float* stats, float* tgt_scratch, float* ws, gt_step_state* state,
                       int skip_update, gt_stream_t stream);

/* Replaces model.predict(src, use_thres=True, thres=0.5) (ref:evaluator.py:173-177): eval forward,
 * h = sigmoid(logit) > thres ? 1 : 0 (or the probability when use_thres == 0); the encoder-decoder
 * runs the 32-step greedy decode.  hvo_out (M,27) is the concatenated HVO the evaluator builds. */
int gt_predict(const gt_config* cfg, const float* params, const float* pe, const float* x,
               float* hvo_out, float thres, int use_thres, float* tgt_scratch, float* ws,
               gt_stream_t stream);
/* model.predict(src, use_pd=True): as gt_predict, but the hits are SAMPLED from the predicted probabilities: h = 1 iff p > u with
 * u = (fmix32((idx * 0x9E3779B1) ^ seed) >> 8) * 2^-24, idx = (row * 27 + voice column) of hvo_out (the hash of the dropout masks,
 * shared with oracle/numpy_groove.py).  The encoder-decoder's greedy decode feeds the sampled hits back. */
int gt_predict_pd(const gt_config* cfg, const float* params, const float* pe, const float* x, float* hvo_out, uint32_t seed,
                  float* tgt_scratch, float* ws, gt_stream_t stream);
/* The same for a CHUNK of a larger evaluation set (ref:evaluator.py:173 hands the whole set over at once; the host walks it in
 * workspace-sized chunks): first_seq = index of x's first sequence inside the set; idx above counts from the start of the SET, so the
 * samples do not depend on the chunk size.  gt_predict_pd == gt_predict_pd_at(first_seq = 0). */
int gt_predict_pd_at(const gt_config* cfg, const float* params, const float* pe, const float* x, float* hvo_out, uint32_t seed,
                     int64_t first_seq, float* tgt_scratch, float* ws, gt_stream_t stream);

/* The generation controls of this model family's front ends beyond one threshold (no counterpart in ref:evaluator.py:173, which passes
 * only use_thres / thres / use_pd): a threshold per voice, a cap on the hits a voice may place in the 32-step pattern, a temperature on
 * the hit logits.  vs is HOST memory, read when the call is enqueued (a captured graph keeps the values).
 * Decision per hit element (row m, voice c), in fp32: p = sigmoid(logit / temperature) -- a division, so temperature 1 gives exactly
 * the probability of gt_predict -- is written to prob_out[m * 9 + c]; mode 0: h = p > thres[c]; mode 1: h = (p > u) && (p > thres[c])
 * with u the uniform of gt_predict_pd_at (same hash, same index first_seq * 32 * 27 + m * 27 + c: thres = 0 is pure sampling, and the
 * samples do not depend on how a set is cut into calls; seed is unused in mode 0).  Velocity and offset pass through as in gt_predict.
 * The encoder-decoder's greedy decode takes this decision at each step, writes that step's rows of prob_out and feeds the decided hits
 * back (velocity and offset unmasked, as in gt_predict).
 * Then ONE pass (gt_voice_select: the same pass over any (n_seq * 32, 27) HVO buffer and (n_seq * 32, 9) probabilities): per (sequence,
 * voice), of the steps with a hit at most max_count[voice] stay -- the most probable ones, and of two equal probabilities the EARLIER
 * step: step t stays iff fewer than max_count other hit steps t' have p[t'] > p[t], or p[t'] == p[t] with t' < t.  Dropped hits become 0.
 * mask_vo: velocity and offset of every (step, voice) whose final hit is 0 become 0; without it those columns are never written.
 * Encoder-decoder: the cap prunes the FINISHED pattern -- the hits fed back during the decode are the uncapped ones.
 * With every cap at 32 and mask_vo 0 the pass is not launched.  No atomics: bitwise reproducible.  No host sync, no allocation; capturable.
 * Rejected before any launch: vs or prob_out NULL, a threshold outside [0,1] or NaN, a cap outside 0..32, a temperature <= 0 or not
 * finite, a mode other than 0 / 1 (gt_voice_select checks the whole struct too), first_seq < 0, an encoder-decoder call without
 * tgt_scratch.  prob_out: (M,9) device floats. */
typedef struct gt_voice_sampling {
  float   thres[GT_VOICES];      /* each in [0,1] */
  int32_t max_count[GT_VOICES];  /* 0..32 hits of this voice per sequence; 32 = no cap */
  float   temperature;           /* > 0, finite; p = sigmoid(logit / temperature) */
  int32_t mode;                  /* 0 = threshold, 1 = sampled */
  int32_t mask_vo;               /* 1: velocity and offset of a (step, voice) without a hit are written as 0 */
} gt_voice_sampling;
int gt_predict_voices(const gt_config* cfg, const float* params, const float* pe, const float* x,
                      float* hvo_out, const gt_voice_sampling* vs, uint32_t seed, int64_t first_seq,
                      float* prob_out, float* tgt_scratch, float* ws, gt_stream_t stream);
int gt_voice_select(float* hvo, const float* prob, const gt_voice_sampling* vs, int64_t n_seq,
                    gt_stream_t stream);

/* Replaces, for the device side, what the reference's evaluator computes from model.predict's output per epoch
 * (ref:evaluator.py:522-525: get_hits_accuracies / get_velocity_errors / get_micro_timing_errors over the 9 voices of
 * ROLAND_REDUCED_MAPPING): hvo_pred / hvo_gt are (n_rows,27) HVO tensors (n_rows = sequences * 32).  out30:
 * [0] hit accuracy over all voices, [1..9] per voice; [10] velocity MSE, [11..19] per voice; [20] offset MSE, [21..29] per
 * voice.  scratch: gt_voice_metrics_scratch_floats(n_rows) floats.  Fixed summation order: bitwise reproducible. */
int64_t gt_voice_metrics_scratch_floats(int64_t n_rows);
int gt_voice_metrics(const float* hvo_pred, const float* hvo_gt, int64_t n_rows, float* out30, float* scratch,
                     gt_stream_t stream);

/* Per-voice hit threshold curves (no counterpart in ref:evaluator.py:522-525, whose only hit metric is the accuracy gt_voice_metrics
 * computes -- dominated by the empty cells): for each voice and each of the two classes (the ground truth is a hit, or is not), how many
 * predicted probabilities lie above each threshold of a grid.  Precision, recall and F-beta at any grid threshold follow from the counts,
 * and so does the threshold that is best under a rule (gt_hit_thresholds): the nine numbers gt_predict_voices' thres takes.
 * prob: device; the probability of row m, voice c is prob[m * prob_stride + c].  prob_stride 9 = the prob_out of gt_predict_voices, 27 = the
 * hit columns of an HVO buffer written by gt_predict with use_thres 0; nothing else is accepted.  hvo_gt (n_rows,27): the class is
 * g = (hvo_gt[m * 27 + c] == 1.0f), the loss's yh == 1 convention.  thres is HOST memory, read when the call is enqueued (a captured graph
 * keeps the values): n_thres values, strictly ascending, each in [0,1].
 * bin(p) = the number of k with p > thres[k] -- fp32 and strict, the comparison gt_predict_voices decides hits with; bin(NaN) = 0.
 * counts: device, 9 * 2 * (n_thres + 1) unsigned 64-bit words; counts[(c * 2 + g) * (n_thres + 1) + bin] += 1 for every element.  The call
 * ADDS: zero the buffer once and walk a set in chunks.  TP_k(c) = sum of counts[c][1][b] over b > k, FP_k(c) the same with g = 0,
 * P(c) = sum of counts[c][1][b] over all b, FN_k = P - TP_k.  Integer arithmetic throughout: the result depends on neither the launch
 * geometry nor on how a set is cut into calls or on their order.
 * Two launches (csrc/gt_curve.h): workgroups with 32-bit LDS histograms write partials to scratch, a second kernel adds them onto counts
 * (one writer per word: no global atomics).  scratch: gt_hit_curve_scratch_words 32-bit words, device; NO precondition (every word read was
 * written by the same call) -- it need not be zeroed and is not left zero.  No host sync, no allocation; capturable.
 * Rejected before any launch, counts untouched: a NULL pointer, n_rows <= 0 or >= 2^31, n_thres < 1 or > GT_CURVE_MAX_THRES, a prob_stride
 * other than 9 or 27, a threshold that is NaN or outside [0,1], thresholds not strictly ascending. */
#define GT_CURVE_MAX_THRES 127
int64_t gt_hit_curve_scratch_words(int64_t n_rows, int32_t n_thres);          /* 32-bit words */
int gt_hit_curve(const float* prob, int32_t prob_stride, const float* hvo_gt, int64_t n_rows,
                 const float* thres, int32_t n_thres, uint64_t* counts, uint32_t* scratch, gt_stream_t stream);
/* The choice, a pure host function (like gt_param_layout): counts_host = a HOST copy of gt_hit_curve's counts over the same grid.  Per voice,
 * in fp64 from the integers above:
 *   criterion 0 (F-beta): with b2 = (double)beta * beta, score_k = (1 + b2) TP_k / ((1 + b2) TP_k + b2 FN_k + FP_k), 0 where TP_k == 0; each
 *     product is rounded on its own and the denominator summed left to right -- compiled with floating-point contraction off, so no fused
 *     multiply-add is formed.  The candidates are the k whose score EQUALS the maximum (equal counts give equal doubles: the plateau
 *     between two distinct probabilities is an exact tie);
 *   criterion 1 (density): the candidates are the k that minimise |TP_k + FP_k - P|, an integer: the voice places as many hits as the
 *     ground truth has.
 * The chosen index is the LOWER MEDIAN of the candidates: element (n - 1) / 2 of their ascending list.  thres_out[c] = thres[index_out[c]].
 * Fallback -- index_out[c] = -1, thres_out[c] = rule->fallback, four zero scores -- where P == 0, and under criterion 0 where the best score is 0.
 * scores_out[4 c ..] at the chosen index: precision TP / (TP + FP) (0 for a zero denominator), recall TP / P, the F-beta score (criterion 1:
 * with rule->beta where that is > 0 and finite, else 0), the density ratio (TP + FP) / P.
 * Rejected: a NULL pointer, a grid gt_hit_curve would reject, a criterion other than 0 / 1, under criterion 0 a beta <= 0 or not finite,
 * a fallback outside [0,1]. */
typedef struct gt_threshold_rule {
  int32_t criterion;   /* 0 = F-beta, 1 = density */
  float beta;          /* > 0, finite; criterion 0 only */
  float fallback;      /* in [0,1]: the threshold of a voice the rule cannot decide */
} gt_threshold_rule;
int gt_hit_thresholds(const uint64_t* counts_host, const float* thres, int32_t n_thres, const gt_threshold_rule* rule,
                      float* thres_out /*9*/, int32_t* index_out /*9*/, float* scores_out /*9 x 4*/);

/* Per-group and removed-cell evaluation counts: the device side of the reference's per-subset evaluation (ref:evaluator.py:171-196 splits a
 * set by genre tag and reports hit, velocity and micro-timing numbers per subset), of hit metrics confined to the cells an infilling pair
 * removed, of the velocity / offset error on the hits that came back, and of per-sequence counts a host can pick examples by -- one counting
 * pass over the two HVO buffers.  hvo_pred / hvo_gt: (n_seq * 32, 27), device.  group (n_seq int32, device, or NULL: every sequence in
 * group 0): a sequence with group[s] < 0 or >= n_groups is SKIPPED -- none of its cells reach acc, and the last word of acc counts it.
 * cells (n_seq x 9 uint32, device, or NULL: every cell): the convention of gt_gather_infill_events and gt_infill_merge_cells -- cell (s, t, c) is
 * counted iff bit t of cells[s * 9 + c] is set.
 * Per counted cell, with m = s * 32 + t, g = group[s], in fp32: ph = (hvo_pred[m * 27 + c] == 1.0f), gh = (hvo_gt[m * 27 + c] == 1.0f) (the
 * loss's and the curve's yh == 1 convention; a NaN is no hit); dv = pred - gt of column 9 + c, ev = dv * dv; eo the same from column 18 + c.
 * acc[(g * 9 + c) * 8 + k] += : k = 0: 1 (counted cells); 1: TP = ph && gh; 2: FP = ph && !gh; 3: FN = !ph && gh; 4: fix of ev; 5: fix of eo;
 * 6 / 7: the same two for TP cells only.  fix of e = (uint64_t)((double)e * 4294967296.0 + 0.5) when e <= 16.0f: 32 fractional bits, exact
 * (an fp32 value times a power of two is exact in fp64).  Any other e (NaN, +-inf, above 16) adds nothing to k = 4..7 and counts as a
 * REJECTED value, once per velocity and once per offset value.  Capacity: with e <= 16 a word holds 2^28 cells in the worst case, 2^32
 * cells of errors <= 1 (velocities in [0,1], offsets in [-0.5,0.5]).
 * Behind the n_groups * 72 words: acc[n_groups * 72 + 2 g] += 1 per sequence of group g, acc[n_groups * 72 + 2 g + 1] += its rejected
 * values; then one word, += 1 per skipped sequence.  GT_GM_ACC_WORDS words in all.  The call ADDS: zero acc once and walk a set in chunks.
 * Integer arithmetic throughout: the result depends on neither the launch geometry nor on how a set is cut into calls or on their order.
 * seq_out (n_seq x 4 uint32, device, or NULL): seq_out[s * 4 + {0,1,2,3}] = the counted cells, TP, FP and FN of sequence s summed over the
 * nine voices -- STORED, not added, for every s < n_seq: a skipped sequence's counts are written all the same, only acc leaves it out.
 * Two launches (csrc/gt_group.h): workgroups with 64-bit accumulators in LDS, one owner thread per word, write partials to scratch; a second
 * kernel adds them onto acc (one writer per word).  No global atomics, no floating-point atomics.  scratch: gt_group_metrics_scratch_words
 * 64-bit words, device; NO precondition (every word read was written by the same call) -- it need not be zeroed and is not left zero.
 * No host sync, no allocation; capturable.
 * Rejected before any launch, acc untouched: hvo_pred, hvo_gt, acc or scratch NULL, n_seq <= 0 or >= 2^26, n_groups < 1 or
 * > GT_GM_MAX_GROUPS. */
#define GT_GM_MAX_GROUPS 64
#define GT_GM_WORDS 8                 /* 64-bit words per (group, voice) */
/* acc: n_groups*9*8 words, then n_groups*2 words (per group: sequences, rejected values), then 1 word (skipped sequences) */
#define GT_GM_ACC_WORDS(n_groups) ((n_groups) * (GT_VOICES * GT_GM_WORDS + 2) + 1)
int64_t gt_group_metrics_scratch_words(int64_t n_seq, int32_t n_groups);      /* 64-bit words */
int gt_group_metrics(const float* hvo_pred, const float* hvo_gt,
                     const int32_t* group  /* n_seq, device; NULL: every sequence in group 0 */,
                     const uint32_t* cells /* n_seq x 9, device; NULL: every cell */,
                     int64_t n_seq, int32_t n_groups, uint64_t* acc,
                     uint32_t* seq_out /* n_seq x 4, device, or NULL */,
                     uint64_t* scratch, gt_stream_t stream);

/* Groove descriptors and rhythmic distances per sequence: the integers behind the reference's table of rhythmic descriptors for
 * __Ground_Truth beside __Prediction (get_stats_from_evaluator, written as stats_<run>_Epoch_<n>.csv on the "all" epochs, ref:evaluator.py:516-601)
 * and behind per-sequence distances of a prediction from its target (the reference keeps a commented get_rhythmic_distances call).  The
 * reference's GrooveEvaluator is not vendored: the definitions below are this library's own.
 * hvo_a, hvo_b (or NULL): (n_seq * 32, 27), device, 16-byte aligned.  feat_a, feat_b (or NULL): n_seq x GT_GF_WORDS 64-bit words; pair (or
 * NULL): n_seq x GT_GF_PAIR_WORDS.  Every output word of every s < n_seq is STORED, not added (reserved words as 0): no zeroed buffer, no
 * scratch, nothing left behind.  hvo_b with feat_b NULL, with pair NULL or with both NULL is legal (a host computes the ground truth's record
 * once and afterwards asks for feat_a and pair only).
 * Conventions: step t = 0..31, voice c = 0..8; a cell is a hit iff hvo[(s * 32 + t) * 27 + c] == 1.0f (the loss's convention; a NaN, 0.5 or
 * 2.0 is no hit).  At a hit v = column 9 + c, o = column 18 + c; v is valid iff 0.0f <= v && v <= 16.0f, o iff fabsf of o <= 16.0f (a NaN
 * fails both).  An invalid value at a hit adds nothing to the value words and the profile and counts as rejected; the hit itself counts.
 * fix of e = (uint64_t)((double)e * 4294967296.0 + 0.5) (gt_group_metrics' fixed point: 32 fractional bits, exact); q of v =
 * (uint32_t)((double)v * 65536.0 + 0.5); the profile P[t] = the sum over c of q of v over the hits of step t with a valid v (< 2^24).
 * Squares (v * v, ...) are one fp32 multiply before fix.
 * feat[s * 32 + k]: 0: hits; 1: voices with at least one hit; 2: steps with at least one hit; 3: hits at t % 4 == 0; 4: hits at t % 4 == 2;
 * 5: hits at odd t; 6: cells (t < 16, c) hit at both t and t + 16; 7: rejected velocities; 8: rejected offsets; 9: sum of fix of v; 10: of
 * fix of v * v; 11: of fix of |o|; 12: of o as signed fixed point (+fix of o for o >= 0, -fix of -o otherwise: a two's-complement 64-bit
 * integer); 13: of fix of o * o; 14: 0; 15 + l, l = 0..16: the circular autocorrelation of the profile, A[l] = sum over t of
 * P[t] * P[(t + l) mod 32].  Worst case (every cell a hit at v = 16): A[l] about 2^51.3, word 10 about 2^48.2.
 * pair[s * 8 + k], p = buffer a, g = buffer b: 0: cells whose hits differ (Hamming); 1: cells hit in both; 2: near misses -- a cell hit in p
 * and not in g while g has a hit of the same voice at t - 1 or t + 1, or the same with p and g exchanged (steps outside 0..31 do not exist:
 * no wrap-around); 3: sum over ALL cells of fix of dv * dv, dv = v'_p - v'_g in fp32, v' = v at a hit with a valid velocity and 0 elsewhere;
 * 4: sum of fix of do * do, do = o_p - o_g, over the cells hit in both with both offsets valid; 5: the number of those cells; 6: sum over t
 * of P_p[t] * P_g[t]; 7: 0.
 * Integers throughout: the result depends on neither the launch geometry, nor a sequence's position in the set, nor its neighbours.
 * One launch (csrc/gt_groove.h); no global atomics, no floating-point atomics, one writer per word; no host sync, no allocation; capturable.
 * Rejected before any launch, outputs untouched: hvo_a or feat_a NULL, n_seq <= 0 or >= 2^26, feat_b or pair given without hvo_b, a
 * misaligned pointer. */
#define GT_GF_WORDS 32                /* 64-bit words per sequence and buffer */
#define GT_GF_PAIR_WORDS 8
int gt_groove_features(const float* hvo_a, const float* hvo_b /* or NULL */, int64_t n_seq,
                       uint64_t* feat_a /* n_seq x 32 */, uint64_t* feat_b /* n_seq x 32, or NULL */,
                       uint64_t* pair /* n_seq x 8, or NULL */, gt_stream_t stream);

/* Replaces GrooveMidiDatasetInfilling.__getitem__ + the DataLoader's collate for a dataset resident in HBM
 * (ref:dataset.py:263-264,355-356; ref:train.py:156-158): x[b] = xs[idx[b]], y[b] = ys[idx[b]] for b < batch, both step
 * inputs in ONE launch.  xs (n_seq,32,src_dim), ys (n_seq,32,27) fp32; idx int64 on the device (out-of-range entries are
 * clamped into the dataset). */
int gt_gather_batch(const float* xs, const float* ys, const int64_t* idx, int64_t n_seq, int32_t batch, int32_t src_dim,
                    float* x, float* y, gt_stream_t stream);

/* Replaces GrooveMidiDatasetInfillingSymbolic's pairing (ref:dataset.py:380-459) and the voice combinations it freezes per groove at
 * preprocessing time (ref:utils.py:69-115) for the symbolic experiments (src_dim 27): the gather itself draws which voices to remove,
 * afresh at every visit of a groove.  hvo_set (n_seq,32,27) FULL grooves; idx: batch int64 indices on the device, clamped like
 * gt_gather_batch's.  x[b] = the groove with the hit / velocity / offset columns c, 9 + c, 18 + c zeroed for every removed voice c (the model's
 * input), y[b] = the groove with those columns kept and all others zeroed (the target: the removed part; ref:evaluator.py:364-372 adds the
 * two back together); kept values are bit copies.  removed (batch int32, or NULL): the removal bitmasks.  io is HOST memory, read when the
 * call is enqueued (a captured graph keeps the values); state is a DEVICE pointer, required: seed_lo, seed_hi and step are read on the
 * device, so a graph replay draws afresh once the update has advanced step.
 * The draw for source index src (after clamping), in unsigned 32-bit wrap-around integers throughout -- no floating point:
 *   voice c is active iff any of the 32 hit values hvo_set[src][t][c] is != 0; n_tot = active voices, n_act = active voices inside
 *   voice_mask (the candidates, in ascending voice order); hi = min(max_remove, n_act, n_tot - 1) (the reference drops pairs whose input or
 *   output would be empty); W_k = count_weight[k - min_remove] * C(n_act, k) for k in min_remove..hi, T = their sum.  T == 0: the sequence
 *   is INELIGIBLE -- nothing is removed (x = the groove, y = zeros, removed = 0); hosts keep such sequences out of the index stream.
 *   key = the dropout streams' key(site) above with site = GT_SITE_INFILL; r_j = fmix32(((uint32)(src * 16 + j) * 0x9E3779B1) ^ key).
 *   Size: pick = ((uint64)r_0 * T) >> 32, k = the smallest size whose running sum of W exceeds pick.  Subset, by selection sampling: need = k,
 *   left = n_act; candidate c is taken iff (((uint64)r_{1+c} * left) >> 32) < need; then left--, and need-- if taken.  Exactly k are taken.
 * The draw depends on src, not on the batch position: two batch elements with the same src in one call get the SAME draw.
 * Rejected before any launch: a NULL pointer other than removed, batch or n_seq <= 0, a zero voice_mask or one with bits >= 9,
 * min_remove < 1, max_remove < min_remove, max_remove > 9, a weight outside 0..1024, all weights of the sizes min_remove..max_remove zero.
 * One launch, no atomics; no host sync, no allocation; capturable. */
#define GT_SITE_INFILL 2      /* free: sites 0, 1 and >= 16 are taken */
typedef struct gt_infill_opts {
  int32_t voice_mask;               /* bit c set: voice c may be removed (voices_params["voice_idx"]); non-zero, no bits >= 9 */
  int32_t min_remove, max_remove;   /* 1 <= min_remove <= max_remove <= 9 */
  int32_t count_weight[GT_VOICES];  /* count_weight[k - min_remove]: weight of EACH combination of size k (the reference's "prob");
                                       0..1024; entries past max_remove - min_remove are ignored */
} gt_infill_opts;
int gt_gather_infill(const float* hvo_set, const int64_t* idx, int64_t n_seq, int32_t batch,
                     const gt_infill_opts* io, const gt_step_state* state,
                     float* x, float* y, int32_t* removed, gt_stream_t stream);
/* Replaces add_removed_part_to_hvo (ref:evaluator.py:364-372): a prediction put back into the groove it was made from, so that what leaves
 * the device is a complete pattern.  hvo_pred, hvo_in, hvo_out: (n_seq * 32, 27); hvo_out may alias hvo_pred.  removed (n_seq int32, or
 * NULL): where voice c is outside removed[row / 32] the prediction's three values of that cell count as 0 -- the model may only fill what
 * was removed.  Per cell (row, voice c) with the input's hit in_h:
 *   mode 0 (the reference's arithmetic): h = in_h != 0 ? in_h : pred_h + in_h;  v = pred_v + in_v;  o = pred_o + in_o
 *   mode 1: where in_h != 0 the input's (h, v, o) win whole; elsewhere (h, v, o) = pred.
 * mode 1 with pred = y, in = x of gt_gather_infill and its removed gives back the source groove exactly (an HVO groove: velocity and
 * offset are 0 wherever the hit is 0).
 * Rejected before any launch: hvo_pred, hvo_in or hvo_out NULL, n_seq <= 0 or >= 2^26 (the grid's reach; hosts walk larger sets in
 * chunks), a mode other than 0 or 1.  One elementwise launch. */
int gt_infill_merge(const float* hvo_pred, const float* hvo_in, const int32_t* removed, int64_t n_seq,
                    int32_t mode, float* hvo_out, gt_stream_t stream);

/* Event-level infilling pairs: replaces GrooveMidiDatasetInfillingRandom's pairing (ref:dataset.py:464-555,
 * hvo_seq.remove_random_events(thres_range=(0.4, 0.6))) in its symbolic form (src_dim 27; the reference's MSO input of these experiments is
 * out of scope).  Where gt_gather_infill removes whole voices, this gather takes a random share of the individual HITS out of a groove,
 * across voices.  hvo_set (n_seq,32,27) FULL grooves; idx: batch int64 indices on the device, clamped like gt_gather_batch's.  Conventions
 * as gt_gather_infill: eo is HOST memory, read when the call is enqueued (a captured graph keeps the values); state is a DEVICE pointer,
 * required: seed_lo, seed_hi and step are read on the device, so a graph replay draws afresh once the update has advanced step; kept
 * values are bit copies.
 * The draw for source index src (after clamping), in unsigned 32-bit wrap-around integers throughout -- no floating point:
 *   cell j = t * 9 + c (step t, voice c, 0 <= j < 288) is an EVENT iff hvo_set[src][t][c] != 0 and a CANDIDATE iff it is an event and bit c
 *   of voice_mask is set; n_ev = events, n_cand = candidates; cap = min(n_cand, n_ev - 1): neither side of the pair may be empty (the
 *   reference drops such pairs, ref:dataset.py:520-524).  cap < 1: the sequence is INELIGIBLE -- x = the groove, y = zeros, its nine cells
 *   words = 0; hosts keep such sequences out of the index stream.
 *   key = the dropout streams' key(site) above with site = GT_SITE_INFILL_EVENTS; base = (uint32)(src * 512);
 *   r_i = fmix32(((base + i) * 0x9E3779B1) ^ key).
 *   Share: q = ratio_lo + (((uint64)r_0 * (uint32)(ratio_hi - ratio_lo + 1)) >> 32).
 *   Count: k0 = (n_cand * q + 32768) >> 16, k = min(max(k0, 1), cap).
 *   Subset: candidate j is removed iff fewer than k candidates j' have r_{1+j'} < r_{1+j} -- the k candidates with the smallest hash.  No
 *   tie rule is needed: fmix32, the odd multiplier and the XOR are each bijections on 32 bits and base + 1 + j is distinct for j < 288, so
 *   the 288 values of one sequence are pairwise different.  Exactly k cells are removed; the rule depends on no visiting order.
 * Outputs: for a removed cell (t, c), x gets 0 in its h, v and o entries (columns c, 9 + c, 18 + c of row t) and y gets the groove's three
 * values; for every other cell x gets the groove's values and y gets 0.  cells (batch x 9 uint32, or NULL): cells[b * 9 + c] has bit t set
 * iff cell (t, c) was removed.
 * The draw depends on src, not on the batch position: two batch elements with the same src in one call get the SAME draw.
 * Rejected before any launch: a NULL pointer other than cells, batch or n_seq <= 0, a zero voice_mask or one with bits >= 9, a ratio
 * outside 0..65536, ratio_lo > ratio_hi.  One launch, no atomics on global memory, bitwise repeatable; no host sync, no allocation;
 * capturable. */
#define GT_SITE_INFILL_EVENTS 3          /* sites 0, 1, 2 and >= 16 are taken */
typedef struct gt_infill_event_opts {
  int32_t voice_mask;           /* bit c set: hits of voice c may be removed; non-zero, no bits >= 9 */
  int32_t ratio_lo, ratio_hi;   /* share of the candidate hits to remove, in 1/65536ths: 0 <= ratio_lo <= ratio_hi <= 65536 */
} gt_infill_event_opts;
int gt_gather_infill_events(const float* hvo_set, const int64_t* idx, int64_t n_seq, int32_t batch,
                            const gt_infill_event_opts* eo, const gt_step_state* state,
                            float* x, float* y, uint32_t* cells /* batch x 9, or NULL */, gt_stream_t stream);
/* gt_infill_merge with the mask per cell: where bit (row % 32) of cells[(row / 32) * 9 + c] is clear, the prediction's three values of cell
 * (row, c) count as 0 -- the model may only fill the cells that were removed.  cells (n_seq x 9 uint32, or NULL): NULL behaves exactly as
 * gt_infill_merge(removed = NULL).  The two modes, the aliasing rule (hvo_out may be hvo_pred), the n_seq range and the rejections are
 * gt_infill_merge's.  With pred = y, in = x and the cells of one gt_gather_infill_events call, both modes give back the source groove
 * exactly (an HVO groove: velocity and offset are +0 wherever the hit is 0).  One elementwise launch. */
int gt_infill_merge_cells(const float* hvo_pred, const float* hvo_in, const uint32_t* cells /* n_seq x 9, or NULL */,
                          int64_t n_seq, int32_t mode, float* hvo_out, gt_stream_t stream);

/* Measurement aid (no reference counterpart): with profiling on, every kernel launch is bracketed by
 * HIP events on its own stream.  gt_profile_report synchronises and writes one text row per kernel
 * class: "label launches total_ms total_flops total_bytes".  Not graph-capturable while on. */
int gt_profile_enable(int on);
/* The pair exchange polls with a bound: a partner workgroup that never arrives (the two were not resident at the same time: another
 * stream's kernel, a CU mask, another process holds CUs) makes the waiting workgroup give up, raise the error word at the head of the
 * "seq_xchg" workspace region (gt_ws_find) and go on with garbage partials.  Fail-safe (round 5): with the word set -- it stays set until
 * the host zeroes the region with gt_workspace_init -- the fused update (gt_train_step, gt_optimizer_step_ws) leaves parameters and
 * optimizer moments untouched and only clears the consumed gradients; the same when gradient element n_floats - 1 (padding behind the
 * 27-float output bias; a data-parallel host writes its error flag there before the all-reduce) is non-zero, so every rank skips
 * together.  (The bound: 2^22 polls = seconds.)
 * "xchg_err" (gt_ws_find) = two 32-bit words at the head of whichever exchange region a shape has: [0] the error word, [1] the number of
 * updates skipped because of it (or of a data-parallel guard) since the last gt_workspace_init.
 * Data-parallel hosts: grads[n_floats - 1] = 1 if this workspace's exchange error word is set, else 0 -- enqueue between the backward
 * (gt_train_step(skip_update = 1 / 2)) and the gradient all-reduce; a no-op for shapes without an exchange region. */
int gt_dp_guard(const gt_config* cfg, float* grads, const float* ws, gt_stream_t stream);
/* torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) over the flat gradient buffer of this configuration (no counterpart in the
 * reference's step, which does not clip): total = grad_scale * ||grads[0 .. n_floats - 1)||_2 -- the guard element n_floats - 1 never
 * counts, the alignment gaps between tensors hold zeros -- coef = min(1, max_norm / (total + 1e-6)) in fp32, grads *= coef over the same
 * range.  Data-parallel: call it on the all-reduced sum; grad_scale (1/world) makes it the norm of the averaged gradient, as with DDP.
 * Fixed summation order (fp64 across workgroups): bitwise reproducible, identical on every rank.  A NaN norm gives a NaN coefficient.
 * out (device, 2 floats): [0] total norm before clipping, [1] the coefficient applied.  scratch: zero once, left zero.
 * max_norm > 0 (+inf = measure only, never scales).  No host sync; capturable. */
int64_t gt_clip_grad_norm_scratch_floats(const gt_config* cfg);
int gt_clip_grad_norm(const gt_config* cfg, float* grads, const gt_step_state* state, float max_norm,
                      float* out, float* scratch, gt_stream_t stream);
/* The optimizer knobs beyond the defaults -- torch.optim.SGD(momentum, nesterov, weight_decay; dampening 0), torch.optim.Adam(weight_decay)
 * and torch.optim.AdamW(weight_decay) -- as ONE launch enqueued just BEFORE the update (gt_optimizer_step / gt_optimizer_step_ws; with
 * gt_train_step: skip_update = 1, [gt_clip_grad_norm,] this call, the update).  It rewrites the gradient buffer (AdamW: the parameter buffer)
 * over [0, n_floats - 1) so that the unchanged update applies the optimizer torch would; the guard element n_floats - 1 is never read as
 * data and never written.  hp is HOST memory, read when the call is enqueued (a captured graph keeps the values); lr and grad_scale are
 * read on the device from *state.  With gs = grad_scale, per element in fp32:
 *   algo 0:                g = grads * gs; [g += weight_decay * params;] [b = momentum * mbuf + g, mbuf = b, g = nesterov ? g + momentum * b : b;]
 *                          grads = g / gs  (exact for gs a power of two).  A zeroed mbuf reproduces torch's first step (buf = grad).
 *   algo 1, decoupled 0:   grads = (grads * gs + weight_decay * params) / gs          (Adam's L2 weight_decay)
 *   algo 1, decoupled 1:   params *= 1 - lr * weight_decay, gradients untouched       (AdamW; the Adam update reads the decayed parameter)
 * Rejected before any launch: momentum with algo 1, decoupled with algo 0, nesterov without momentum, a negative weight_decay or momentum,
 * momentum with mbuf == NULL.  weight_decay == 0 and momentum == 0: returns 0 and launches nothing.
 * The buffers are the WHOLE flat buffers of the configuration (mbuf: n_floats floats, zeroed once; NULL without momentum).  Their alignment
 * gaps stay zero.  ws != NULL: the fail-safe predicate of gt_optimizer_step_ws -- with the "xchg_err" word set or a non-zero guard element
 * the pass writes NOTHING (no momentum advances, no parameter decays; the update that follows skips too).  ws == NULL: plain, like
 * gt_optimizer_step.  Pass ws to both calls or to neither.  Never touches state->step / opt_step.  No atomics: bitwise reproducible,
 * identical on every data-parallel rank.  No host sync; capturable. */
typedef struct gt_opt_hparams {
  float weight_decay;     /* >= 0 */
  float momentum;         /* >= 0; algo 0 only */
  int32_t nesterov;       /* needs momentum > 0 */
  int32_t decoupled;      /* algo 1 only: 1 = AdamW, 0 = L2 (added to the gradient) */
} gt_opt_hparams;
int gt_optimizer_prepare(const gt_config* cfg, int algo, float* params, float* grads, float* mbuf, const float* ws,
                         const gt_step_state* state, const gt_opt_hparams* hp, gt_stream_t stream);
/* The process-wide schedule switches (gt_set_*) and the test / measurement aids (gt_debug_*) are declared in groove_hip_debug.h: no host
 * that trains or predicts needs them.  What such a host may have to ASK stays here. */
/* Advances whenever the level in force of a switch the workspace layout depends on changes (today: the bf16 operand shadows).  A host that keeps
 * workspaces across calls compares it with the value it saw when it sized them and re-makes them on a mismatch (StepEngine.slot does). */
int gt_layout_epoch(void);
/* The level of bf16 operand shadows in force for a configuration: 0 none, 1 beside the fp32 tensors, 2 (the default where precision >= 1 applies
 * them) the GEMM-only tensors stored in bf16 ALONE -- which decides gt_workspace_bytes and which gt_ws_find names are live. */
int gt_operand_shadow_level(const gt_config* cfg);
/* The precision a configuration really runs at: 2 only where gt_config.precision = 2 applies (see there), else 1 / 0. */
int gt_precision_in_force(const gt_config* cfg);
/* Kernel launches of one gt_train_step for this configuration when it runs on the sequence-resident path (7 whole-sequence; SPLIT: 2 L + 4 with rider weight gradients, 2 L + 6
 * without; one less with GT_STEP_PACKS_CURRENT), 0 when
 * it runs one kernel per operation (dozens to hundreds).  A host that replays the step as a captured hipGraph can use it to
 * decide: measured on MI355X / ROCm 7.2 a 12-launch step is 2 % FASTER enqueued directly (0.241 vs 0.246 ms) -- the graph costs
 * ~0.4 us per node, and at this count the host stays ahead of the GPU by itself. */
int gt_step_launches(const gt_config* cfg);
int gt_profile_report(char* buf, size_t buf_len, int max_rows);

#ifdef __cplusplus
}
#endif
#endif /* GROOVE_HIP_H */
