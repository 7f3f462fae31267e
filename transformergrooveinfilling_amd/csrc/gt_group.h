// Per-group evaluation counts (include/groove_hip.h: gt_group_metrics): hit counts, squared velocity / offset errors and per-sequence
// counts of a prediction against its ground truth, split by a group tag per sequence and confined to a cell mask.
//
// COUNTING.  Cell (s, t, c) -- sequence s, step t, voice c -- adds eight 64-bit integers to the words of (group[s], c): the cell itself, TP,
// FP, FN, and the squared velocity / offset error as 32.32 fixed point (over every counted cell, and over the TP cells alone).  Integers
// throughout: no rounding, so the result depends on neither the launch geometry nor on how a set is cut into calls.
//
// Kernel 1 (group_metrics_partial_kernel<MAXG>): a bounded, grid-stride number of 256-thread workgroups, ONE sequence per workgroup and
// iteration.  The 2 x 864 floats of a sequence (16-byte aligned: 3456 bytes) come in as 2 x 216 float4 loads; the loads of the NEXT
// sequence (its group id and its nine cell words too) are issued before the current one is counted, so a workgroup always has a sequence
// in flight.  From the LDS copy, thread j (and j + 256 for the last 32) evaluates cell j = t * 9 + c: a packed count word
// (cell | TP << 8 | FP << 16 | FN << 24) and the two squared errors in fixed point (the conversion runs on all 256 threads, not 32 times on
// each owner below: measured both ways, DESIGN.md "Per-group counts").  72 OWNER threads (voice c, word k) then sum their 32 steps
// and add the sum onto the workgroup's 64-bit accumulator in LDS -- a workgroup counts one sequence at a time, so each accumulator word has
// exactly one writer and plain 64-bit read-modify-writes do (the emulator build has no 64-bit atomic).  The only atomic is a 32-bit LDS add
// for the rejected values of a sequence (at most 576; moved into the 64-bit word and zeroed per sequence), which real data never takes.
// The accumulators mirror acc's layout, sized by the template (4 / 16 / 64 groups: 2.4 / 9.5 / 37.9 KB beside 12.8 KB of staging), so a
// small group count keeps 7 or more workgroups on a CU.  At the end the workgroup writes ALL words of its slot of scratch (plain stores).
// Kernel 2 (group_metrics_sum_kernel): 32 words x 8 slices of workgroups per 256-thread block; the eight slice sums meet in LDS and ONE
// thread per word adds onto acc -- one writer per word, no global atomics.
// scratch has NO precondition and is left with the partials of the call: every word kernel 2 reads was written by kernel 1 of the same call.
// GEOMETRY.  Workgroups = min(cap, n_seq / 2, the number whose slots cost half the bytes the call reads), at least 1: with 64 groups a slot
// is 37.9 KB -- five sequences' worth of input -- and a short set must not spend its time on partials.
#pragma once
#include "gt_common.h"

#define GT_GM_THREADS 256
#define GT_GM_CELLS (32 * GT_VOICES)              // 288 cells of a sequence
#define GT_GM_Q (32 * GT_TGT / 4)                 // float4 per sequence and buffer (216)
#define GT_GM_SUM_WORDS 32
#define GT_GM_SUM_SLICES (GT_GM_THREADS / GT_GM_SUM_WORDS)

static inline int gt_gm_variant(int n_groups) { return n_groups <= 4 ? 4 : n_groups <= 16 ? 16 : GT_GM_MAX_GROUPS; }
static inline int gt_gm_wgs(int64_t n_seq, int n_groups) {
  const int64_t cap = gt_gm_variant(n_groups) <= 16 ? 2048 : 768;            // about 8 resp. 3 workgroups per CU: what their LDS admits
  const int64_t by_traffic = n_seq * (2 * GT_GM_CELLS * 3 * 4) / (2 * 8 * (int64_t)GT_GM_ACC_WORDS(n_groups));
  int64_t w = (n_seq + 1) / 2;
  if (w > by_traffic) w = by_traffic;
  if (w > cap) w = cap;
  return (int)(w < 1 ? 1 : w);
}

// fix(e): 32 fractional bits; exact, an fp32 value times a power of two is exact in fp64
__device__ static inline uint64_t gt_gm_fix(const float e) { return (uint64_t)((double)e * 4294967296.0 + 0.5); }

template <int MAXG>
__global__ __launch_bounds__(GT_GM_THREADS) void group_metrics_partial_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                             const int32_t* __restrict__ group,
                                                                             const uint32_t* __restrict__ cells, const int64_t n_seq,
                                                                             const int n_groups, uint64_t* __restrict__ part,
                                                                             uint32_t* __restrict__ seq_out) {
  __shared__ uint64_t acc[GT_GM_ACC_WORDS(MAXG)];
  __shared__ float4 sp[GT_GM_Q], sg[GT_GM_Q];
  __shared__ uint64_t sfx[2][GT_GM_CELLS];
  __shared__ unsigned scnt[GT_GM_CELLS];
  __shared__ unsigned scw[GT_VOICES], svs[4][GT_VOICES], srej;
  const int t = threadIdx.x;
  const int words = GT_GM_ACC_WORDS(n_groups);
  for (int i = t; i < words; i += GT_GM_THREADS) acc[i] = 0ull;
  if (t == 0) srej = 0u;
  float4 rp = make_float4(0.f, 0.f, 0.f, 0.f), rg = rp;
  unsigned rcw = 0xFFFFFFFFu;
  int rgid = 0;
  int64_t s = blockIdx.x;                                   // (the grid never has more workgroups than sequences)
  if (t < GT_GM_Q) {
    rp = reinterpret_cast<const float4*>(pred)[s * GT_GM_Q + t];
    rg = reinterpret_cast<const float4*>(gt)[s * GT_GM_Q + t];
  }
  if (cells && t < GT_VOICES) rcw = cells[s * GT_VOICES + t];
  if (group) rgid = group[s];
  for (; s < n_seq; s += gridDim.x) {
    if (t < GT_GM_Q) { sp[t] = rp; sg[t] = rg; }
    if (t < GT_VOICES) scw[t] = rcw;
    const int g = rgid;
    const bool valid = g >= 0 && g < n_groups;
    const int64_t nx = s + gridDim.x;
    if (nx < n_seq) {                                       // the next sequence is under way while this one is counted
      if (t < GT_GM_Q) {
        rp = reinterpret_cast<const float4*>(pred)[nx * GT_GM_Q + t];
        rg = reinterpret_cast<const float4*>(gt)[nx * GT_GM_Q + t];
      }
      if (cells && t < GT_VOICES) rcw = cells[nx * GT_VOICES + t];
      if (group) rgid = group[nx];
    }
    __syncthreads();
    const float* fp = reinterpret_cast<const float*>(sp);
    const float* fg = reinterpret_cast<const float*>(sg);
    for (int j = t; j < GT_GM_CELLS; j += GT_GM_THREADS) {
      const int tt = j / GT_VOICES, c = j % GT_VOICES, o = tt * GT_TGT + c;
      unsigned w = 0u;
      uint64_t xv = 0ull, xo = 0ull;
      if ((scw[c] >> tt) & 1u) {
        const bool ph = fp[o] == 1.0f, gh = fg[o] == 1.0f;
        const float dv = fp[o + GT_VOICES] - fg[o + GT_VOICES], dof = fp[o + 2 * GT_VOICES] - fg[o + 2 * GT_VOICES];
        const float ev = dv * dv, eo = dof * dof;
        w = 1u | ((ph && gh) ? 1u << 8 : 0u) | ((ph && !gh) ? 1u << 16 : 0u) | ((!ph && gh) ? 1u << 24 : 0u);
        const bool okv = ev <= 16.0f, oko = eo <= 16.0f;                             // (NaN <= x is false)
        if (okv) xv = gt_gm_fix(ev);
        if (oko) xo = gt_gm_fix(eo);
        if (!okv || !oko) atomicAdd(&srej, (okv ? 0u : 1u) + (oko ? 0u : 1u));
      }
      scnt[j] = w;
      sfx[0][j] = xv;
      sfx[1][j] = xo;
    }
    __syncthreads();
    if (t < GT_VOICES * GT_GM_WORDS) {                      // the owner of (voice c, word k): the only writer of its accumulator word
      const int c = t / GT_GM_WORDS, k = t % GT_GM_WORDS;
      uint64_t a = 0ull;
      if (k < 4) {
#pragma unroll 8
        for (int tt = 0; tt < 32; ++tt) a += (scnt[tt * GT_VOICES + c] >> (8 * k)) & 0xFFu;
        svs[k][c] = (unsigned)a;
      } else {
        const uint64_t* e = sfx[k & 1];
#pragma unroll 8
        for (int tt = 0; tt < 32; ++tt) {
          const int j = tt * GT_VOICES + c;
          if (k < 6 || ((scnt[j] >> 8) & 1u)) a += e[j];
        }
      }
      if (valid) acc[(g * GT_VOICES + c) * GT_GM_WORDS + k] += a;
    } else if (t == GT_VOICES * GT_GM_WORDS) {
      const unsigned r = srej;
      srej = 0u;
      if (valid) acc[n_groups * GT_VOICES * GT_GM_WORDS + 2 * g + 1] += r;
    } else if (t == GT_VOICES * GT_GM_WORDS + 1) {
      if (valid) acc[n_groups * GT_VOICES * GT_GM_WORDS + 2 * g] += 1ull;
      else acc[words - 1] += 1ull;
    }
    __syncthreads();
    if (seq_out && t < 4) {
      unsigned a = 0u;
#pragma unroll
      for (int c = 0; c < GT_VOICES; ++c) a += svs[t][c];
      seq_out[s * 4 + t] = a;
    }
  }
  __syncthreads();
  uint64_t* out = part + (size_t)blockIdx.x * words;
  for (int i = t; i < words; i += GT_GM_THREADS) out[i] = acc[i];
}

__global__ __launch_bounds__(GT_GM_THREADS) void group_metrics_sum_kernel(const uint64_t* __restrict__ part, const int nwg, const int words,
                                                                         uint64_t* __restrict__ accout) {
  __shared__ uint64_t s[GT_GM_SUM_SLICES][GT_GM_SUM_WORDS];
  const int i = blockIdx.x * GT_GM_SUM_WORDS + (threadIdx.x % GT_GM_SUM_WORDS), sl = threadIdx.x / GT_GM_SUM_WORDS;
  uint64_t a = 0ull;
  if (i < words)
    for (int w = sl; w < nwg; w += GT_GM_SUM_SLICES) a += part[(size_t)w * words + i];
  s[sl][threadIdx.x % GT_GM_SUM_WORDS] = a;
  __syncthreads();
  if (sl == 0 && i < words) {
#pragma unroll
    for (int k = 1; k < GT_GM_SUM_SLICES; ++k) a += s[k][threadIdx.x];
    accout[i] += a;
  }
}
