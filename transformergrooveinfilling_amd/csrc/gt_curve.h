// Per-voice hit threshold curves (include/groove_hip.h: gt_hit_curve, gt_hit_thresholds).
//
// COUNTING.  Element e = m * 9 + c (row m, voice c) has a probability p and a class g = (ground-truth hit == 1); its bin is the number of
// grid values below p (fp32, strict; NaN -> 0).  counts[(c * 2 + g) * (n_thres + 1) + bin] += 1, in 64-bit integers: no rounding, so the
// result depends on neither the launch geometry nor on how a set is cut into calls.
//
// Kernel 1 (hit_curve_partial_kernel): a bounded, grid-stride number of 256-thread workgroups.  A workgroup walks chunks of 256 CONSECUTIVE
// elements -- thread t takes element chunk * 256 + t, so the probabilities of stride 9 are read as full lines -- and keeps 32-bit
// histograms in LDS.  The grid (at most 127 values, padded with +inf to 127) sits in LDS; the bin comes from a branch-free 7-step search.
// CONTENTION.  Real probabilities are skewed: most elements of a voice and class fall into one or two bins, and lanes of one wave that add
// to the same LDS word are served one after the other.  What was built: LANE-GROUP HISTOGRAM COPIES.  Inside a wave the lanes of one voice
// are l, l + 9, l + 18, ... (the elements are consecutive), so lane l adds into copy l / 9 (8 copies): two lanes of one wave instruction
// never meet on a word, whatever the data -- the one-bin case costs what the spread case costs.  A copy's stride is odd, so the 7 or 8
// lanes of one (voice, class, bin) also fall on different banks.  Waves of a workgroup share the copies; their adds are separate LDS
// instructions.  At 127 thresholds: 8 x (18 x 128 + 1) words + the grid = 72.5 KB of LDS, two workgroups per CU.
// The workgroup then sums its 8 copies and writes ALL 18 x (n_thres + 1) words of its slot of `scratch` (plain stores).
// Kernel 2 (hit_curve_sum_kernel): one thread per counter adds the workgroups' partials in 64 bits and adds the sum onto counts -- one
// writer per word, no global atomics.  A partial is at most ceil(chunks / workgroups) * 256 < 2^27: no 32-bit overflow below 2^31 rows.
// scratch has NO precondition and is left with the partials of the call: every word kernel 2 reads was written by kernel 1 of the same call.
//
// CHOICE (gt_curve_select): pure host code over the 64-bit counts, fp64 scores.
#pragma once
#include <math.h>

#include "gt_common.h"

#define GT_CURVE_THREADS 256
#define GT_CURVE_COPIES 8                      // ceil(64 / 9): lanes of one wave that share a voice
#define GT_CURVE_CLASSES (GT_VOICES * 2)
#define GT_CURVE_PAD 127                       // the searched grid: GT_CURVE_MAX_THRES values, the tail +inf
#define GT_CURVE_MAX_WGS 256
#define GT_CURVE_CHUNKS_PER_WG 8               // a workgroup is worth its histogram's zeroing and flush from ~2048 elements on
#define GT_CURVE_COPY_STRIDE (GT_CURVE_CLASSES * (GT_CURVE_MAX_THRES + 1) + 1)

struct CurveGrid { float t[GT_CURVE_PAD + 1]; };      // [0, n_thres) ascending, then +inf

__host__ __device__ static inline int64_t gt_curve_chunks(int64_t n_rows) { return (n_rows * GT_VOICES + GT_CURVE_THREADS - 1) / GT_CURVE_THREADS; }
static inline int gt_curve_wgs(int64_t n_rows) {
  const int64_t w = (gt_curve_chunks(n_rows) + GT_CURVE_CHUNKS_PER_WG - 1) / GT_CURVE_CHUNKS_PER_WG;
  return (int)(w < 1 ? 1 : w > GT_CURVE_MAX_WGS ? GT_CURVE_MAX_WGS : w);
}

__global__ __launch_bounds__(GT_CURVE_THREADS) void hit_curve_partial_kernel(const float* __restrict__ prob, int stride,
                                                                            const float* __restrict__ gt, int64_t n_rows, CurveGrid grid,
                                                                            int nb, unsigned* __restrict__ part) {
  __shared__ unsigned hist[GT_CURVE_COPIES * GT_CURVE_COPY_STRIDE];
  __shared__ float thr[GT_CURVE_PAD + 1];
  const int t = threadIdx.x;
  const int keys = GT_CURVE_CLASSES * nb;                 // counters in use; a copy's stride: keys | 1 (odd)
  const int cstride = keys | 1;
  for (int i = t; i < GT_CURVE_COPIES * cstride; i += GT_CURVE_THREADS) hist[i] = 0u;
  if (t <= GT_CURVE_PAD) thr[t] = grid.t[t];
  __syncthreads();
  unsigned* mine = hist + ((t & 63) / GT_VOICES) * cstride;
  const int64_t total = n_rows * GT_VOICES, chunks = gt_curve_chunks(n_rows);
  for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int64_t e0 = ch * GT_CURVE_THREADS;
    if (e0 + t < total) {
      const int q = (int)(e0 % GT_VOICES) + t;            // (e0 is the same for the whole workgroup: one 64-bit division per chunk)
      const int64_t m = e0 / GT_VOICES + q / GT_VOICES;
      const int c = q % GT_VOICES;
      const float p = prob[m * stride + c];
      const int g = gt[m * GT_TGT + c] == 1.0f ? 1 : 0;
      int b = 0;
#pragma unroll
      for (int step = 64; step >= 1; step >>= 1)
        if (p > thr[b + step - 1]) b += step;             // (NaN > x is false: bin 0; +inf padding is never passed)
      atomicAdd(&mine[(c * 2 + g) * nb + b], 1u);
    }
  }
  __syncthreads();
  unsigned* out = part + (size_t)blockIdx.x * keys;
  for (int i = t; i < keys; i += GT_CURVE_THREADS) {
    unsigned a = 0u;
#pragma unroll
    for (int k = 0; k < GT_CURVE_COPIES; ++k) a += hist[k * cstride + i];
    out[i] = a;
  }
}

__global__ __launch_bounds__(GT_CURVE_THREADS) void hit_curve_sum_kernel(const unsigned* __restrict__ part, int nwg, int keys,
                                                                        uint64_t* __restrict__ counts) {
  const int i = blockIdx.x * GT_CURVE_THREADS + threadIdx.x;
  if (i >= keys) return;
  uint64_t a = 0;
  for (int w = 0; w < nwg; ++w) a += part[(size_t)w * keys + i];
  counts[i] += a;
}

// the grid both entry points accept: 1..GT_CURVE_MAX_THRES values in [0, 1], strictly ascending (a NaN fails the range test)
static inline const char* gt_curve_grid_error(const float* thres, int32_t n_thres) {
  if (n_thres < 1 || n_thres > GT_CURVE_MAX_THRES) return "n_thres outside 1..GT_CURVE_MAX_THRES";
  for (int k = 0; k < n_thres; ++k) {
    if (!(thres[k] >= 0.f && thres[k] <= 1.f)) return "a threshold is NaN or outside [0, 1]";
    if (k && !(thres[k] > thres[k - 1])) return "the thresholds are not strictly ascending";
  }
  return nullptr;
}

// The F-beta score of one threshold from its integers, in fp64: (1 + b2) TP / ((1 + b2) TP + b2 FN + FP), each product rounded on its own
// and the sum taken left to right.  No fused multiply-add may be formed -- a contraction would make the last bit depend on the compiler --
// so contraction is switched off for this function by pragma (clang: the HIP build's host pass; GCC contracts only with an FMA target,
// which neither build selects, and takes the optimize attribute besides).
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
static double gt_curve_fbeta(double b2, uint64_t tp, uint64_t fn, uint64_t fp) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (tp == 0) return 0.0;
  const double a = (1.0 + b2) * (double)tp;
  const double bfn = b2 * (double)fn;
  const double den = (a + bfn) + (double)fp;
  return a / den;
}

// One voice: cnt = its 2 x (n_thres + 1) counters [class][bin].  criterion 0: the k of the largest F-beta; 1: the k whose number of placed
// hits TP + FP is nearest the number of true hits P.  Of equal candidates the lower median.  Returns the index, or -1 (the fallback).
static int gt_curve_choose(const uint64_t* cnt, int n_thres, int criterion, double b2, uint64_t* tp_o, uint64_t* fp_o, uint64_t* p_o) {
  const int nb = n_thres + 1;
  uint64_t P = 0, tp[GT_CURVE_MAX_THRES], fp[GT_CURVE_MAX_THRES];
  for (int b = 0; b < nb; ++b) P += cnt[nb + b];
  uint64_t st = 0, sf = 0;
  for (int k = n_thres - 1; k >= 0; --k) {                  // TP_k = sum over bins > k
    st += cnt[nb + k + 1];
    sf += cnt[k + 1];
    tp[k] = st;
    fp[k] = sf;
  }
  *p_o = P;
  if (P == 0) return -1;
  int first[GT_CURVE_MAX_THRES], n = 0;
  if (criterion == 0) {
    double best = 0.0;
    for (int k = 0; k < n_thres; ++k) {
      const double s = gt_curve_fbeta(b2, tp[k], P - tp[k], fp[k]);
      if (s > best) { best = s; n = 0; }
      if (s == best) first[n++] = k;
    }
    if (!(best > 0.0)) return -1;
  } else {
    uint64_t best = ~0ull;
    for (int k = 0; k < n_thres; ++k) {
      const uint64_t placed = tp[k] + fp[k], dist = placed > P ? placed - P : P - placed;
      if (dist < best) { best = dist; n = 0; }
      if (dist == best) first[n++] = k;
    }
  }
  const int k = first[(n - 1) / 2];
  *tp_o = tp[k];
  *fp_o = fp[k];
  return k;
}
