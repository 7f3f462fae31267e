// Groove descriptors and rhythmic distances per sequence (include/groove_hip.h: gt_groove_features): per sequence and buffer a record of 32
// 64-bit integers (hit-mask counts, fixed-point velocity / offset sums, the circular autocorrelation of the velocity profile), and per
// sequence eight more that compare buffer a with buffer b.  Integers throughout, every word STORED by exactly one thread: the result depends
// on neither the launch geometry nor on a sequence's position in the set.
//
// ONE launch: a bounded, grid-stride number of 64-thread workgroups -- one wavefront, ONE sequence per workgroup and iteration.  The 864
// floats of a sequence and buffer (16-byte aligned: 3456 bytes) come in as 216 float4 loads; the loads of the NEXT sequence are issued
// before the current one is processed (gt_group.h's staging), so a wavefront always has a sequence in flight.
// Phase A: lane (t = lane % 32, half = lane / 32) evaluates step t, voices 0..4 (half 0) or 5..8 (half 1), of BOTH buffers -- the pair terms
//   need the two buffers' values of a cell in one place.  It leaves in LDS: 17 64-bit partials (the five value sums of each buffer, the
//   two pair sums, the five small counts), its part of the hit bits of step t and of the profile P[t] of each buffer.
// Phase B: lanes 0..16 are the OWNERS of the 17 summed words: each adds the 64 partials of its row (rows padded to 65 words: the owners
//   read 17 different banks) and stores the word; lanes 32..49 turn the hit bits into a 32-bit mask per (buffer, voice); every lane adds the
//   two halves of one P[t].
// Phase C: lanes 0..33 own one autocorrelation lag of one buffer (32 multiply-adds of 24-bit values into 64 bits), lane 34 the profile
//   product of the pair, lanes 35 / 36 the seven mask-count words of a buffer's record, lane 37 the three of the pair: population counts
//   of mask expressions.
// The emulator build has neither a ballot nor a population count: the masks go through LDS with owner lanes, and gt_gf_popc below is the
// one shim.
#pragma once
#include "gt_group.h"                              // gt_gm_fix

#define GT_GF_THREADS 64
#define GT_GF_Q (32 * GT_TGT / 4)                 // float4 per sequence and buffer (216)
#define GT_GF_LOADS ((GT_GF_Q + GT_GF_THREADS - 1) / GT_GF_THREADS)
#define GT_GF_ROWS 17                             // summed words: 5 + 5 value sums, 2 pair sums, 2 + 2 rejected counts, 1 pair count
#define GT_GF_PITCH 65
#define GT_GF_LAGS 17

// workgroups: at most 8 per CU's worth (17 KB of LDS each admit 9 beside one another; 512 / 1024 / 2048 / 4096 measured, DESIGN.md "Groove
// descriptors"), and never more than half the sequences -- a workgroup that walks two or more keeps the next one's loads in flight
static inline int gt_gf_wgs(int64_t n_seq) {
  int64_t w = (n_seq + 1) / 2;
  if (w > 2048) w = 2048;
  return (int)(w < 1 ? 1 : w);
}

#ifdef GT_EMU
static inline int gt_gf_popc(const uint32_t x) { return __builtin_popcount(x); }
#else
__device__ static inline int gt_gf_popc(const uint32_t x) { return __popc(x); }
#endif

// q(v): 16 fractional bits of a valid velocity (0..16 -> below 2^21; nine of them below 2^24)
__device__ static inline uint32_t gt_gf_q(const float v) { return (uint32_t)((double)v * 65536.0 + 0.5); }

struct GfCell { bool hit, okv, oko; float v, o; };

// One cell of one buffer: adds its values onto the lane's five sums (s: words 9..13 of the record), its rejected values onto rv / ro, its
// bit onto hb and its quantised velocity onto prof.  -> what the pair terms need of it.
__device__ static inline GfCell gt_gf_cell(const float* __restrict__ row, const int c, uint64_t* s, unsigned& rv, unsigned& ro, unsigned& hb,
                                           uint32_t& prof) {
  GfCell r;
  r.hit = row[c] == 1.0f;
  r.v = 0.f; r.o = 0.f; r.okv = false; r.oko = false;
  if (r.hit) {
    const float v = row[GT_VOICES + c], o = row[2 * GT_VOICES + c];
    hb |= 1u << c;
    r.okv = 0.0f <= v && v <= 16.0f;                 // (a NaN fails both)
    r.oko = fabsf(o) <= 16.0f;
    if (r.okv) {
      const float vv = v * v;
      r.v = v;
      prof += gt_gf_q(v);
      s[0] += gt_gm_fix(v);
      s[1] += gt_gm_fix(vv);
    } else ++rv;
    if (r.oko) {
      const float oo = o * o;
      r.o = o;
      s[2] += gt_gm_fix(fabsf(o));
      if (o >= 0.0f) s[3] += gt_gm_fix(o); else s[3] -= gt_gm_fix(-o);       // two's complement
      s[4] += gt_gm_fix(oo);
    } else ++ro;
  }
  return r;
}

__global__ __launch_bounds__(GT_GF_THREADS) void groove_features_kernel(const float* __restrict__ hvo_a, const float* __restrict__ hvo_b,
                                                                       const int64_t n_seq, uint64_t* __restrict__ feat_a,
                                                                       uint64_t* __restrict__ feat_b, uint64_t* __restrict__ pair) {
  __shared__ float4 sa[GT_GF_Q], sb[GT_GF_Q];
  __shared__ uint64_t spart[GT_GF_ROWS][GT_GF_PITCH];
  __shared__ unsigned shb[2][GT_GF_THREADS];       // [buffer][lane]: the hit bits (bit c) of the lane's step and voices
  __shared__ uint32_t spp[2][GT_GF_THREADS];       // [buffer][lane]: the lane's part of P[t]
  __shared__ uint32_t sP[2][32];
  __shared__ uint32_t smask[2][GT_VOICES + 1];
  const int lane = threadIdx.x;
  const bool has_b = hvo_b != nullptr && (feat_b != nullptr || pair != nullptr);
  const float4* ga = reinterpret_cast<const float4*>(hvo_a);
  const float4* gb = reinterpret_cast<const float4*>(hvo_b);
  float4 ra[GT_GF_LOADS], rb[GT_GF_LOADS];
  int64_t s = blockIdx.x;                                   // (the grid never has more workgroups than sequences)
#pragma unroll
  for (int i = 0; i < GT_GF_LOADS; ++i) {
    const int q = lane + i * GT_GF_THREADS;
    ra[i] = rb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < GT_GF_Q) {
      ra[i] = ga[s * GT_GF_Q + q];
      if (has_b) rb[i] = gb[s * GT_GF_Q + q];
    }
  }
  for (; s < n_seq; s += gridDim.x) {
#pragma unroll
    for (int i = 0; i < GT_GF_LOADS; ++i) {
      const int q = lane + i * GT_GF_THREADS;
      if (q < GT_GF_Q) { sa[q] = ra[i]; sb[q] = rb[i]; }
    }
    const int64_t nx = s + gridDim.x;
    if (nx < n_seq) {                                       // the next sequence is under way while this one is processed
#pragma unroll
      for (int i = 0; i < GT_GF_LOADS; ++i) {
        const int q = lane + i * GT_GF_THREADS;
        if (q < GT_GF_Q) {
          ra[i] = ga[nx * GT_GF_Q + q];
          if (has_b) rb[i] = gb[nx * GT_GF_Q + q];
        }
      }
    }
    __syncthreads();
    {                                                       // ---- phase A: step t, voices c0 .. c0 + nc - 1, both buffers
      const int t = lane & 31, c0 = lane < 32 ? 0 : 5, nc = lane < 32 ? 5 : 4;
      const float* rowa = reinterpret_cast<const float*>(sa) + t * GT_TGT;
      const float* rowb = reinterpret_cast<const float*>(sb) + t * GT_TGT;
      uint64_t xa[5] = {0ull, 0ull, 0ull, 0ull, 0ull}, xb[5] = {0ull, 0ull, 0ull, 0ull, 0ull}, pv = 0ull, po = 0ull;
      unsigned rva = 0u, roa = 0u, rvb = 0u, rob = 0u, hba = 0u, hbb = 0u, both = 0u;
      uint32_t pa = 0u, pb = 0u;
      for (int i = 0; i < nc; ++i) {
        const int c = c0 + i;
        const GfCell a = gt_gf_cell(rowa, c, xa, rva, roa, hba, pa);
        if (has_b) {
          const GfCell b = gt_gf_cell(rowb, c, xb, rvb, rob, hbb, pb);
          if (a.hit || b.hit) {
            const float dv = a.v - b.v;                     // (v' = 0 where there is no hit or no valid velocity)
            const float ev = dv * dv;
            pv += gt_gm_fix(ev);
            if (a.hit && b.hit && a.oko && b.oko) {
              const float d = a.o - b.o;
              const float eo = d * d;
              po += gt_gm_fix(eo);
              ++both;
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 5; ++k) { spart[k][lane] = xa[k]; spart[5 + k][lane] = xb[k]; }
      spart[10][lane] = pv; spart[11][lane] = po;
      spart[12][lane] = rva; spart[13][lane] = roa; spart[14][lane] = rvb; spart[15][lane] = rob; spart[16][lane] = both;
      shb[0][lane] = hba; shb[1][lane] = hbb;
      spp[0][lane] = pa; spp[1][lane] = pb;
    }
    __syncthreads();
    if (lane < GT_GF_ROWS) {                                // ---- phase B: the owner of one summed word, its only writer
      uint64_t a = 0ull;
#pragma unroll 8
      for (int i = 0; i < GT_GF_THREADS; ++i) a += spart[lane][i];
      // rows 0..4 / 5..9: words 9..13 of a / b; 10, 11: pair 3, 4; 12, 13 / 14, 15: words 7, 8 of a / b; 16: pair 5
      uint64_t* dst = lane < 5    ? feat_a + s * GT_GF_WORDS + 9 + lane
                      : lane < 10 ? (feat_b ? feat_b + s * GT_GF_WORDS + 4 + lane : nullptr)
                      : lane < 12 ? (pair ? pair + s * GT_GF_PAIR_WORDS + lane - 7 : nullptr)
                      : lane < 14 ? feat_a + s * GT_GF_WORDS + lane - 5
                      : lane < 16 ? (feat_b ? feat_b + s * GT_GF_WORDS + lane - 7 : nullptr)
                                  : (pair ? pair + s * GT_GF_PAIR_WORDS + 5 : nullptr);
      if (dst) *dst = a;
    } else if (lane >= 32 && lane < 32 + 2 * GT_VOICES) {   // the mask of (buffer, voice): bit t = a hit at step t
      const int buf = (lane - 32) / GT_VOICES, c = (lane - 32) % GT_VOICES;
      const unsigned* hb = shb[buf] + (c < 5 ? 0 : 32);
      uint32_t m = 0u;
#pragma unroll 8
      for (int t = 0; t < 32; ++t) m |= ((hb[t] >> c) & 1u) << t;
      smask[buf][c] = m;
    }
    sP[lane >> 5][lane & 31] = spp[lane >> 5][lane & 31] + spp[lane >> 5][32 + (lane & 31)];
    __syncthreads();
    if (lane < 2 * GT_GF_LAGS + 1) {                        // ---- phase C: one lag of one buffer; lane 34: the pair's profile product
      const int buf = lane < GT_GF_LAGS ? 0 : 1, l = lane < 2 * GT_GF_LAGS ? lane - buf * GT_GF_LAGS : 0;
      const uint32_t* X = lane < 2 * GT_GF_LAGS ? sP[buf] : sP[0];
      const uint32_t* Y = sP[buf];
      uint64_t* dst = lane < GT_GF_LAGS       ? feat_a + s * GT_GF_WORDS + 15 + l
                      : lane < 2 * GT_GF_LAGS ? (feat_b ? feat_b + s * GT_GF_WORDS + 15 + l : nullptr)
                                              : (pair ? pair + s * GT_GF_PAIR_WORDS + 6 : nullptr);
      if (dst) {
        uint64_t a = 0ull;
#pragma unroll 8
        for (int t = 0; t < 32; ++t) a += (uint64_t)X[t] * (uint64_t)Y[(t + l) & 31];
        *dst = a;
      }
    } else if (lane < 2 * GT_GF_LAGS + 3) {                 // lanes 35 / 36: words 0..6 and the reserved word 14 of a buffer's record
      const int buf = lane - (2 * GT_GF_LAGS + 1);
      uint64_t* dst = buf == 0 ? feat_a + s * GT_GF_WORDS : (feat_b ? feat_b + s * GT_GF_WORDS : nullptr);
      if (dst) {
        unsigned hits = 0u, voices = 0u, any = 0u, w3 = 0u, w4 = 0u, w5 = 0u, w6 = 0u;
#pragma unroll
        for (int c = 0; c < GT_VOICES; ++c) {
          const uint32_t m = smask[buf][c];
          hits += gt_gf_popc(m);
          voices += m != 0u;
          any |= m;
          w3 += gt_gf_popc(m & 0x11111111u);
          w4 += gt_gf_popc(m & 0x44444444u);
          w5 += gt_gf_popc(m & 0xAAAAAAAAu);
          w6 += gt_gf_popc(m & (m >> 16) & 0xFFFFu);
        }
        dst[0] = hits; dst[1] = voices; dst[2] = (unsigned)gt_gf_popc(any); dst[3] = w3; dst[4] = w4; dst[5] = w5; dst[6] = w6;
        dst[14] = 0ull;
      }
    } else if (lane == 2 * GT_GF_LAGS + 3 && pair) {        // lane 37: Hamming, hit in both, near misses; the reserved word 7
      unsigned ham = 0u, both = 0u, near = 0u;
#pragma unroll
      for (int c = 0; c < GT_VOICES; ++c) {
        const uint32_t p = smask[0][c], g = smask[1][c], fp = p & ~g, fn = g & ~p;
        ham += gt_gf_popc(p ^ g);
        both += gt_gf_popc(p & g);
        near += gt_gf_popc(fp & ((g << 1) | (g >> 1))) + gt_gf_popc(fn & ((p << 1) | (p >> 1)));
      }
      uint64_t* dst = pair + s * GT_GF_PAIR_WORDS;
      dst[0] = ham; dst[1] = both; dst[2] = near; dst[7] = 0ull;
    }
    // (no barrier here: the next iteration writes sa / sb, which nobody reads after phase A, then meets the one behind the staging)
  }
}
