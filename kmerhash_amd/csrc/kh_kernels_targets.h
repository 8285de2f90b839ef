// kh_kernels_targets.h -- gfx950 device code of kh_anchor_targets, included once by kmerhash_amd.hip after kh_kernels_records.h.  Prefix
// k_target_.
//
// kh_anchor_targets regroups the anchors of every segment (read) by the target (contig) their reference position falls in, so that
// the segments handed to kh_chain_anchors are (read, target) groups and no chain crosses a contig (definition:
// include/kmerhash_amd.h, model: tests/targets_model.py).  Integers only; no atomics on anchor data: the order is a function of the
// input alone.
//   k_target_find<STAGED>  one lane per anchor: the upper-bound binary search of rpos in t_start, then the three conditions of a
//                          target id.  STAGED: both tables are copied into dynamic LDS once per workgroup (8 n_t bytes) and searched
//                          there; otherwise they are searched through L2
//   k_target_group<EMIT>   one wavefront per segment, fixed grid, grid-stride over the segments.  One step per distinct id of the
//                          segment, ascending (KTG_NONE is the largest uint32, so "NONE last" is the plain unsigned order): the wave
//                          walks the segment 64 anchors per tile, ballots the lanes that hold the current id, places them by mbcnt
//                          behind the running offset and collects the smallest id above the current one for the next step.  A
//                          segment of at most 64 anchors keeps its ids in registers; a longer one reloads its tiles every step
//                          ((distinct ids) x (tiles) tile visits).  EMIT = false counts the groups of every segment and raises *bad
//                          for offsets that are no ascending partition of [0, m); the index's scan kernels turn the counts into each
//                          segment's first group; EMIT = true writes the permuted anchors and the group rows, and nothing at all
//                          when *bad is set
// Segment bounds are clamped to [0, m] by kch_segment, the chain kernels' own; a group row is written only below m and an anchor
// only inside its own segment, so nothing outside the arrays is touched whatever the offsets hold.
#pragma once
#include "kh_kernels_chain.h"

#define KTG_THREADS 256
#define KTG_WAVES (KTG_THREADS / 64)
#define KTG_NONE 0xFFFFFFFFu      // KH_TARGET_NONE, and KH_POS_INVALID for the rpos of such an anchor

struct KtgIn {
  const uint32_t* qpos; const uint32_t* rpos; const uint8_t* rev; const uint64_t* seg;
  uint32_t m, n_seg;
};
struct KtgOut {
  uint32_t *q, *r; uint8_t* v; uint32_t *tid, *src;
  uint64_t* g_off; uint32_t *g_seg, *g_tid;
};

// the definition's loop, word for word: the upper bound of r in ts[0, n_t), minus one; then the three conditions
__device__ __forceinline__ uint32_t ktg_lookup(const uint32_t* ts, const uint32_t* te, uint32_t n_t, uint32_t r, uint32_t k) {
  uint32_t lo = 0, hi = n_t;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (ts[mid] <= r) lo = mid + 1u; else hi = mid;
  }
  if (lo == 0u || (r >> 31)) return KTG_NONE;
  return r + k <= te[lo - 1u] ? lo - 1u : KTG_NONE;      // (r < 2^31, k <= 64: the sum does not wrap)
}

template <bool STAGED>
__global__ __launch_bounds__(KTG_THREADS) void k_target_find(const uint32_t* __restrict__ rpos, uint32_t m, const uint32_t* __restrict__ t_start,
                                                             const uint32_t* __restrict__ t_end, uint32_t n_t, uint32_t k, uint32_t* __restrict__ tid) {
  extern __shared__ __attribute__((aligned(16))) uint32_t ktg_tables[];      // STAGED: t_start[n_t], then t_end[n_t]
  if (STAGED) {
    for (uint32_t j = threadIdx.x; j < n_t; j += KTG_THREADS) { ktg_tables[j] = t_start[j]; ktg_tables[n_t + j] = t_end[j]; }
    __syncthreads();
  }
  const uint32_t stride = gridDim.x * KTG_THREADS;
  for (uint32_t i = blockIdx.x * KTG_THREADS + threadIdx.x; i < m; i += stride)      // (m <= 2^24: i does not wrap)
    tid[i] = STAGED ? ktg_lookup(ktg_tables, ktg_tables + n_t, n_t, rpos[i], k) : ktg_lookup(t_start, t_end, n_t, rpos[i], k);
}

__device__ __forceinline__ uint32_t ktg_wave_min(uint32_t v) {
  for (int d = 1; d < 64; d <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d));
  return v;
}
// the number of set bits of `mask` below this lane
__device__ __forceinline__ uint32_t ktg_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

template <bool EMIT>
__global__ __launch_bounds__(KTG_THREADS) void k_target_group(KtgIn P, const uint32_t* __restrict__ tid, uint32_t* __restrict__ counts /*[segments]*/,
                                                              const uint64_t* __restrict__ first_grp /*[segments + 1]*/, uint32_t* bad, KtgOut O) {
  const uint32_t lane = threadIdx.x & 63, ns = P.seg ? P.n_seg : 1u, stride = gridDim.x * KTG_WAVES, m = P.m;
  if (EMIT) {
    if (*bad) return;                                          // broken offsets: the counts cannot be trusted; nothing is written
    const uint64_t total = first_grp[ns];
    if (total > m) return;                                     // (a partition of m anchors has at most m groups)
    if (blockIdx.x == 0 && threadIdx.x == 0) O.g_off[total] = m;
  }
  for (uint32_t s = kch_first_segment(); s < ns; s += stride) {
    uint32_t a, b;
    kch_segment<!EMIT>(P.seg, P.n_seg, s, m, lane, bad, a, b);
    if (a == b) { if (!EMIT && lane == 0) counts[s] = 0u; continue; }
    const bool single = b - a <= 64u;
    const uint64_t g0 = EMIT ? first_grp[s] : 0ull;
    // the smallest id of the segment (a lane outside it holds KTG_NONE, as an anchor without a target does: `in` tells them apart)
    uint32_t reg = KTG_NONE, mn = KTG_NONE;
    for (uint32_t t0 = a; t0 < b; t0 += 64u) {
      const uint32_t i = t0 + lane;
      if (i < b) { reg = tid[i]; mn = min(mn, reg); }
    }
    mn = ktg_wave_min(mn);
    uint32_t off = 0, j = 0;
    for (;;) {                                                 // one step per distinct id, ascending
      const uint32_t off0 = off;
      uint32_t nx = KTG_NONE;
      bool more = false;
      for (uint32_t t0 = a; t0 < b; t0 += 64u) {
        const uint32_t i = t0 + lane;
        const bool in = i < b;
        const uint32_t t = single ? reg : in ? tid[i] : KTG_NONE;
        const bool hit = in && t == mn;
        const unsigned long long hits = __ballot(hit);
        if (EMIT && hit) {                                     // input order inside the group: tile by tile, lane by lane
          const uint32_t d = a + off + ktg_below(hits);        // (< b: every anchor of the segment is placed exactly once)
          O.q[d] = P.qpos[i]; O.r[d] = t == KTG_NONE ? KTG_NONE : P.rpos[i]; O.v[d] = P.rev[i]; O.tid[d] = t; O.src[d] = i;
        }
        off += (uint32_t)__popcll(hits);
        if (in && t > mn) { nx = min(nx, t); more = true; }
      }
      if (EMIT && lane == 0 && g0 + j < m) { O.g_off[g0 + j] = a + off0; O.g_seg[g0 + j] = s; O.g_tid[g0 + j] = mn; }
      ++j;
      if (!__ballot(more)) break;
      mn = ktg_wave_min(nx);
    }
    if (!EMIT && lane == 0) counts[s] = j;
  }
}
