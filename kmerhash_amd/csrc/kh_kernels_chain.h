// kh_kernels_chain.h -- gfx950 device code of kh_chain_anchors, included once by kmerhash_amd.hip after kh_kernels_csr.h.  Prefix k_chain_.
//
// Collinear chaining of oriented anchors (qpos, rpos, rev), segment by segment (definition: include/kmerhash_amd.h, model:
// tests/chain_model.py).  The DP is a dependent chain in the anchor index and parallel in its <= 64 candidates: one wavefront per
// segment, the last 64 anchors as a ring in registers (slot = (i - segment start) & 63 = lane), fields of anchor i broadcast with
// v_readlane, no LDS and no global-memory round trip between two anchors.
//   k_chain_dp      f and pred, i ascending: every lane scores its ring slot, one DPP max-reduction, a ballot for the tie rule
//   k_chain_link    i descending: g and best_child in a ring; then i ascending: the start anchor of every anchor's chain; count and last
//                   anchor are accumulated at the start anchor with global atomics
//   k_chain_emit<0> flags the kept start anchors;  scan(flags) with the index's scan kernels;  k_chain_emit<1> chain numbers and table rows
// Segment bounds are clamped to [0, m] wherever they are read, and every index that comes out of memory (pred, start anchor, last
// anchor) is range-checked before it addresses anything: offsets that do not ascend from 0 to m raise the `bad` word and the outputs
// are unspecified, but nothing outside the arrays is touched.
#pragma once
#include "kh_kernels_index.h"

#define KCH_THREADS 256
#define KCH_WAVES (KCH_THREADS / 64)
struct KchParams { uint32_t k, h, G, B; };

__device__ __forceinline__ uint32_t kch_rl(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ int kch_rl(int v, uint32_t l) { return __builtin_amdgcn_readlane(v, (int)l); }
// max over the wave, in every lane's return value: four row rotations (DPP row_ror 1, 2, 4, 8: all 16 lanes of a row hold the row's
// max), then one lane of each of the four rows.  EXEC must be full.
__device__ __forceinline__ int kch_wave_max(int v) {
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x121, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x122, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x124, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x128, 0xf, 0xf, false));
  return max(max(kch_rl(v, 0u), kch_rl(v, 16u)), max(kch_rl(v, 32u), kch_rl(v, 48u)));
}
// segment s clamped to [0, m]: a <= b <= m whatever seg holds.  REPORT: offsets that are no ascending partition of [0, m) raise *bad.
template <bool REPORT>
__device__ __forceinline__ void kch_segment(const uint64_t* __restrict__ seg, uint32_t n_seg, uint32_t s, uint32_t m, uint32_t lane, uint32_t* bad, uint32_t& a,
                                            uint32_t& b) {
  if (!seg) { a = 0; b = m; return; }
  const uint64_t lo = seg[s], hi = seg[(uint64_t)s + 1];
  a = lo < m ? (uint32_t)lo : m;
  b = hi < m ? (uint32_t)hi : m;
  if (b < a) b = a;
  if (REPORT) {
    const bool ok = lo <= hi && hi <= m && (s != 0 || lo == 0) && (s + 1 != n_seg || hi == m);
    if (!ok && lane == 0) atomicOr(bad, 1u);
  }
}
// the wave's first segment and its stride (wave-uniform by construction)
__device__ __forceinline__ uint32_t kch_first_segment() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * KCH_WAVES + (threadIdx.x >> 6))); }

__global__ __launch_bounds__(KCH_THREADS) void k_chain_dp(const uint32_t* __restrict__ qpos, const uint32_t* __restrict__ rpos, const uint8_t* __restrict__ rev, uint32_t m,
                                                          const uint64_t* __restrict__ seg, uint32_t n_seg, KchParams P, int32_t* __restrict__ out_f,
                                                          int32_t* __restrict__ out_pred, uint32_t* bad) {
  const uint32_t lane = threadIdx.x & 63, ns = seg ? n_seg : 1u, stride = gridDim.x * KCH_WAVES;
  const int k = (int)P.k;
  for (uint32_t s = kch_first_segment(); s < ns; s += stride) {
    uint32_t a, b;
    kch_segment<true>(seg, n_seg, s, m, lane, bad, a, b);
    uint32_t cq = 0, cr = 0, cv = 0; int cf = 0;               // the ring: anchor i lives in lane (i - a) & 63
    uint32_t nq = 0, nr = 0, nv = 0;                           // the tile being worked on, one anchor per lane
    if (a + lane < b) { nq = qpos[a + lane]; nr = rpos[a + lane]; nv = rev[a + lane]; }
    for (uint32_t t0 = a; t0 < b; t0 += 64) {
      const uint32_t cnt = b - t0 < 64u ? b - t0 : 64u;
      uint32_t pq = 0, pr = 0, pv = 0;                         // the next tile, in flight while this one is worked on
      if (b - t0 > 64u && t0 + 64u + lane < b) { pq = qpos[t0 + 64 + lane]; pr = rpos[t0 + 64 + lane]; pv = rev[t0 + 64 + lane]; }
      const bool older = t0 != a;                              // lanes >= step hold anchors of the tile before: are there any?
      int of = k, op = -1;
      for (uint32_t st = 0; st < cnt; ++st) {
        const uint32_t qi = kch_rl(nq, st), ri = kch_rl(nr, st), vi = kch_rl(nv, st) & 1u;
        int best = k, bp = -1;
        if (!((qi | ri) >> 31)) {
          const uint32_t d = lane < st ? st - lane : st - lane + 64u;          // i - j of this lane's slot
          bool ok = d <= P.h && (lane < st || older) && !((cq | cr) >> 31) && cv == vi;
          const uint32_t dq = qi - cq, dr = vi ? cr - ri : ri - cr;           // both operands < 2^31 where ok
          ok = ok && (int)dq >= 1 && dq <= P.G && (int)dr >= 1 && dr <= P.G;
          const int df = (int)(dq - dr);
          const uint32_t dd = df < 0 ? 0u - (uint32_t)df : (uint32_t)df;
          ok = ok && dd <= P.B;
          // (k * dd) >> 7 without 64-bit products: dd = 128 hi + lo
          const uint32_t cost = dd ? P.k * (dd >> 7) + ((P.k * (dd & 127u)) >> 7) + ((31u - (uint32_t)__clz((int)dd)) >> 1) : 0u;
          const uint32_t mn = min(min(dq, dr), P.k);
          int cand = (int)((uint32_t)cf + mn - cost);
          cand = ok && cand > k ? cand : k;
          const int mx = kch_wave_max(cand);
          if (mx > k) {                                        // ties go to the largest j: the highest lane below st, else the highest lane
            const unsigned long long eq = __ballot(cand == mx), low = eq & ((1ull << st) - 1ull);
            const uint32_t l = 63u - (uint32_t)__clzll((long long)(low ? low : eq));
            best = mx;
            bp = (int)(l < st ? t0 + l : t0 + l - 64u);
          }
        }
        if (lane == st) { cq = qi; cr = ri; cv = vi; cf = best; of = best; op = bp; }
      }
      if (lane < cnt) { out_f[t0 + lane] = of; out_pred[t0 + lane] = op; }
      nq = pq; nr = pr; nv = pv;
    }
  }
}

// is p a link the DP can have written for anchor i of segment [a, b)?  (guards the ring against anything else memory may hold)
__device__ __forceinline__ bool kch_pred_ok(int p, uint32_t i, uint32_t a) { return p >= 0 && (uint32_t)p >= a && (uint32_t)p < i && i - (uint32_t)p <= 64u; }

__global__ __launch_bounds__(KCH_THREADS) void k_chain_link(const int32_t* __restrict__ f, const int32_t* __restrict__ pred, uint32_t m, const uint64_t* __restrict__ seg,
                                                            uint32_t n_seg, int32_t* bc /*[m] scratch*/, int32_t* __restrict__ head /*[m]*/, uint32_t* __restrict__ count,
                                                            uint32_t* __restrict__ last) {
  const uint32_t lane = threadIdx.x & 63, ns = seg ? n_seg : 1u, stride = gridDim.x * KCH_WAVES;
  for (uint32_t s = kch_first_segment(); s < ns; s += stride) {
    uint32_t a, b;
    kch_segment<false>(seg, n_seg, s, m, lane, nullptr, a, b);
    if (a == b) continue;
    const uint32_t ntiles = (b - a + 63u) >> 6;
    // ---- i descending: g(i) = max(f(i), g of its children), best_child(i) = the child of greatest g, smallest index on ties
    {
      int nf = 0, np = -1;
      { const uint32_t i = a + (ntiles - 1) * 64 + lane; if (i < b) { nf = f[i]; np = pred[i]; } }
      int cg = 0, cbg = 0, cbc = -1;                            // the ring: g, the best child's g, the best child
      for (uint32_t T = ntiles; T-- > 0;) {
        const uint32_t t0 = a + T * 64, cnt = b - t0 < 64u ? b - t0 : 64u;
        int pf = 0, pp = -1;                                   // the tile below (whole whenever it exists)
        if (T) { pf = f[t0 - 64 + lane]; pp = pred[t0 - 64 + lane]; }
        if (T == ntiles - 1) cg = lane < cnt ? nf : pf;
        int obc = -1;
        for (uint32_t st = cnt; st-- > 0;) {
          const uint32_t i = t0 + st;
          const int gi = kch_rl(cg, st), p = kch_rl(np, st);
          // slot st is shared by i and i - 64: read i out and hand the slot to i - 64 BEFORE the update, which may be for i - 64
          if (lane == st) { obc = cbc; cg = pf; cbg = 0; cbc = -1; }
          if (kch_pred_ok(p, i, a) && lane == (((uint32_t)p - a) & 63u)) {
            if (cbc < 0 || gi >= cbg) { cbc = (int)i; cbg = gi; }
            cg = max(cg, gi);
          }
        }
        if (lane < cnt) bc[t0 + lane] = obc;
        nf = pf; np = pp;
      }
    }
    // ---- i ascending: i continues the chain of pred(i) iff it is its best child, else it starts one
    {
      int np = -1, nb = -1;
      if (a + lane < b) { np = pred[a + lane]; nb = bc[a + lane]; }
      int ch = 0, cb = -1;                                      // the ring: chain start, best child
      for (uint32_t t0 = a; t0 < b; t0 += 64) {
        const uint32_t cnt = b - t0 < 64u ? b - t0 : 64u;
        int pp = -1, pb = -1;
        if (b - t0 > 64u && t0 + 64u + lane < b) { pp = pred[t0 + 64 + lane]; pb = bc[t0 + 64 + lane]; }
        int oh = 0;
        for (uint32_t st = 0; st < cnt; ++st) {
          const uint32_t i = t0 + st;
          const int p = kch_rl(np, st);
          int hd = (int)i;
          if (kch_pred_ok(p, i, a)) {
            const uint32_t lp = ((uint32_t)p - a) & 63u;
            const int bcp = kch_rl(cb, lp), hp = kch_rl(ch, lp);
            if (bcp == (int)i) hd = hp;
          }
          if (lane == st) { ch = hd; cb = nb; oh = hd; }
        }
        if (lane < cnt) {                                      // (oh is i itself or came down the ring from an earlier i of this segment: a <= oh < b)
          head[t0 + lane] = oh;
          atomicAdd(&count[oh], 1u);
          atomicMax(&last[oh], t0 + lane);
        }
        np = pp; nb = pb;
      }
    }
  }
}

// PHASE 0: flag[i] = 1 iff i starts a chain that is kept.  PHASE 1 (after the scan of flag into num): out_chain[i] = the number of i's chain
// or -1, in place over the start anchors, and one table row per kept chain when there is a table and it is large enough.
template <int PHASE>
__global__ __launch_bounds__(256) void k_chain_emit(const int32_t* __restrict__ f, const int32_t* __restrict__ pred, int32_t* chain /*[m] in: start anchor*/, uint32_t m,
                                                    const uint32_t* __restrict__ count, const uint32_t* __restrict__ last, int32_t min_score, uint32_t min_count,
                                                    uint32_t* flag, const uint32_t* __restrict__ num, const unsigned long long* __restrict__ total, const uint32_t* __restrict__ bad,
                                                    uint32_t* __restrict__ c_first, uint32_t* __restrict__ c_last, uint32_t* __restrict__ c_count, int32_t* __restrict__ c_score,
                                                    uint64_t cap) {
  const uint32_t stride = gridDim.x * 256u;
  if (*bad) {                                                  // broken offsets: nothing below can be trusted; no chain is kept
    if (PHASE == 0) for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < m; i += stride) flag[i] = 0u;
    return;
  }
  const bool rows = PHASE == 1 && c_first && *total <= cap;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < m; i += stride) {
    const uint32_t h = (uint32_t)chain[i];
    if (PHASE == 0) {
      uint32_t keep = 0u;
      if (h == i) {
        const uint32_t l = last[i];
        const int p = pred[i];
        const int sc = (l < m ? f[l] : 0) - (p >= 0 && (uint32_t)p < m ? f[p] : 0);
        keep = sc >= min_score && count[i] >= min_count ? 1u : 0u;
      }
      flag[i] = keep;
    } else {
      const bool keep = h < m && flag[h];
      chain[i] = keep ? (int)num[h] : -1;
      if (rows && keep && h == i) {
        const uint32_t c = num[i], l = last[i];
        const int p = pred[i];
        c_first[c] = i; c_last[c] = l; c_count[c] = count[i];
        c_score[c] = (l < m ? f[l] : 0) - (p >= 0 && (uint32_t)p < m ? f[p] : 0);
      }
    }
  }
}
