// kh_kernels_edits.h -- gfx950 device code of kh_chain_edits, included once by kmerhash_amd.hip after kh_kernels_chain.h.  Prefix k_edits_.
//
// Unit-cost edit distance of every link of every kept chain (definition: include/kmerhash_amd.h, model: tests/edits_model.py).  A link
// is anchor i with its predecessor j = pred(i) in the same kept chain; A = the query bases [q_j, q_i), B = the reference bases A faces.
//   k_edits_classify  one lane per anchor: link or not, the range checks, and where |A| == |B| a direct compare, 8 bases per step; what
//                     is not settled goes onto a worklist of anchor indices, one reservation per wave (ked_wave_reserve)
//   k_edits_wfa       one wavefront per worklist entry, fixed grid, grid-stride over the device-side count: furthest-reaching points
//                     (Landau-Vishkin) with one diagonal per lane, neighbours by lane shuffles, the points in one register per lane
// Orientation of k_edits_wfa: lane l owns diagonal d = l - 32 = (offset in B) - (offset in A); F[d] is the furthest offset in A reached
// on d with e edits.  e -> e + 1: F[d] = max(F[d - 1], F[d] + 1, F[d + 1] + 1) -- a base of B skipped, a substitution, a base of A
// skipped -- clamped to min(|A|, |B| - d), then extended while the bases match.  The link is done at the first e at which lane
// |B| - |A| + 32 holds |A|.  Lane 0 (d = -32) stays empty: |d| <= 31 = the largest max_edits.
// Bases: the byte with bit 5 cleared must be one of A C G T; its code is bits 1..2 (A 0, C 1, T 2, G 3), so the complement is code ^ 2.
// Eight bytes are turned into eight codes at a time, an invalid byte gets bit 7 and matches nothing.
// Every index that comes out of memory (pred, chain, worklist entry) is range-checked before it addresses anything, in both kernels;
// text offsets follow from the range checks of ked_link, and an 8-byte load is only issued where all 8 bytes lie inside the text.
#pragma once
#include "kh_kernels_chain.h"

#define KED_THREADS 256
#define KED_WAVES (KED_THREADS / 64)
#define KED_NOLINK (-1)
#define KED_OVER (-2)
#define KED_NEG (-(1 << 20))        // an unreached diagonal: stays negative under the <= 32 increments of a link

struct KedArgs {
  const uint8_t* qtext; const uint8_t* rtext;
  const uint32_t* qpos; const uint32_t* rpos; const uint8_t* rev; const int32_t* pred; const int32_t* chain;
  uint32_t nq, nr, ref_base, m, n_chains, k, max_edits;
};
// a link that passed the range checks: A = qtext[a0, a0 + dq); B forward = rtext[b0, b0 + dr), B reverse = the complement of
// rtext[b0 - dr, b0) read downwards from b0 - 1
struct KedLink {
  uint32_t a0, b0, rev; int dq, dr, chain;
  __device__ __forceinline__ uint32_t a_down() const { return 0u; }      // (how ked_extend reads the two strings)
  __device__ __forceinline__ uint32_t b_down() const { return rev; }
  __device__ __forceinline__ uint32_t comp() const { return rev; }
};

#define KED_B(x) (0x0101010101010101ull * (uint64_t)(x))
// bit 7 of every byte of v that is not zero (exact: no carry leaves a byte)
__device__ __forceinline__ uint64_t ked_nonzero(uint64_t v) { return (((v & KED_B(0x7f)) + KED_B(0x7f)) | v) & KED_B(0x80); }
// eight text bytes -> eight codes: 0..3, or bit 7 set for a byte that is no base
__device__ __forceinline__ uint64_t ked_codes(uint64_t w) {
  const uint64_t u = w & KED_B(0xdf);                                   // case folded
  const uint64_t c = (u >> 1) & KED_B(0x03), c0 = c & KED_B(0x01), c1 = (c >> 1) & KED_B(0x01);
  const uint64_t cg = c0 & c1, t = c1 & ~c0;                            // G: 01000111, T: 01010100
  const uint64_t expect = KED_B(0x41) ^ (c0 << 1) ^ (cg << 2) ^ t ^ (t << 2) ^ (t << 4);
  return c | ked_nonzero(u ^ expect);
}
// text[pos, pos + 8) with byte t in bits 8t..; bytes at or beyond n come as 0 (no base).  pos <= n.
// (The padding bounds the READ, not the result: ked_extend cuts every run at hi, which lies inside both strings, so no caller ever
//  looks at a byte at or beyond n, and no result test can tell the zero from whatever lies behind the text.)
__device__ __forceinline__ uint64_t ked_load_up(const uint8_t* __restrict__ text, uint32_t n, uint32_t pos) {
  uint64_t w = 0;
  if (n - pos >= 8u) { __builtin_memcpy(&w, text + pos, 8); return w; }
  for (uint32_t t = 0; t < n - pos; ++t) w |= (uint64_t)text[pos + t] << (8u * t);
  return w;
}
// text[end - 1], text[end - 2], ... with byte t in bits 8t..; bytes below 0 come as 0.  end <= the text's length.
__device__ __forceinline__ uint64_t ked_load_down(const uint8_t* __restrict__ text, uint32_t end) {
  uint64_t w = 0;
  if (end >= 8u) { __builtin_memcpy(&w, text + (end - 8u), 8); return __builtin_bswap64(w); }
  for (uint32_t t = 0; t < end; ++t) w |= (uint64_t)text[end - 1u - t] << (8u * t);
  return w;
}
// from offset i in A on diagonal d: the offset after the run of matching bases, at most hi (= min(|A|, |B| - d): inside both strings).
// STR says how the two strings lie in the texts: a string read upwards from x has its base t at text[x + t], one read downwards from x at
// text[x - 1 - t]; comp(): B's bases are complemented.  A link (KedLink) reads A upwards and B upwards, or downwards and complemented on
// the reverse strand; the ends of a chain (KenEnd, kh_kernels_ends.h) run away from the seed in all four ways.
template <typename STR>
__device__ __forceinline__ int ked_extend(const KedArgs& P, const STR& L, int i, int d, int hi) {
  while (i < hi) {
    const uint64_t a = ked_codes(L.a_down() ? ked_load_down(P.qtext, L.a0 - (uint32_t)i) : ked_load_up(P.qtext, P.nq, L.a0 + (uint32_t)i));
    const uint32_t j = (uint32_t)(i + d);
    const uint64_t b = L.b_down() ? ked_codes(ked_load_down(P.rtext, L.b0 - j)) ^ (L.comp() ? KED_B(0x02) : 0ull)
                                  : ked_codes(ked_load_up(P.rtext, P.nr, L.b0 + j)) ^ (L.comp() ? KED_B(0x02) : 0ull);
    const uint64_t bad = ked_nonzero((a ^ b) | (a & KED_B(0x80)));     // a valid and equal to b: b is valid too
    int run = bad ? (int)((uint32_t)__builtin_ctzll(bad) >> 3) : 8;
    run = min(run, hi - i);
    i += run;
    if (bad) break;
  }
  return i;
}
// does anchor i have a link, and is it inside the texts?  KED_NOLINK, KED_OVER (L.chain is set), or 0 with L filled in
__device__ __forceinline__ int ked_link(const KedArgs& P, uint32_t i, KedLink& L) {
  const int c = P.chain[i], p = P.pred[i];
  if (c < 0 || (uint32_t)c >= P.n_chains || p < 0 || (uint32_t)p >= i) return KED_NOLINK;
  if (P.chain[p] != c) return KED_NOLINK;
  L.chain = c;
  const uint32_t qi = P.qpos[i], qj = P.qpos[p], ri = P.rpos[i], rj = P.rpos[p], rv = P.rev[i] & 1u;
  if ((qi | qj | ri | rj) >> 31) return KED_OVER;
  const int dq = (int)qi - (int)qj, dr = rv ? (int)rj - (int)ri : (int)ri - (int)rj;
  if (dq < 1 || dr < 1 || (uint64_t)qi + P.k > P.nq) return KED_OVER;
  const int64_t lo = (int64_t)(rv ? ri + P.k : rj) - (int64_t)P.ref_base, hi = lo + dr;      // B's stretch of rtext
  if (lo < 0 || hi > (int64_t)P.nr) return KED_OVER;
  const int dd = dq - dr;
  if ((uint32_t)(dd < 0 ? -dd : dd) > P.max_edits) return KED_OVER;
  L.a0 = qj; L.b0 = (uint32_t)(rv ? hi : lo); L.rev = rv; L.dq = dq; L.dr = dr;
  return 0;
}
// one reservation per wave on a worklist, called by whole waves: the first queued lane adds the wave's count to *wl_count, every queued
// lane takes its rank behind that base and puts anchor i into that slot of wl; a lane that does not queue writes nothing.  (The slot is
// used here and not returned: handing it to the caller cost k_edits_classify one more VGPR and k_cigar_classify two.)
__device__ __forceinline__ void ked_wave_reserve(bool queue, uint32_t lane, uint32_t i, uint32_t* __restrict__ wl, uint32_t* __restrict__ wl_count) {
  const unsigned long long mask = __ballot(queue);
  if (mask) {
    const uint32_t leader = (uint32_t)__builtin_ctzll(mask);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(wl_count, (uint32_t)__popcll(mask));
    base = (uint32_t)__shfl((int)base, (int)leader);
    if (queue) wl[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = i;      // (at most one entry per anchor: base + rank < m)
  }
}

__global__ __launch_bounds__(KED_THREADS) void k_edits_classify(KedArgs P, int32_t* __restrict__ out_link, uint32_t* __restrict__ c_over, uint32_t* __restrict__ wl,
                                                                uint32_t* __restrict__ wl_count) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KED_THREADS;
  for (uint32_t i0 = blockIdx.x * KED_THREADS + (threadIdx.x & ~63u); i0 < P.m; i0 += stride) {      // (i0 is the same in a whole wave)
    const uint32_t i = i0 + lane;
    bool queue = false;
    if (i < P.m) {
      KedLink L;
      int res = ked_link(P, i, L);
      if (res == 0) {
        if (L.dq == L.dr && ked_extend(P, L, 0, 0, L.dq) == L.dq) out_link[i] = 0;
        else queue = true;
      } else {
        out_link[i] = res;
        if (res == KED_OVER) atomicAdd(&c_over[L.chain], 1u);
      }
    }
    ked_wave_reserve(queue, lane, i, wl, wl_count);
  }
}

__global__ __launch_bounds__(KED_THREADS) void k_edits_wfa(KedArgs P, const uint32_t* __restrict__ wl, const uint32_t* __restrict__ wl_count, int32_t* __restrict__ out_link,
                                                           uint32_t* __restrict__ c_edits, uint32_t* __restrict__ c_over) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KED_WAVES;
  const uint32_t n = min(*wl_count, P.m);
  const int d = (int)lane - 32;
  for (uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * KED_WAVES + (threadIdx.x >> 6))); w < n; w += stride) {
    const uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)wl[w]);
    if (i >= P.m) continue;
    KedLink L;
    if (ked_link(P, i, L) != 0) continue;                        // (settled by k_edits_classify; the same inputs give the same answer here)
    const int hi = min(L.dq, L.dr - d);
    const uint32_t target = (uint32_t)(L.dr - L.dq + 32);        // 1..63: |dq - dr| <= max_edits <= 31
    int F = lane == 32u ? 0 : KED_NEG;
    int res = KED_OVER;
    for (uint32_t e = 0;; ++e) {
      if (F >= 0) F = ked_extend(P, L, F, d, hi);
      if (__ballot(lane == target && F == L.dq)) { res = (int)e; break; }
      if (e == P.max_edits) break;
      int up = __shfl_up(F, 1), dn = __shfl_down(F, 1);
      if (lane == 0u) up = KED_NEG;
      if (lane == 63u) dn = KED_NEG;
      const int c = min(max(up, max(F, dn) + 1), hi);
      F = lane != 0u && c >= 0 && c + d >= 0 ? c : KED_NEG;
    }
    if (lane == 0u) {
      out_link[i] = res;
      if (res > 0) atomicAdd(&c_edits[L.chain], (uint32_t)res);
      if (res == KED_OVER) atomicAdd(&c_over[L.chain], 1u);
    }
  }
}
