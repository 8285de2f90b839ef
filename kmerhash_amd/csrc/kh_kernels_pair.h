// kh_kernels_pair.h -- gfx950 device code of kh_pair_chains, included once by kmerhash_amd.hip after kh_kernels_sam.h.  Prefix k_pair_.
//
// The concordant chain pair of every read pair (definition: include/kmerhash_amd.h, model: tests/pair_model.py).  Integers only.  One
// kernel, one wavefront per pair, everything in registers: no LDS, no scratch, no atomics, and no second size class.
//   select   the up to KPR_CAP candidates of a mate.  A group of at most 64 chains is one load: lane i holds chain i of the group, which
//            is chain order already.  A longer group is streamed 64 chains at a time under the key (score, ~chain): the chunk is ranked
//            by counting (the uniform broadcast loop of k_select_wave) and pushed into descending order, read back to front, and the
//            lane-wise larger of (the 64 best so far, descending) and (the chunk, ascending) is the 64 best of the 128 -- the first half
//            of a bitonic merge; one more count and push puts them into order again.  Two loops of 64 steps per chunk, O(size) for a
//            group of any size.  At the end one count and push by chain number: lane order is chain order for both mates, with gaps
//            where a lane holds no candidate.
//   combine  lane i holds a candidate a of mate 1; a uniform loop broadcasts the candidates b of mate 2 in chain order.  Every lane keeps
//            its greatest pair score, the first b that reaches it, the greatest over every other b, and its count.  (a*, b*) is then ONE
//            wave max over the packed key (ps + 2^32 + 1) << 12 | (63 - lane of a) << 6 | (63 - lane of b), 0 where a lane has no
//            combination; alt1 the max of the lanes' best scores but for the lane of a*, alt2 the max of "best, or the runner-up where
//            the best's b is b*", the count a wave sum.  Lane 0 writes mate 1 and the pair, lane 1 mate 2, with vector stores.
// Group bounds are clamped to [0, n] where they are read (ksel_group's rule) and every chain number the wave holds came from such a
// group: offsets that do not ascend give unspecified outputs for those pairs, and nothing outside the arrays is touched.
#pragma once
#include "kh_kernels_select.h"

#define KPR_THREADS 256
#define KPR_WAVES (KPR_THREADS / 64)
#define KPR_CAP 64u          // candidates per mate: part of the definition (KH_PAIR_CANDIDATES)
#define KPR_NONE 0xFFFFFFFFu // KH_TARGET_NONE
#define KPR_BIAS 0x100000001ull      // ps + KPR_BIAS is 1..2^33 - 1: 0 stays free for "no combination"

struct KprArgs {
  const uint32_t *rs, *re; const uint8_t* rev; const int32_t* score; const uint32_t* tid; const uint8_t *use, *mapq_in; uint32_t n;
  const uint64_t* off; uint32_t n_pairs;
  uint32_t min_ins, max_ins, pen;
  int32_t* row; uint8_t* mapq; int32_t* tlen; uint8_t* flag; int32_t* score_out; uint32_t* nconc;
};

__device__ __forceinline__ unsigned long long kpr_rl64(unsigned long long v, uint32_t l) {
  return ((unsigned long long)kch_rl((uint32_t)(v >> 32), l) << 32) | (unsigned long long)kch_rl((uint32_t)v, l);
}
// max / sum over the wave in every lane's return value (a butterfly of six exchanges).  EXEC must be full.
__device__ __forceinline__ unsigned long long kpr_wave_max(unsigned long long v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d) << 32) | (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)v, d);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t kpr_wave_sum(uint32_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d);
  return v;
}
// The 64 keys of a wave into descending order: lane r receives the key of rank r.  Equal keys (the zeroes of empty lanes) rank by lane,
// so the ranks are a permutation of the lanes and the push has one writer per lane.  EXEC must be full.
__device__ __forceinline__ unsigned long long kpr_sort_desc(unsigned long long k, uint32_t lane) {
  uint32_t rk = 0;
  for (uint32_t j = 0; j < 64; ++j) {
    const unsigned long long kj = kpr_rl64(k, j);
    rk += (kj > k || (kj == k && j < lane)) ? 1u : 0u;
  }
  const int to = (int)(rk << 2);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_permute(to, (int)(uint32_t)(k >> 32));
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_permute(to, (int)(uint32_t)k);
  return ((unsigned long long)hi << 32) | lo;
}
// The candidates of group [a, b) (a <= b <= P.n), one per lane in chain order, gaps allowed: -> has this lane one; idx its chain, s its
// score.  EXEC must be full.
__device__ __forceinline__ bool kpr_select(const KprArgs& P, uint32_t a, uint32_t b, uint32_t lane, uint32_t& idx, int& s) {
  unsigned long long K = 0;      // (score ^ 2^31) << 32 | ~chain: greater is better; 0 = no candidate (~chain >= 2^32 - 2^23 > 0)
  for (uint32_t c0 = a; c0 < b; c0 += 64) {
    const uint32_t i = c0 + lane;
    unsigned long long N = 0;
    if (i < b && (!P.use || P.use[i]) && P.re[i] > P.rs[i]) N = ((unsigned long long)((uint32_t)P.score[i] ^ 0x80000000u) << 32) | (unsigned long long)(~i);
    if (b - a <= 64u) { K = N; break; }      // one load: chain order as it stands
    if (__ballot(N != 0ull) == 0ull) continue;
    N = kpr_sort_desc(N, lane);
    const int from = (int)((63u - lane) << 2);
    const unsigned long long R = ((unsigned long long)(uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)(uint32_t)(N >> 32)) << 32) |
                                 (unsigned long long)(uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)(uint32_t)N);
    K = kpr_sort_desc(R > K ? R : K, lane);
  }
  if (b - a > 64u) {      // into chain order: (~chain, score) descending = chain ascending, the empty lanes last
    K = kpr_sort_desc((K << 32) | (K >> 32), lane);
    K = (K << 32) | (K >> 32);
  }
  idx = ~(uint32_t)K;
  s = (int)((uint32_t)(K >> 32) ^ 0x80000000u);
  return K != 0ull;
}
// group g of the CSR clamped to [0, n]: a <= b <= n whatever off holds
__device__ __forceinline__ void kpr_group(const KprArgs& P, uint32_t g, uint32_t& a, uint32_t& b) {
  const uint64_t lo = P.off[g], hi = P.off[(uint64_t)g + 1];
  a = lo < P.n ? (uint32_t)lo : P.n;
  b = hi < P.n ? (uint32_t)hi : P.n;
  if (b < a) b = a;
}
__device__ __forceinline__ uint32_t kpr_quality(long long ps, unsigned long long alt_biased) {
  if (ps <= 0) return 0u;
  long long alt = alt_biased ? (long long)alt_biased - (long long)KPR_BIAS : 0ll;
  if (alt < 0) alt = 0;      // (alt <= ps: ps is the greatest)
  const unsigned long long q = 60ull * (unsigned long long)(ps - alt) / (unsigned long long)ps;
  return q < 60ull ? (uint32_t)q : 60u;
}

__global__ __launch_bounds__(KPR_THREADS) void k_pair_wave(KprArgs P) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KPR_WAVES;
  for (uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * KPR_WAVES + (threadIdx.x >> 6))); p < P.n_pairs; p += stride) {
    uint32_t a0, a1, b0, b1;
    kpr_group(P, 2u * p, a0, a1);
    kpr_group(P, 2u * p + 1u, b0, b1);
    uint32_t ai, bi; int as, bs;
    const bool av = kpr_select(P, a0, a1, lane, ai, as), bv = kpr_select(P, b0, b1, lane, bi, bs);
    uint32_t ars = 0, are = 0, arv = 0, atd = 0, brs = 0, bre = 0, brv = 0, btd = 0;
    if (av) { ars = P.rs[ai]; are = P.re[ai]; arv = P.rev[ai] & 1u; atd = P.tid ? P.tid[ai] : 0u; }
    if (bv) { brs = P.rs[bi]; bre = P.re[bi]; brv = P.rev[bi] & 1u; btd = P.tid ? P.tid[bi] : 0u; }
    // the singles: the greatest (score, ~chain) of each mate
    const unsigned long long ka = kpr_wave_max(av ? ((unsigned long long)((uint32_t)as ^ 0x80000000u) << 32) | (unsigned long long)(~ai) : 0ull);
    const unsigned long long kb = kpr_wave_max(bv ? ((unsigned long long)((uint32_t)bs ^ 0x80000000u) << 32) | (unsigned long long)(~bi) : 0ull);
    // combine: this lane's a against every b, in chain order
    unsigned long long best = 0, second = 0;      // biased pair scores, 0 = none
    uint32_t best_b = 0, cnt = 0;
    for (unsigned long long todo = __ballot(bv); todo; todo &= todo - 1ull) {
      const uint32_t j = (uint32_t)__ffsll((long long)todo) - 1u;
      const uint32_t jrs = kch_rl(brs, j), jre = kch_rl(bre, j), jrv = kch_rl(brv, j), jtd = kch_rl(btd, j);
      const int js = kch_rl(bs, j);
      const uint32_t frs = arv ? jrs : ars, fre = arv ? jre : are, rrs = arv ? ars : jrs, rre = arv ? are : jre;      // forward, reverse
      const uint32_t frag = rre - frs;
      const bool ok = av && atd == jtd && atd != KPR_NONE && arv != jrv && frs <= rrs && fre <= rre && frag >= P.min_ins && frag <= P.max_ins;
      const unsigned long long ps = (unsigned long long)((long long)as + (long long)js + (long long)KPR_BIAS);
      if (ok) {
        ++cnt;
        if (ps > best) { second = best; best = ps; best_b = j; }
        else if (ps > second) second = ps;
      }
    }
    const unsigned long long top = kpr_wave_max(cnt ? (best << 12) | (unsigned long long)((63u - lane) << 6) | (unsigned long long)(63u - best_b) : 0ull);
    const uint32_t la = 63u - (uint32_t)((top >> 6) & 63ull), lb = 63u - (uint32_t)(top & 63ull);
    const unsigned long long alt1 = kpr_wave_max(cnt && lane != la ? best : 0ull);
    const unsigned long long alt2 = kpr_wave_max(cnt ? (best_b == lb ? second : best) : 0ull);
    const uint32_t total = kpr_wave_sum(cnt);
    const uint32_t star_a = (uint32_t)__shfl((int)ai, (int)la), star_b = (uint32_t)__shfl((int)bi, (int)lb);
    if (lane < 2u) {
      const bool exists = top != 0ull;
      const long long ps = exists ? (long long)(top >> 12) - (long long)KPR_BIAS : 0ll;
      const int r0a = ka ? (int)~(uint32_t)ka : -1, r0b = kb ? (int)~(uint32_t)kb : -1;
      const long long singles = (ka ? (long long)(int)((uint32_t)(ka >> 32) ^ 0x80000000u) : 0ll) + (kb ? (long long)(int)((uint32_t)(kb >> 32) ^ 0x80000000u) : 0ll);
      const bool proper = exists && ps + (long long)P.pen >= singles;
      const int r1 = proper ? (int)star_a : r0a, r2 = proper ? (int)star_b : r0b;
      const int mine = lane ? r2 : r1, other = lane ? r1 : r2;
      const bool both = r1 >= 0 && r2 >= 0;
      uint32_t mq = 0, m_rs = 0, m_re = 0, m_td = 0, o_rs = 0, o_re = 0, o_td = 0;
      if (mine >= 0) { mq = P.mapq_in ? P.mapq_in[mine] : 0u; m_rs = P.rs[mine]; m_re = P.re[mine]; m_td = P.tid ? P.tid[mine] : 0u; }
      if (other >= 0) { o_rs = P.rs[other]; o_re = P.re[other]; o_td = P.tid ? P.tid[other] : 0u; }
      if (proper) mq = max(mq, kpr_quality(ps, lane ? alt2 : alt1));
      const bool share = both && m_td == o_td && m_td != KPR_NONE;
      int tl = 0;
      if (share) {
        const long long t = min((long long)max(m_re, o_re) - (long long)min(m_rs, o_rs), 0x7FFFFFFFll);
        const bool plus = lane ? m_rs < o_rs : m_rs <= o_rs;      // equal starts: mate 1 takes the plus
        tl = plus ? (int)t : -(int)t;
      }
      const uint64_t r = 2ull * p + lane;
      P.row[r] = mine;
      P.mapq[r] = (uint8_t)mq;
      P.tlen[r] = tl;
      if (lane == 0u) {
        P.flag[p] = (uint8_t)((proper ? 1u : 0u) | (both ? 2u : 0u) | (share ? 4u : 0u));
        P.score_out[p] = exists ? (int32_t)max(min(ps, 0x7FFFFFFFll), -0x80000000ll) : 0;
        P.nconc[p] = total;
      }
    }
  }
}
