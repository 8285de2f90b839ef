// kh_kernels_select.h -- gfx950 device code of kh_chain_select, included once by kmerhash_amd.hip after kh_kernels_ends.h.  Prefix k_select_.
//
// Primary / secondary chains per group (one read) and a mapping quality per primary (definition: include/kmerhash_amd.h, model:
// tests/select_model.py).  Integers only.  Two kernels are launched over ALL groups and each skips the groups of the other size class,
// so the host never has to know a group's size:
//   k_select_wave   groups of 0..64 chains: one wavefront per group, one chain per lane, everything in registers.  Rank by counting
//                   (a uniform loop broadcasts (score, lane), every lane counts who beats it), one push permute into rank order, the
//                   greedy sweep with the primaries as a 64-bit scalar mask, ballots for sub / nsub / the kept ordinal.
//   k_select_block  groups of more than 64 chains: one workgroup per group.  Sort by (score descending, index ascending) -- bitonic in
//                   LDS up to KSEL_TILE chains, beyond it a stable LSD radix sort of chain indices over scratch -- then the same sweep
//                   64 ranks at a time: all four waves look for the first covering primary among those of earlier batches (list in LDS,
//                   or in scratch beyond a tile), wave 0 settles the batch with the wave sweep.  Correct for any size, not fast.
// No atomics anywhere.  Group bounds are clamped to [0, n] where they are read and every index that comes out of scratch is clamped
// before it addresses anything: offsets that are no ascending partition give unspecified outputs, but nothing outside the arrays is
// touched (groups that overlap may race on scratch; the clamps are what keeps that harmless).
#pragma once
#include "kh_kernels_chain.h"

#define KSEL_THREADS 256
#define KSEL_WAVES (KSEL_THREADS / 64)
#define KSEL_TILE 2048      // chains of a group that are sorted and swept in LDS
#define KSEL_NONE 0xFFFFFFFFu

struct KselArgs {
  const uint32_t *qs, *qe; const int32_t* score; const uint32_t* count; uint32_t n;
  const uint64_t* off; uint32_t n_grp;
  uint32_t mask_pct, pri_pct, best_n;
  int32_t* parent; uint32_t* rank; uint8_t *mapq, *flag; int32_t* sub; uint32_t* nsub; int32_t* best;
};
// scratch of k_select_block: seven arrays of `stride` >= n words behind one pointer (one pointer and a stride instead of seven pointers
// keep the kernel's scalar registers unspilled) -- the two index buffers of the radix sort, then the primaries of a group in rank
// order: q_start, q_end, chain, nsub, sub
#define KSEL_SCRATCH_ARRAYS 7
struct KselScratch { uint32_t* base; uint32_t stride; };

// group g clamped to [0, n]: a <= b <= n whatever off holds
__device__ __forceinline__ void ksel_group(const KselArgs& P, uint32_t g, uint32_t& a, uint32_t& b) {
  if (!P.off) { a = 0; b = P.n; return; }
  const uint64_t lo = P.off[g], hi = P.off[(uint64_t)g + 1];
  a = lo < P.n ? (uint32_t)lo : P.n;
  b = hi < P.n ? (uint32_t)hi : P.n;
  if (b < a) b = a;
}
// does p cover c?  100 ov(c, p) >= mask_pct min(len_c, len_p), in signed 64-bit
__device__ __forceinline__ bool ksel_covers(uint32_t cs, uint32_t ce, uint32_t ps, uint32_t pe, uint32_t mask_pct) {
  const long long lc = max(0ll, (long long)ce - (long long)cs), lp = max(0ll, (long long)pe - (long long)ps);
  const long long ov = max(0ll, (long long)min(ce, pe) - (long long)max(cs, ps));
  return 100ll * ov >= (long long)mask_pct * min(lc, lp);
}
__device__ __forceinline__ uint32_t ksel_mapq(int s, int sub, uint32_t cnt) {
  if (s <= 0) return 0u;
  const unsigned long long t = 60ull * (unsigned long long)((long long)s - (long long)sub) * (unsigned long long)min(cnt, 10u) * (unsigned long long)min(s, 100);
  const unsigned long long q = t / (1000ull * (unsigned long long)s);
  return q < 60ull ? (uint32_t)q : 60u;
}
// is secondary (score s, `ord` secondaries of its parent before it) of a parent with score sp kept?
__device__ __forceinline__ bool ksel_kept(int s, int sp, uint32_t ord, const KselArgs& P) {
  return 100ll * (long long)s >= (long long)P.pri_pct * (long long)sp && ord < P.best_n;
}
// ascending in this key = descending in the score
__device__ __forceinline__ uint32_t ksel_key(int s) { return ~((uint32_t)s ^ 0x80000000u); }
__device__ __forceinline__ unsigned long long ksel_below(uint32_t lane) { return (1ull << lane) - 1ull; }

// The greedy sweep over the `cnt` chains a wave holds in rank order, lane r = rank r of the batch.  pre: KSEL_NONE, or the chain is
// already covered by a primary of an earlier batch and takes no part.  -> the mask of the lanes that are primary; pl = the lane of the
// covering primary of smallest rank, the lane itself for a primary, KSEL_NONE for a lane with pre.  EXEC must be full.
__device__ __forceinline__ unsigned long long ksel_sweep(uint32_t lane, uint32_t cnt, uint32_t qs, uint32_t qe, uint32_t pre, uint32_t mask_pct, uint32_t& pl) {
  unsigned long long pm = 0;
  pl = KSEL_NONE;
  for (uint32_t r = 0; r < cnt; ++r) {
    if (kch_rl(pre, r) != KSEL_NONE) continue;
    const uint32_t cs = kch_rl(qs, r), ce = kch_rl(qe, r);
    const unsigned long long cov = __ballot(((pm >> lane) & 1ull) && ksel_covers(cs, ce, qs, qe, mask_pct));
    if (cov) {
      if (lane == r) pl = (uint32_t)__ffsll((long long)cov) - 1u;
    } else {
      if (lane == r) pl = r;
      pm |= 1ull << r;
    }
  }
  return pm;
}
// The secondaries of a batch, by parent (ppos: the parent's position among the group's primaries).  For a secondary: ord = the
// secondaries of its parent before it IN THIS BATCH, gcnt = how many the batch holds, gfirst = the score of the first of them.  For a
// primary of this batch: gcnt and gfirst of its own secondaries (gcnt = 0: none).  EXEC must be full.
__device__ __forceinline__ void ksel_subs(uint32_t lane, bool valid, bool prim, uint32_t ppos, int s, uint32_t& ord, uint32_t& gcnt, int& gfirst) {
  unsigned long long todo = __ballot(valid && !prim);
  ord = 0; gcnt = 0; gfirst = 0;
  while (todo) {
    const uint32_t l = (uint32_t)__ffsll((long long)todo) - 1u, pp = kch_rl(ppos, l);      // (l: the first of its parent's secondaries)
    const unsigned long long peers = __ballot(valid && !prim && ppos == pp);
    const uint32_t c = (uint32_t)__popcll(peers);
    const int fs = kch_rl(s, l);
    if ((peers >> lane) & 1ull) { ord = (uint32_t)__popcll(peers & ksel_below(lane)); gcnt = c; gfirst = fs; }
    if (valid && prim && ppos == pp) { gcnt = c; gfirst = fs; }
    todo &= ~peers;
  }
}

__global__ __launch_bounds__(KSEL_THREADS) void k_select_wave(KselArgs P) {
  const uint32_t lane = threadIdx.x & 63, ng = P.off ? P.n_grp : 1u, stride = gridDim.x * KSEL_WAVES;
  for (uint32_t g = kch_first_segment(); g < ng; g += stride) {
    uint32_t a, b;
    ksel_group(P, g, a, b);
    const uint32_t len = b - a;
    if (len > 64u) continue;                                   // k_select_block's
    if (len == 0u) { if (P.best && lane == 0) P.best[g] = -1; continue; }
    const bool valid = lane < len;
    uint32_t qs = 0, qe = 0, cn = 0; int s = 0;
    if (valid) { qs = P.qs[a + lane]; qe = P.qe[a + lane]; s = P.score[a + lane]; cn = P.count[a + lane]; }
    // rank by counting; the lanes beyond the group keep their own number, so that rank is a permutation of the lanes
    uint32_t rk = 0;
    for (uint32_t j = 0; j < len; ++j) {
      const int sj = kch_rl(s, j);
      rk += (sj > s || (sj == s && j < lane)) ? 1u : 0u;
    }
    if (!valid) rk = lane;
    // into rank order: lane rk receives what this lane holds
    const int to = (int)(rk << 2);
    qs = (uint32_t)__builtin_amdgcn_ds_permute(to, (int)qs);
    qe = (uint32_t)__builtin_amdgcn_ds_permute(to, (int)qe);
    cn = (uint32_t)__builtin_amdgcn_ds_permute(to, (int)cn);
    s = __builtin_amdgcn_ds_permute(to, s);
    const uint32_t src = (uint32_t)__builtin_amdgcn_ds_permute(to, (int)lane);
    uint32_t pl;
    const unsigned long long pm = ksel_sweep(lane, len, qs, qe, KSEL_NONE, P.mask_pct, pl);
    const bool prim = valid && pl == lane;
    const uint32_t plc = pl < 64u ? pl : lane;
    uint32_t ord, gcnt; int gfirst;
    ksel_subs(lane, valid, prim, (uint32_t)__popcll(pm & ksel_below(plc)), s, ord, gcnt, gfirst);
    const uint32_t psrc = (uint32_t)__shfl((int)src, (int)plc);
    const int sp = __shfl(s, (int)plc);
    if (valid) {
      const uint32_t i = a + src;
      const int sb = prim && gcnt ? max(0, gfirst) : 0;
      P.parent[i] = (int32_t)(a + psrc);
      P.rank[i] = lane;
      P.mapq[i] = prim ? (uint8_t)ksel_mapq(s, sb, cn) : (uint8_t)0;
      P.flag[i] = prim ? (uint8_t)3 : (ksel_kept(s, sp, ord, P) ? (uint8_t)2 : (uint8_t)0);
      P.sub[i] = sb;
      P.nsub[i] = prim ? gcnt : 0u;
      if (P.best && lane == 0) P.best[g] = (int32_t)i;
    }
  }
}

// the lanes of the wave that hold the same 8-bit digit as this one (valid lanes only; unspecified for the others).  EXEC must be full.
__device__ __forceinline__ unsigned long long ksel_match8(uint32_t d, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (uint32_t bit = 0; bit < 8; ++bit) {
    const bool on = (d >> bit) & 1u;
    const unsigned long long bb = __ballot(on);
    m &= on ? bb : ~bb;
  }
  return m;
}

__global__ __launch_bounds__(KSEL_THREADS) void k_select_block(KselArgs P, KselScratch S) {
  __shared__ unsigned long long keys[KSEL_TILE];              // the bitonic keys, then the tile's chains in rank order (uint32)
  __shared__ uint32_t t_list[5 * KSEL_TILE];                  // the tile's primaries: q_start, q_end, chain, nsub, sub
  __shared__ uint32_t cand[KSEL_WAVES][64];
  __shared__ uint32_t wcnt[KSEL_WAVES][256], bins[256];       // radix: digits per wave of the chunk in hand, running bin starts
  __shared__ uint32_t nprim;
  __shared__ uint8_t isbig[KSEL_THREADS];
  // The seven output pointers wait in LDS and come back as vector registers where a result is stored: held as scalars through the
  // sort and the sweep they were 14 registers too many, and the compiler spilled.
  __shared__ void* outp[7];
  if (threadIdx.x == 0) { outp[0] = P.parent; outp[1] = P.rank; outp[2] = P.mapq; outp[3] = P.flag; outp[4] = P.sub; outp[5] = P.nsub; outp[6] = P.best; }
  __syncthreads();
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ng = P.off ? P.n_grp : 1u, nmax = P.n - 1u;
  // Workgroup x owns the groups x, x + gridDim.x, ...  Its threads look at 256 of them at a time, one each, so that a batch of short
  // reads costs a workgroup one round of loads and not one dependent load per group; the large ones are then taken in turn.
  for (uint32_t base = 0; (uint64_t)blockIdx.x + (uint64_t)base * gridDim.x < ng; base += KSEL_THREADS) {
    {
      const uint64_t gm = (uint64_t)blockIdx.x + (uint64_t)(base + tid) * gridDim.x;
      bool big = false;
      if (gm < ng) { uint32_t a0, b0; ksel_group(P, (uint32_t)gm, a0, b0); big = b0 - a0 > 64u; }
      __syncthreads();                                         // (the round before is done with the flags)
      isbig[tid] = big ? 1 : 0;
      __syncthreads();
    }
    for (uint32_t j = 0; j < KSEL_THREADS; ++j) {
      if (!isbig[j]) continue;                                   // k_select_wave's, or past the last group
      const uint32_t g = blockIdx.x + (base + j) * gridDim.x;
      uint32_t a, b;
      ksel_group(P, g, a, b);
      const uint32_t len = b - a;
      __syncthreads();                                           // (the group before is done with the LDS)
      const uint32_t* order;
      uint32_t* L; uint32_t ls;                                  // the primaries' list: field f of entry p is L[f * ls + p]
      if (len <= KSEL_TILE) {
        // ---- bitonic sort of (key << 32 | index in the group), padded with all-ones to a power of two
        uint32_t n2 = 128;
        while (n2 < len) n2 <<= 1;
        for (uint32_t i = tid; i < n2; i += KSEL_THREADS)
          keys[i] = i < len ? ((unsigned long long)ksel_key(P.score[a + i]) << 32) | i : ~0ull;
        __syncthreads();
        for (uint32_t k2 = 2; k2 <= n2; k2 <<= 1)
          for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < n2; i += KSEL_THREADS) {
              const uint32_t o = i ^ j;
              if (o > i) {
                const unsigned long long x = keys[i], y = keys[o];
                if ((x > y) == ((i & k2) == 0u)) { keys[i] = y; keys[o] = x; }
              }
            }
            __syncthreads();
          }
        // the keys become chain indices in place: every key is in a register before the first index is written
        uint32_t mine[KSEL_TILE / KSEL_THREADS];
  #pragma unroll
        for (uint32_t t = 0; t < KSEL_TILE / KSEL_THREADS; ++t) { const uint32_t i = tid + t * KSEL_THREADS; mine[t] = i < len ? a + (uint32_t)keys[i] : 0u; }
        __syncthreads();
        uint32_t* o32 = reinterpret_cast<uint32_t*>(keys);
  #pragma unroll
        for (uint32_t t = 0; t < KSEL_TILE / KSEL_THREADS; ++t) { const uint32_t i = tid + t * KSEL_THREADS; if (i < len) o32[i] = mine[t]; }
        order = o32;
        L = t_list; ls = KSEL_TILE;
      } else {
        // ---- stable LSD radix sort of the chain indices by the 32-bit key, 8 bits a pass: identity -> a -> b -> a -> b
        for (uint32_t pass = 0; pass < 4; ++pass) {
          const uint32_t* src = pass == 0 ? nullptr : S.base + ((pass & 1u) ? 0u : S.stride) + a;
          uint32_t* dst = S.base + ((pass & 1u) ? S.stride : 0u) + a;
          const uint32_t shift = pass * 8;
  #pragma unroll
          for (uint32_t w = 0; w < KSEL_WAVES; ++w) wcnt[w][tid] = 0;
          __syncthreads();
          for (uint32_t c0 = 0; c0 < len; c0 += KSEL_THREADS) {  // histogram: a row of counters per wave, one writer per digit
            const uint32_t i = c0 + tid;
            const bool v = i < len;
            const uint32_t idx = v ? (src ? min(src[i], nmax) : a + i) : 0u;
            const uint32_t d = v ? (ksel_key(P.score[idx]) >> shift) & 255u : 0u;
            const unsigned long long peers = ksel_match8(d, v);
            if (v && (peers & ksel_below(lane)) == 0ull) wcnt[wave][d] += (uint32_t)__popcll(peers);
          }
          __syncthreads();
          uint32_t tot = 0;
  #pragma unroll
          for (uint32_t w = 0; w < KSEL_WAVES; ++w) { tot += wcnt[w][tid]; wcnt[w][tid] = 0; }
          bins[tid] = tot;
          __syncthreads();
          if (tid == 0) { uint32_t run = 0; for (uint32_t d = 0; d < 256; ++d) { const uint32_t t = bins[d]; bins[d] = run; run += t; } }
          __syncthreads();
          for (uint32_t c0 = 0; c0 < len; c0 += KSEL_THREADS) {  // scatter, 256 entries at a time in their order
            const uint32_t i = c0 + tid;
            const bool v = i < len;
            const uint32_t idx = v ? (src ? min(src[i], nmax) : a + i) : 0u;
            const uint32_t d = v ? (ksel_key(P.score[idx]) >> shift) & 255u : 0u;
            const unsigned long long peers = ksel_match8(d, v);
            const uint32_t before = (uint32_t)__popcll(peers & ksel_below(lane));
            if (v && before == 0u) wcnt[wave][d] = (uint32_t)__popcll(peers);
            __syncthreads();
            if (v) {
              uint32_t pos = bins[d] + before;
              for (uint32_t w = 0; w < wave; ++w) pos += wcnt[w][d];
              if (pos < len) dst[pos] = idx;                     // (always, unless groups overlap)
            }
            __syncthreads();
            uint32_t add = 0;
  #pragma unroll
            for (uint32_t w = 0; w < KSEL_WAVES; ++w) { add += wcnt[w][tid]; wcnt[w][tid] = 0; }
            bins[tid] += add;
            __syncthreads();
          }
        }
        order = S.base + S.stride + a;
        L = S.base + 2u * S.stride + a; ls = S.stride;
      }
      if (tid == 0) nprim = 0;
      __syncthreads();
      // ---- the sweep, 64 ranks at a time
      for (uint32_t b0 = 0; b0 < len; b0 += 64) {
        const uint32_t np = nprim, cnt = len - b0 < 64u ? len - b0 : 64u;
        const bool valid = lane < cnt;
        const uint32_t idx = valid ? min(order[b0 + lane], nmax) : 0u;
        uint32_t qs = 0, qe = 0;
        if (valid) { qs = P.qs[idx]; qe = P.qe[idx]; }
        // the first primary of an earlier batch that covers this chain: every wave takes every fourth of them
        uint32_t c = KSEL_NONE;
        if (valid)
          for (uint32_t p = wave; p < np; p += KSEL_WAVES)
            if (ksel_covers(qs, qe, L[p], L[ls + p], P.mask_pct)) { c = p; break; }
        cand[wave][lane] = c;
        __syncthreads();
        if (wave == 0) {
          uint32_t pre = min(min(cand[0][lane], cand[1][lane]), min(cand[2][lane], cand[3][lane]));
          if (!valid) pre = KSEL_NONE;
          const int s = valid ? P.score[idx] : 0;
          uint32_t pl;
          const unsigned long long pm = ksel_sweep(lane, cnt, qs, qe, pre, P.mask_pct, pl);
          const bool prim = valid && pl == lane;
          const uint32_t plc = pl < 64u ? pl : lane;
          const uint32_t ppos = pre != KSEL_NONE ? pre : np + (uint32_t)__popcll(pm & ksel_below(plc));
          uint32_t ord, gcnt; int gfirst;
          ksel_subs(lane, valid, prim, ppos, s, ord, gcnt, gfirst);
          uint32_t pidx = (uint32_t)__shfl((int)idx, (int)plc);
          int sp = __shfl(s, (int)plc);
          uint32_t base = 0;
          if (pre != KSEL_NONE) { pidx = min(L[2u * ls + pre], nmax); sp = P.score[pidx]; base = L[3u * ls + pre]; }
          if (valid) {
            int32_t* o_parent = static_cast<int32_t*>(outp[0]);
            uint8_t *o_mapq = static_cast<uint8_t*>(outp[2]), *o_flag = static_cast<uint8_t*>(outp[3]);
            static_cast<uint32_t*>(outp[1])[idx] = b0 + lane;
            if (prim) {
              L[ppos] = qs; L[ls + ppos] = qe; L[2u * ls + ppos] = idx; L[3u * ls + ppos] = gcnt; L[4u * ls + ppos] = (uint32_t)(gcnt ? max(0, gfirst) : 0);
              o_parent[idx] = (int32_t)idx;
              o_flag[idx] = (uint8_t)3;                          // (mapq, sub and nsub: when the group's last batch is through)
            } else {
              o_parent[idx] = (int32_t)pidx;
              o_mapq[idx] = (uint8_t)0;
              o_flag[idx] = ksel_kept(s, sp, base + ord, P) ? (uint8_t)2 : (uint8_t)0;
              static_cast<int32_t*>(outp[4])[idx] = 0;
              static_cast<uint32_t*>(outp[5])[idx] = 0u;
              if (pre != KSEL_NONE && ord == 0u) {               // the first of them in this batch brings the parent's entry up to date
                L[3u * ls + pre] = base + gcnt;
                if (base == 0u) L[4u * ls + pre] = (uint32_t)max(0, s);
              }
            }
          }
          if (lane == 0) nprim = np + (uint32_t)__popcll(pm);
        }
        __syncthreads();
      }
      const uint32_t np = nprim;
      for (uint32_t i = tid; i < np; i += KSEL_THREADS) {
        const uint32_t idx = min(L[2u * ls + i], nmax);
        const int sb = (int)L[4u * ls + i];
        static_cast<uint8_t*>(outp[2])[idx] = (uint8_t)ksel_mapq(P.score[idx], sb, P.count[idx]);
        static_cast<int32_t*>(outp[4])[idx] = sb;
        static_cast<uint32_t*>(outp[5])[idx] = L[3u * ls + i];
      }
      if (tid == 0 && outp[6]) static_cast<int32_t*>(outp[6])[g] = (int32_t)min(order[0], nmax);
    }
  }
}
