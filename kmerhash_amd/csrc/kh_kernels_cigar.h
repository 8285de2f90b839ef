// kh_kernels_cigar.h -- gfx950 device code of kh_chain_cigars, included once by kmerhash_amd.hip after kh_kernels_edits.h.  Prefix k_cigar_.
//
// The alignment operations of every link of every kept chain as run-length rows of a CSR (definition: include/kmerhash_amd.h, model:
// tests/cigar_model.py).  Links, strings, orientation, base codes and the 8-bases-per-step compare are those of kh_kernels_edits.h
// (KedArgs with max_edits = 31, ked_link, ked_extend); link[i] is the distance kh_chain_edits found and bounds the search here.
//   k_cigar_classify  one lane per anchor: 0 runs for a row that is empty by the range checks, 1 run for link == 0 with dq == dr (no
//                     text is read); the rest goes onto a worklist of anchor indices, one reservation per wave (ked_wave_reserve)
//   k_cigar_wfa       one wavefront per worklist entry, fixed grid, grid-stride over the device-side count: the furthest-reaching points
//                     with one diagonal per lane (lane l owns d = l - 32), and per lane the MOVE of its diagonal at every level as 2 bits
//                     of one 64-bit register (31 levels: 62 bits) -- no LDS, no history of F (kcg_level).  At the level that reaches the
//                     target the traceback (kcg_traceback) walks the moves backwards with lane reads and packs them, level t at bits
//                     2(t - 1), into the link's path word; a forward replay of that path (ked_extend on one diagonal per level) counts the
//                     row's runs and its I and D bases
//   k_cigar_emit      one lane per anchor with a non-empty row: the single run of a link == 0 row, or the replay of the stored path, runs
//                     written in forward order; the recurrence does not run again
// Moves: 1 = X (from F[d] + 1), 2 = I (from F[d + 1] + 1: a base of A), 3 = D (from F[d - 1]: a base of B), 0 = no level -- so the number
// of levels of a path is the number of its leading non-zero fields and no distance is stored beside it.  A candidate that leaves
// [.., hi(d)] or has v + d < 0 is dropped, not clamped (k_edits_wfa clamps: it needs no traceback); ties go to X, then I, then D.
// Every index that comes out of memory (pred, chain, link, worklist entry, path word, offset) is range-checked before it addresses
// anything: the replay re-validates every move of a path word against hi(d) and |d| <= 31 before ked_extend reads a byte, and a row never
// writes more runs than its own offsets give it, nor beyond the total the host passes in.
#pragma once
#include "kh_kernels_edits.h"

#define KCG_I 1u      // BAM operation codes
#define KCG_D 2u
#define KCG_EQ 7u
#define KCG_X 8u
#define KCG_MAXLEN (1 << 28)      // run lengths must fit (len << 4)

// the link of anchor i as kh_chain_cigars defines a non-empty row: ked_link's conditions (P.max_edits is 31), 0 <= link[i] <= 31 and both
// strings shorter than 2^28.  -> link[i], or -1 for an empty row
__device__ __forceinline__ int kcg_link(const KedArgs& P, const int32_t* __restrict__ link, uint32_t i, KedLink& L) {
  if (ked_link(P, i, L) != 0) return -1;
  const int e = link[i];
  if (e < 0 || e > 31 || L.dq >= KCG_MAXLEN || L.dr >= KCG_MAXLEN) return -1;
  return e;
}

// the runs of a row, built in forward order: equal neighbours merge, zero lengths vanish; with EMIT run r goes to out[r] while r < cap
// -- with `back` to out[cap - 1 - r]: a row that was found from its far end (the head of a chain, kh_kernels_ends.h)
template <bool EMIT>
struct KcgRuns {
  uint32_t* out; uint32_t cap, n, op, len, ins, del, back;
  __device__ __forceinline__ void flush() {
    if (len) { if (EMIT && n < cap) out[back ? cap - 1u - n : n] = (len << 4) | op; ++n; }
  }
  __device__ __forceinline__ void add(uint32_t o, uint32_t l) {
    if (!l) return;
    if (o == op) { len += l; return; }
    flush();
    op = o; len = l;
  }
};
// forward replay of a path word along one diagonal per level, over the strings L (a KedLink, or the KenEnd of kh_kernels_ends.h: a STR of
// ked_extend with dq = |A| and dr = |B|) -> the point (v_end, d_end) it ends in, or false where a move leaves the strings or the word has
// a 32nd level
template <bool EMIT, typename STR>
__device__ __forceinline__ bool kcg_walk(const KedArgs& P, const STR& L, uint64_t path, KcgRuns<EMIT>& R, int& v_end, int& d_end) {
  int d = 0, v = ked_extend(P, L, 0, 0, min(L.dq, L.dr));
  R.add(KCG_EQ, (uint32_t)v);
  for (uint32_t t = 0; t < 31u; ++t, path >>= 2) {
    const uint32_t mv = (uint32_t)path & 3u;
    if (!mv) break;
    if (mv == 1u) { ++v; R.add(KCG_X, 1u); }
    else if (mv == 2u) { ++v; --d; R.add(KCG_I, 1u); ++R.ins; }
    else { ++d; R.add(KCG_D, 1u); ++R.del; }
    const int hi = min(L.dq, L.dr - d);
    if (d < -31 || d > 31 || v > hi || v + d < 0) return false;      // (no valid move leads here: a path word that was not written by k_cigar_wfa)
    const int w = ked_extend(P, L, v, d, hi);
    R.add(KCG_EQ, (uint32_t)(w - v));
    v = w;
  }
  R.flush();
  v_end = v; d_end = d;
  return (path & 3u) == 0;
}
// the replay of a link's path -> false if it does not end in (|A|, |B|): nothing it says is used then
template <bool EMIT>
__device__ __forceinline__ bool kcg_replay(const KedArgs& P, const KedLink& L, uint64_t path, KcgRuns<EMIT>& R) {
  int v, d;
  return kcg_walk<EMIT>(P, L, path, R, v, d) && v == L.dq && d == L.dr - L.dq;
}
// one level of the furthest-reaching points with moves, by whole waves: lane `lane` holds F of diagonal d = lane - 32 at level `level`
// -> its F at level + 1 before the extension, from the neighbours by lane shuffles; a candidate outside [-d, hi] is dropped, ties go to
// X, then I, then D, and the move goes into bits 2 level of `moves`
__device__ __forceinline__ int kcg_level(int F, int d, int hi, uint32_t lane, uint32_t level, uint64_t& moves) {
  int up = __shfl_up(F, 1), dn = __shfl_down(F, 1);
  if (lane == 0u) up = KED_NEG;
  if (lane == 63u) dn = KED_NEG;
  const int lo = -d;                                         // v + d >= 0
  const int x = F >= 0 && F + 1 <= hi && F + 1 >= lo ? F + 1 : KED_NEG;
  const int a = dn >= 0 && dn + 1 <= hi && dn + 1 >= lo ? dn + 1 : KED_NEG;
  const int b = up >= 0 && up <= hi && up >= lo ? up : KED_NEG;
  int best = x; uint32_t mv = 1u;
  if (a > best) { best = a; mv = 2u; }
  if (b > best) { best = b; mv = 3u; }
  if (lane == 0u || best < 0) { best = KED_NEG; mv = 0u; }   // (lane 0 is d = -32: stays empty)
  moves |= (uint64_t)mv << (2u * level);                     // level + 1 at bits 2 level
  return best;
}
// the walk back through the moves from diagonal dd at level `level` to level 0, one lane read per level, by whole waves -> the path
// word; dd: the diagonal the walk ends on (0: it began at the origin); ok (false on entry: no walk) stays true while every level has a
// move and dd + 32 stays a lane of this wave
__device__ __forceinline__ uint64_t kcg_traceback(uint64_t moves, int level, int& dd, bool& ok) {
  uint64_t path = 0;
  for (int t = level; ok && t >= 1; --t) {
    const uint32_t lo32 = (uint32_t)__shfl((int)(uint32_t)moves, dd + 32), hi32 = (uint32_t)__shfl((int)(uint32_t)(moves >> 32), dd + 32);
    const uint64_t mv = ((((uint64_t)hi32 << 32) | lo32) >> (2 * (t - 1))) & 3ull;
    path |= mv << (2 * (t - 1));
    dd += mv == 2ull ? 1 : mv == 3ull ? -1 : 0;
    ok = mv != 0ull && dd >= -31 && dd <= 31;
  }
  return path;
}

__global__ __launch_bounds__(KED_THREADS) void k_cigar_classify(KedArgs P, const int32_t* __restrict__ link, uint32_t* __restrict__ runs, uint32_t* __restrict__ wl,
                                                                uint32_t* __restrict__ wl_count) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KED_THREADS;
  for (uint32_t i0 = blockIdx.x * KED_THREADS + (threadIdx.x & ~63u); i0 < P.m; i0 += stride) {      // (i0 is the same in a whole wave)
    const uint32_t i = i0 + lane;
    bool queue = false;
    if (i < P.m) {
      KedLink L;
      const int e = kcg_link(P, link, i, L);
      queue = e > 0;
      runs[i] = e == 0 && L.dq == L.dr ? 1u : 0u;      // (a queued row: until k_cigar_wfa has settled it)
    }
    ked_wave_reserve(queue, lane, i, wl, wl_count);
  }
}

__global__ __launch_bounds__(KED_THREADS) void k_cigar_wfa(KedArgs P, const int32_t* __restrict__ link, const uint32_t* __restrict__ wl, const uint32_t* __restrict__ wl_count,
                                                           uint32_t* __restrict__ runs, uint64_t* __restrict__ paths, uint32_t* __restrict__ c_ins, uint32_t* __restrict__ c_del) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KED_WAVES;
  const uint32_t n = min(*wl_count, P.m);
  const int d = (int)lane - 32;
  for (uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * KED_WAVES + (threadIdx.x >> 6))); w < n; w += stride) {
    const uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)wl[w]);
    if (i >= P.m) continue;
    KedLink L;
    const int bound = kcg_link(P, link, i, L);
    if (bound < 1) continue;                                     // (settled by k_cigar_classify; the same inputs give the same answer here)
    const int hi = min(L.dq, L.dr - d);
    const int td = L.dr - L.dq;                                  // the target diagonal, -31..31
    int F = lane == 32u ? 0 : KED_NEG;
    uint64_t moves = 0;
    int found = -1;
    for (int e = 0;; ++e) {
      if (F >= 0) F = ked_extend(P, L, F, d, hi);
      if (__ballot(d == td && F == L.dq)) { found = e; break; }
      if (e == bound) break;
      F = kcg_level(F, d, hi, lane, (uint32_t)e, moves);
    }
    // traceback from (found, td) to (0, 0)
    bool ok = found >= 0;
    int dd = td;
    const uint64_t path = kcg_traceback(moves, found, dd, ok);
    if (lane == 0u) {
      KcgRuns<false> R{nullptr, 0u, 0u, 0u, 0u, 0u, 0u};
      if (ok && dd == 0 && kcg_replay<false>(P, L, path, R)) {
        paths[i] = path;
        runs[i] = R.n;
        if (R.ins) atomicAdd(&c_ins[L.chain], R.ins);
        if (R.del) atomicAdd(&c_del[L.chain], R.del);
      }
    }
  }
}

__global__ __launch_bounds__(KED_THREADS) void k_cigar_emit(KedArgs P, const int32_t* __restrict__ link, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ paths,
                                                            uint64_t total, uint32_t* __restrict__ out_ops) {
  const uint32_t stride = gridDim.x * KED_THREADS;
  for (uint32_t i = blockIdx.x * KED_THREADS + threadIdx.x; i < P.m; i += stride) {
    const uint64_t o0 = offsets[i], o1 = offsets[i + 1];
    if (o1 <= o0 || o1 > total || o1 - o0 > 63ull) continue;     // an empty row; or offsets that are not this call's
    KedLink L;
    const int e = kcg_link(P, link, i, L);
    if (e < 0) continue;
    if (e == 0) {
      if (L.dq == L.dr) out_ops[o0] = ((uint32_t)L.dq << 4) | KCG_EQ;
      continue;
    }
    KcgRuns<true> R{out_ops + o0, (uint32_t)(o1 - o0), 0u, 0u, 0u, 0u, 0u};
    kcg_replay<true>(P, L, paths[i], R);
  }
}
