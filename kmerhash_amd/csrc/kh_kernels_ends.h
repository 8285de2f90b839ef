// kh_kernels_ends.h -- gfx950 device code of kh_chain_ends, included once by kmerhash_amd.hip after kh_kernels_cigar.h.  Prefix k_ends_.
//
// The two ends of every kept chain -- row 2c the HEAD (the read's bases before the chain's first seed), row 2c + 1 the TAIL (those behind
// its last seed) -- extended from the seed outwards until the read ends or stopping scores better, with the alignment as a run-length row
// of a CSR (definition: include/kmerhash_amd.h, model: tests/ends_model.py).  Base codes, the match rule, the 8-bases-per-step compare
// (ked_extend), the level step with its moves (kcg_level), the traceback into a path word (kcg_traceback), KcgRuns and the replay
// (kcg_walk) are those of kh_kernels_edits.h / _cigar.h.
//   k_ends_wfa    one wavefront per end, fixed grid, grid-stride over the 2 n_chains rows (no worklist: an end of no bases costs a wave a
//                 few loads): the furthest-reaching points with one diagonal per lane (lane l owns d = l - 32), F and the 2-bit moves in
//                 one register each (kcg_level), and per lane the best S = F - clip_cost * e of its own diagonal with the level it
//                 was first seen at.  The levels stop where a diagonal holds |A| (or at max_edits); one butterfly over a packed key then
//                 picks the winner (S, then smaller e, then smaller |d|, then d < 0), kcg_traceback walks the moves back from it with
//                 lane reads into the end's path word, and a forward replay of that path counts the row's runs
//   k_ends_emit   one lane per end with a non-empty row: the replay of the stored path, runs written in forward order for a tail and back
//                 to front for a head -- so that head row, link rows, the last seed and tail row read as one CIGAR
// A differs from a link in that B's end is free (|B| = min(|A| + max_edits, what rtext has left in that direction), every diagonal may be
// the last) and in the four ways the strings run away from the seed: the tail reads A upwards, the head downwards; B runs upwards for
// tail-forward and head-reverse, downwards for tail-reverse and head-forward, complemented on the reverse strand.
// Every index that comes out of memory (c_first, c_last, positions, q_lo, q_hi, path word, offset) is range-checked before it addresses
// anything: ken_end admits a row only where the seed lies inside the read, the read inside qtext and the seed inside rtext; the replay
// re-validates every move against hi(d) and |d| <= 31 before ked_extend reads a byte, and a row never writes more runs than its own offsets
// give it, nor beyond the total the host passes in.
#pragma once
#include "kh_kernels_cigar.h"

// T: the texts and anchors (pred and chain are not used: null); T.n_chains chains, rows 0 .. 2 T.n_chains - 1
struct KenArgs {
  KedArgs T;
  const uint32_t* c_first; const uint32_t* c_last; const uint32_t* q_lo; const uint32_t* q_hi;
  uint32_t clip_cost;
};
// an end that passed the range checks: where its strings start and how they run (STR of ked_extend), dq = |A| (1 .. 2^28 - 1) and
// dr = |B| (0 .. dq + max_edits)
struct KenEnd {
  uint32_t a0, b0, head, down, rev; int dq, dr;
  __device__ __forceinline__ uint32_t a_down() const { return head; }
  __device__ __forceinline__ uint32_t b_down() const { return down; }
  __device__ __forceinline__ uint32_t comp() const { return rev; }
};

// row `row` as kh_chain_ends defines a row that is looked at -> false: an empty row (|A| == 0 included)
__device__ __forceinline__ bool ken_end(const KenArgs& P, uint32_t row, KenEnd& E) {
  const KedArgs& T = P.T;
  const uint32_t c = row >> 1, head = (row & 1u) ^ 1u;
  const uint32_t a = head ? P.c_first[c] : P.c_last[c];
  if (a >= T.m) return false;
  const uint32_t q = T.qpos[a], r = T.rpos[a], rv = T.rev[a] & 1u, lo = P.q_lo[c], hi = P.q_hi[c];
  if ((q | r) >> 31) return false;
  if (hi > T.nq || lo > q || q + T.k > hi) return false;                 // the seed inside the read, the read inside qtext (q + k < 2^32)
  if (r < T.ref_base || (uint64_t)(r - T.ref_base) + T.k > T.nr) return false;      // the seed inside rtext
  const uint32_t rr = r - T.ref_base;
  const uint32_t n = head ? q - lo : hi - (q + T.k);
  if (n == 0u || n >= (uint32_t)KCG_MAXLEN) return false;
  const uint32_t b_down = head ^ rv;                                     // B runs towards rtext[0]: head-forward and tail-reverse
  const uint32_t left = b_down ? rr : T.nr - (rr + T.k);                 // bases of rtext in B's direction
  E.a0 = head ? q : q + T.k; E.b0 = b_down ? rr : rr + T.k; E.head = head; E.down = b_down; E.rev = rv;
  E.dq = (int)n; E.dr = (int)min(n + T.max_edits, left);
  return true;
}

// the winner's key: greater S first, then smaller e, then smaller |d|, then d < 0; 0 = a diagonal that was never reached
__device__ __forceinline__ uint64_t ken_key(int S, uint32_t e, int d) {
  const uint32_t tie = 2u * (uint32_t)(d < 0 ? -d : d) + (d > 0 ? 1u : 0u);         // 0..63
  return ((uint64_t)(uint32_t)(S + (1 << 13)) << 11) | ((uint64_t)(31u - e) << 6) | (63u - tie);      // S >= -255 * 31 > -2^13
}
__device__ __forceinline__ uint64_t ken_wave_max(uint64_t v) {
  for (int m = 1; m < 64; m <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(KED_THREADS) void k_ends_wfa(KenArgs P, uint32_t* __restrict__ e_q, uint32_t* __restrict__ e_r, uint32_t* __restrict__ e_edits,
                                                          uint32_t* __restrict__ e_clip, uint32_t* __restrict__ runs, uint64_t* __restrict__ paths) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KED_WAVES, rows = 2u * P.T.n_chains;
  const int d = (int)lane - 32;
  // lanes 0..4 write one of the row's five numbers each: one store, and the five pointers live in one register pair per lane
  uint32_t* const mine = lane == 0u ? e_q : lane == 1u ? e_r : lane == 2u ? e_edits : lane == 3u ? e_clip : runs;
  for (uint32_t row = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * KED_WAVES + (threadIdx.x >> 6))); row < rows; row += stride) {
    KenEnd E;
    if (!ken_end(P, row, E)) {
      if (lane < 5u) mine[row] = 0u;
      continue;
    }
    const int hi = min(E.dq, E.dr - d);
    int F = lane == 32u ? 0 : KED_NEG;
    uint64_t moves = 0;
    int bestS = KED_NEG; uint32_t bestE = 0;
    for (uint32_t e = 0;; ++e) {
      if (F >= 0) {
        F = ked_extend(P.T, E, F, d, hi);
        const int S = F - (int)(P.clip_cost * e);
        if (S > bestS) { bestS = S; bestE = e; }
      }
      if (__ballot(F == E.dq) || e == P.T.max_edits) break;
      F = kcg_level(F, d, hi, lane, e, moves);
    }
    // the winner: lane 32 was reached at level 0, so the maximum is a real key
    const uint64_t key = ken_wave_max(bestS > KED_NEG ? ken_key(bestS, bestE, d) : 0ull);
    const int we = 31 - (int)((key >> 6) & 31u), tie = 63 - (int)(key & 63u);
    const int wd = (tie & 1) ? (tie >> 1) : -(tie >> 1);
    const int wF = (int)(uint32_t)(key >> 11) - (1 << 13) + (int)P.clip_cost * we;
    // traceback from (we, wd) to (0, 0)
    bool ok = true;
    int dd = wd;
    const uint64_t path = kcg_traceback(moves, we, dd, ok);
    uint32_t n_runs = 0xffffffffu;                               // lane 0 replays the path; all ones: not confirmed
    if (lane == 0u) {
      KcgRuns<false> R{nullptr, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      int v, rd;
      if (ok && dd == 0 && kcg_walk<false>(P.T, E, path, R, v, rd) && v == wF && rd == wd) { paths[row] = path; n_runs = R.n; }
    }
    n_runs = (uint32_t)__shfl((int)n_runs, 0);
    const uint32_t num = lane == 0u ? (uint32_t)wF : lane == 1u ? (uint32_t)(wF + wd) : lane == 2u ? (uint32_t)we : lane == 3u ? (uint32_t)(E.dq - wF) : n_runs;
    if (lane < 5u) mine[row] = n_runs != 0xffffffffu ? num : 0u;  // (not confirmed: the replay of a path this wave has just traced ends where the trace began)
  }
}

__global__ __launch_bounds__(KED_THREADS) void k_ends_emit(KenArgs P, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ paths, uint64_t total,
                                                           uint32_t* __restrict__ out_ops) {
  const uint32_t stride = gridDim.x * KED_THREADS, rows = 2u * P.T.n_chains;
  for (uint32_t row = blockIdx.x * KED_THREADS + threadIdx.x; row < rows; row += stride) {
    const uint64_t o0 = offsets[row], o1 = offsets[row + 1];
    if (o1 <= o0 || o1 > total || o1 - o0 > 63ull) continue;     // an empty row; or offsets that are not this call's
    KenEnd E;
    if (!ken_end(P, row, E)) continue;
    KcgRuns<true> R{out_ops + o0, (uint32_t)(o1 - o0), 0u, 0u, 0u, 0u, 0u, (row & 1u) ^ 1u};      // a head is stored in read order
    int v, d;
    kcg_walk<true>(P.T, E, paths[row], R, v, d);
  }
}
