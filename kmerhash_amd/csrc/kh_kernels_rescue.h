// kh_kernels_rescue.h -- gfx950 device code of kh_mate_rescue, included once by kmerhash_amd.hip after kh_kernels_pair.h.  Prefix k_rescue_.
//
// A mate without a chain row, aligned end to end inside the window its partner allows (definition: include/kmerhash_amd.h, model:
// tests/rescue_model.py).  There is no seed, so the first phase is not a furthest-reaching-point pass: it is a bit-parallel scan of
// the whole window, which says where the mate ends and at what distance; from that end the second phase is the extension of a chain's
// HEAD without a clip cost, so that it never stops early: the strings of kh_kernels_ends.h (KenEnd), its winner's key and wave maximum
// (ken_key, ken_wave_max), and the compare, level step, traceback and replay of kh_kernels_edits.h / _cigar.h (ked_extend, kcg_level,
// kcg_traceback, kcg_walk).  The device functions are shared; no kernel of those files is touched.
//   k_rescue_scan<NW>  one LANE per request, the scan serial in the column (Myers' bit-vector recurrence in Hyyro's block form, the
//                      horizontal delta carried from word to word; word 0 takes 0: the reference start is free).  The pattern R lives
//                      in three bit planes of NW 64-bit words -- low code bit, high code bit, is a base -- packed once from qtext, so
//                      the equality word of a reference base is valid & ~((low ^ b0) | (high ^ b1)): no table per symbol.  Vertical
//                      deltas VP / VN: NW words each.  All of it sits in registers: no LDS, no scratch, no atomics.  The reference is
//                      read 8 bytes at a time where the address is 8-byte aligned and 8 bytes are left in the window, byte by byte
//                      before and behind.  The score D[m][c] is followed at bit (m - 1) mod 64 of word (m - 1) / 64; best, e (first
//                      column attaining it) and last (last column) are three registers.
//                      Instantiated for NW = 1, 2, 3, 4, 8: a request of ceil(m / 64) words is taken by the smallest NW that holds it,
//                      the others pass it by, so that a 150-base mate carries 3 words of state and not 8.  The lanes of a wave are in
//                      step where the mates of a call are equally long (a sequencing run); mixed lengths cost idle lanes, not results.
//                      NW = 1 also writes the answer of every request that is not looked at.
//   k_rescue_wfa       one wavefront per request the scan settled with 0 <= d* <= max_edits: the furthest-reaching points over A = R read
//                      downwards from its last base and B = the reference read downwards from window column e - 1, one diagonal per
//                      lane, levels 0..d*; E == d* by construction, checked; the traceback into the path word and its replay
//   k_rescue_emit      one lane per request with a row: the replay of the stored path, runs written back to front (reference order)
// Every index that comes out of memory (q_lo, q_hi, w_lo, w_hi, the scan's own e and d*, path word, offset) is range-checked before it
// addresses anything: krs_request admits a request only where the mate lies inside qtext and the window inside rtext, krs_end an end
// column only inside the window.
#pragma once
#include "kh_kernels_ends.h"

#define KRS_NONE (-1)
#define KRS_OVER (-2)
#define KRS_MAX_READ 512u
#define KRS_MAX_WINDOW 65536u
#define KRS_THREADS 64      // k_rescue_scan: one wave per block, so that few requests still spread over many SIMDs

// T: the texts, ref_base and max_edits (no anchors: null); n requests
struct KrsArgs {
  KedArgs T;
  const uint32_t* q_lo; const uint32_t* q_hi; const uint32_t* w_lo; const uint32_t* w_hi; const uint8_t* rev;
  uint32_t n;
};
// a request that passed the range checks: the mate qtext[q_lo, q_hi) of m bases, the window rtext[w0, w0 + W) whose first base is the
// global coordinate w_lo
struct KrsReq { uint32_t q_lo, q_hi, w_lo, w0, W, m, rev; };

// request j as kh_mate_rescue defines one that is looked at -> false: KH_RESCUE_NONE
__device__ __forceinline__ bool krs_request(const KrsArgs& P, uint32_t j, KrsReq& R) {
  const uint32_t lo = P.q_lo[j], hi = P.q_hi[j], wl = P.w_lo[j], wh = P.w_hi[j];
  if (lo >= hi || hi > P.T.nq || hi - lo > KRS_MAX_READ) return false;
  if (wl < P.T.ref_base || wh < wl || wh - P.T.ref_base > P.T.nr || wh - wl > KRS_MAX_WINDOW) return false;
  R.q_lo = lo; R.q_hi = hi; R.w_lo = wl; R.w0 = wl - P.T.ref_base; R.W = wh - wl; R.m = hi - lo; R.rev = P.rev[j] & 1u;
  return true;
}
// the instantiation that takes a mate of nw words
__device__ __forceinline__ int krs_class(uint32_t nw) { return nw <= 4u ? (int)nw : 8; }

// one block of one column: the equality word Eq, the vertical deltas VP / VN of the block and the horizontal delta hin (-1, 0, 1) that
// enters at its bit 0 -> the delta that leaves at bit 63; Ph / Mh: the horizontal deltas of the block's rows before the shift
__device__ __forceinline__ int krs_block(uint64_t Eq, uint64_t& VP, uint64_t& VN, int hin, uint64_t& Ph, uint64_t& Mh) {
  const uint64_t hneg = hin < 0 ? 1ull : 0ull, hpos = hin > 0 ? 1ull : 0ull;
  const uint64_t Xv = Eq | VN;
  Eq |= hneg;
  const uint64_t Xh = (((Eq & VP) + VP) ^ VP) | Eq;
  Ph = VN | ~(Xh | VP);
  Mh = VP & Xh;
  const int hout = (int)(Ph >> 63) - (int)(Mh >> 63);
  const uint64_t ph = (Ph << 1) | hpos, mh = (Mh << 1) | hneg;
  VP = mh | ~(Xv | ph);
  VN = ph & Xv;
  return hout;
}

template <int NW>
__global__ __launch_bounds__(KRS_THREADS) void k_rescue_scan(KrsArgs P, int32_t* __restrict__ out_edits, uint32_t* __restrict__ out_rs, uint32_t* __restrict__ out_re,
                                                             uint32_t* __restrict__ out_span, uint32_t* __restrict__ runs) {
  const uint32_t stride = gridDim.x * KRS_THREADS;
  for (uint32_t j = blockIdx.x * KRS_THREADS + threadIdx.x; j < P.n; j += stride) {
    KrsReq R;
    if (!krs_request(P, j, R)) {
      if (NW == 1) { out_edits[j] = KRS_NONE; out_rs[j] = 0u; out_re[j] = 0u; out_span[j] = 0u; runs[j] = 0u; }
      continue;
    }
    if (krs_class((R.m + 63u) >> 6) != NW) continue;
    // the pattern as bit planes: bit i of word w is base 64 w + i of R -- the mate as it stands, or its reverse complement
    uint64_t PL[NW], PH[NW], PV[NW], VP[NW], VN[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      uint64_t l = 0, h = 0, v = 0;
      for (uint32_t g = 0; g < 8u; ++g) {
        const uint32_t i0 = 64u * (uint32_t)w + 8u * g;
        if (i0 >= R.m) break;
        uint64_t c = ked_codes(R.rev ? ked_load_down(P.T.qtext, R.q_hi - i0) : ked_load_up(P.T.qtext, P.T.nq, R.q_lo + i0));
        if (R.rev) c ^= KED_B(0x02);
        const uint32_t cnt = min(8u, R.m - i0);
        for (uint32_t t = 0; t < cnt; ++t, c >>= 8) {
          const uint64_t bit = 1ull << (8u * g + t);
          if (c & 1ull) l |= bit;
          if (c & 2ull) h |= bit;
          if (!(c & 0x80ull)) v |= bit;
        }
      }
      PL[w] = l; PH[w] = h; PV[w] = v; VP[w] = ~0ull; VN[w] = 0ull;
    }
    const uint32_t sw = (R.m - 1u) >> 6, sb = (R.m - 1u) & 63u;      // where D[m][c] is followed
    int score = (int)R.m, best = (int)R.m;                            // column 0: D[m][0] = m
    uint32_t e = 0, last = 0, col = 0;
    const uint8_t* __restrict__ ref = P.T.rtext + R.w0;
    while (col < R.W) {
      uint64_t codes; uint32_t cnt;
      if ((reinterpret_cast<uintptr_t>(ref + col) & 7u) == 0u && R.W - col >= 8u) { codes = ked_codes(*reinterpret_cast<const uint64_t*>(ref + col)); cnt = 8u; }
      else { codes = ked_codes((uint64_t)ref[col]); cnt = 1u; }
#pragma unroll 1
      for (uint32_t t = 0; t < cnt; ++t, codes >>= 8) {
        const uint64_t b0 = (codes & 1ull) ? ~0ull : 0ull, b1 = (codes & 2ull) ? ~0ull : 0ull, bv = (codes & 0x80ull) ? 0ull : ~0ull;
        int hin = 0;                                                  // the free start: D[0][c] = 0
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          if ((uint32_t)w <= sw) {
            uint64_t Ph, Mh;
            hin = krs_block(PV[w] & bv & ~((PL[w] ^ b0) | (PH[w] ^ b1)), VP[w], VN[w], hin, Ph, Mh);
            if ((uint32_t)w == sw) score += (int)((Ph >> sb) & 1ull) - (int)((Mh >> sb) & 1ull);
          }
        }
        ++col;
        if (score < best) { best = score; e = col; last = col; }
        else if (score == best) last = col;
      }
    }
    const bool over = (uint32_t)best > P.T.max_edits;
    out_edits[j] = over ? KRS_OVER : best;
    out_rs[j] = 0u;                                                   // (k_rescue_wfa: the start)
    out_re[j] = over ? 0u : R.w_lo + e;
    out_span[j] = over ? 0u : last - e;
    runs[j] = 0u;
  }
}

// the strings of phase 2 for request j, from what the scan wrote: A = R read downwards from its last base -- the mate read downwards
// from q_hi, or upwards from q_lo with B complemented instead, which is the same comparison --, B = rtext read downwards from window
// column e - 1, |B| = min(m + max_edits, e).  -> false: no row (not looked at, over, or numbers that are not the scan's)
__device__ __forceinline__ bool krs_end(const KrsArgs& P, uint32_t j, const int32_t* edits, const uint32_t* re, KenEnd& E, int& dstar) {
  KrsReq R;
  if (!krs_request(P, j, R)) return false;
  dstar = edits[j];
  const uint32_t x = re[j];
  if (dstar < 0 || (uint32_t)dstar > P.T.max_edits || x < R.w_lo || x - R.w_lo > R.W) return false;
  const uint32_t e = x - R.w_lo;
  E.a0 = R.rev ? R.q_lo : R.q_hi; E.b0 = R.w0 + e; E.head = R.rev ^ 1u; E.down = 1u; E.rev = R.rev;
  E.dq = (int)R.m; E.dr = (int)min(R.m + P.T.max_edits, e);
  return true;
}

__global__ __launch_bounds__(KED_THREADS) void k_rescue_wfa(KrsArgs P, int32_t* out_edits, uint32_t* __restrict__ out_rs, uint32_t* out_re,
                                                            uint32_t* __restrict__ out_span, uint32_t* __restrict__ runs, uint64_t* __restrict__ paths) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KED_WAVES;
  const int d = (int)lane - 32;
  for (uint32_t row = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * KED_WAVES + (threadIdx.x >> 6))); row < P.n; row += stride) {
    KenEnd E; int dstar;
    if (!krs_end(P, row, out_edits, out_re, E, dstar)) continue;      // (settled by k_rescue_scan)
    const int hi = min(E.dq, E.dr - d);
    int F = lane == 32u ? 0 : KED_NEG;
    uint64_t moves = 0;
    uint32_t e = 0;
    for (;; ++e) {                                               // no clip cost, no early stop: the levels up to the first that holds |A|
      if (F >= 0) F = ked_extend(P.T, E, F, d, hi);
      if (__ballot(F == E.dq) || e == (uint32_t)dstar) break;
      F = kcg_level(F, d, hi, lane, e, moves);
    }
    // the target among the diagonals that hold |A| at this level: the smaller |d|, then d < 0 -- the tie rule of an end with equal S
    const uint64_t key = ken_wave_max(F == E.dq ? ken_key(0, e, d) : 0ull);
    const int tie = 63 - (int)(key & 63u), wd = (tie & 1) ? (tie >> 1) : -(tie >> 1);
    bool ok = key != 0ull && e == (uint32_t)dstar;               // E == d* by construction
    int dd = wd;
    const uint64_t path = kcg_traceback(moves, (int)e, dd, ok);
    if (lane == 0u) {
      KcgRuns<false> R{nullptr, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      int v, rd;
      if (ok && dd == 0 && kcg_walk<false>(P.T, E, path, R, v, rd) && v == E.dq && rd == wd) {
        paths[row] = path; runs[row] = R.n; out_rs[row] = out_re[row] - (uint32_t)(E.dq + wd);
      } else { out_edits[row] = KRS_NONE; out_re[row] = 0u; out_span[row] = 0u; }      // (no scan of this call leads here)
    }
  }
}

__global__ __launch_bounds__(KED_THREADS) void k_rescue_emit(KrsArgs P, const int32_t* __restrict__ edits, const uint32_t* __restrict__ re, const uint64_t* __restrict__ offsets,
                                                             const uint64_t* __restrict__ paths, uint64_t total, uint32_t* __restrict__ out_ops) {
  const uint32_t stride = gridDim.x * KED_THREADS;
  for (uint32_t row = blockIdx.x * KED_THREADS + threadIdx.x; row < P.n; row += stride) {
    const uint64_t o0 = offsets[row], o1 = offsets[row + 1];
    if (o1 <= o0 || o1 > total || o1 - o0 > 63ull) continue;     // an empty row; or offsets that are not this call's
    KenEnd E; int dstar;
    if (!krs_end(P, row, edits, re, E, dstar)) continue;
    KcgRuns<true> R{out_ops + o0, (uint32_t)(o1 - o0), 0u, 0u, 0u, 0u, 0u, 1u};      // found from the end: stored in reference order
    int v, d;
    kcg_walk<true>(P.T, E, paths[row], R, v, d);
  }
}
