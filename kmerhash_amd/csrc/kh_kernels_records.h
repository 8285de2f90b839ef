// kh_kernels_records.h -- gfx950 device code of kh_chain_records and kh_cigar_text, included once by kmerhash_amd.hip after
// kh_kernels_select.h.  Prefixes k_records_ and k_text_.
//
// kh_chain_records joins what the chain calls left in pieces -- the link rows of kh_chain_cigars, the two end rows and the clips of
// kh_chain_ends, the chains' first and last anchors -- into one run-length row and one line of numbers per chain (definition:
// include/kmerhash_amd.h, model: tests/records_model.py).  No text is read.
//   k_records_count  one wavefront per chain, fixed grid, grid-stride over the chains: the pieces before the links (clip, head row) go
//                    through the run machine wave-uniformly; then the wave walks the anchors [first, last] 64 per step with one
//                    coalesced load of chain[]: a member lane runs the machine over its own link row from an empty state (runs,
//                    first and last op, the three sums), takes the last op of the nearest non-empty piece before it -- a lane read
//                    below it in the ballot of non-empty pieces, or the value carried across steps -- and merges its first run iff
//                    the two ops are equal; the pieces behind the links (k '=', tail row, clip) go through the machine again.
//                    Runs of the chain = the sum of (runs - merge) over the pieces.  Writes the nine numbers and the run count
//   k_records_emit   the same walk; a wave prefix sum over (runs - merge) gives every piece the output index of its first new run,
//                    and the lane runs the machine over its row from the state (that index, the op before it).  A run goes to its
//                    place with an integer atomic add onto the zeroed row: a first run that merges adds its length to the run
//                    before its piece, wherever the cascade of single-run pieces has put that -- sums of integers, so the bits do
//                    not depend on the order.  With ref_order a reverse-strand chain's run r goes to place n - 1 - r
// The run machine is the definition: a run of length 0 vanishes, a run whose op equals the op before it adds its length to it
// (mod 2^28: the length field), any other starts a new run.
//
// kh_cigar_text renders a run CSR as text: decimal length, then the op letter.
//   k_text_count     one lane per run: its bytes (digits + 1)
//   k_text_rows      one lane per row bound: the byte offset of the bound, from the scan of the byte counts; the last one is the total
//   k_text_emit      one lane per run: the digits and the letter, byte stores at its scanned offset
// Both scans are the index's (k_index_tile_sums / _scan_sums / _scan_apply), unchanged.
// Every index that comes out of memory (c_first, c_last, chain, both offset arrays, the scanned offsets) is range-checked or clamped
// before it addresses anything: a row of more than 63 runs counts as empty, a row bound is clamped to the number of runs, a run is
// written only inside its own chain's row and below the total the host passes in.
#pragma once
#include "kh_kernels_cigar.h"

#define KRC_THREADS 256
#define KRC_WAVES (KRC_THREADS / 64)
#define KRC_NONE 16u          // no op before this one
#define KRC_S 4u              // BAM soft clip
#define KRC_ROWMAX 63u        // runs of a link or end row (2 * 31 + 1)
#define KRC_LENMASK 0x0fffffffu

struct KrcArgs {
  const uint32_t* qpos; const uint32_t* rpos; const uint8_t* rev; const int32_t* chain;
  const uint64_t* lk_off; const uint32_t* lk_ops;
  const uint32_t* c_first; const uint32_t* c_last; const uint32_t* q_lo; const uint32_t* q_hi;
  const uint32_t* e_q; const uint32_t* e_r; const uint32_t* e_clip; const uint64_t* en_off; const uint32_t* en_ops;
  uint64_t n_lk, n_en;
  uint32_t m, n_chains, k, ref_order;
};
struct KrcOut {
  uint8_t* valid;
  uint32_t *qs, *qe, *rs, *re, *qlen, *n_match, *n_block, *nm;
};

// row `i` of a CSR with `n` runs: bounds clamped to [0, n], a descending pair or more than KRC_ROWMAX runs -> empty
__device__ __forceinline__ uint32_t krc_row(const uint64_t* __restrict__ off, uint64_t n, uint64_t i, uint64_t& o0) {
  const uint64_t a = min(off[i], n), b = min(off[i + 1], n);
  o0 = a;
  return b > a && b - a <= (uint64_t)KRC_ROWMAX ? (uint32_t)(b - a) : 0u;
}

// the run machine.  pos: the index of the next new run; op: the op of the run before it (KRC_NONE: none).  With EMIT a run is added to
// out[place(index)] while the index lies below n_row: the row was zeroed, so the sum is the run
template <bool EMIT>
struct KrcMachine {
  uint32_t pos, op, first;            // first: the op of the first run that was fed (KRC_NONE: none yet)
  uint32_t s_match, s_block, s_nm;
  uint32_t* out; uint32_t n_row, flip; bool write;
  __device__ __forceinline__ void feed(uint32_t o, uint32_t l) {
    if (!l) return;
    if (first == KRC_NONE) first = o;
    if (o == KCG_EQ) { s_match += l; s_block += l; }
    else if (o == KCG_X || o == KCG_I || o == KCG_D) { s_block += l; s_nm += l; }
    uint32_t at, v;
    if (o == op) { at = pos - 1u; v = l << 4; }
    else { at = pos++; v = (l << 4) | o; op = o; }
    if (EMIT && write && at < n_row) atomicAdd(&out[flip ? n_row - 1u - at : at], v);
  }
  __device__ __forceinline__ void row(const uint32_t* __restrict__ ops, uint64_t o0, uint32_t n) {
    for (uint32_t j = 0; j < n; ++j) { const uint32_t v = ops[o0 + j]; feed(v & 15u, v >> 4); }
  }
};

__device__ __forceinline__ uint32_t krc_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t krc_wave_sum(uint32_t v) {
  for (int m = 1; m < 64; m <<= 1) v += (uint32_t)__shfl_xor((int)v, m);
  return v;
}

// the eight per-chain numbers of the input, one load by each of the lanes 0..7: the seven pointers live in one register pair per lane
struct KrcNums { uint32_t hq, tq, hr, tr, lo, hi, hclip, tclip; };
__device__ __forceinline__ const uint32_t* krc_src(const KrcArgs& P, uint32_t lane) {
  return lane < 2u ? P.e_q : lane < 4u ? P.e_r : lane == 4u ? P.q_lo : lane == 5u ? P.q_hi : P.e_clip;
}
__device__ __forceinline__ KrcNums krc_nums(const uint32_t* src, uint32_t c, uint32_t lane) {
  uint32_t v = 0;
  if (lane < 8u) v = src[(lane & 6u) == 4u ? c : 2u * c + (lane & 1u)];
  KrcNums N;
  N.hq = (uint32_t)__shfl((int)v, 0); N.tq = (uint32_t)__shfl((int)v, 1); N.hr = (uint32_t)__shfl((int)v, 2); N.tr = (uint32_t)__shfl((int)v, 3);
  N.lo = (uint32_t)__shfl((int)v, 4); N.hi = (uint32_t)__shfl((int)v, 5); N.hclip = (uint32_t)__shfl((int)v, 6); N.tclip = (uint32_t)__shfl((int)v, 7);
  return N;
}

// the walk of one chain by one wave.  EMIT: the chain's row is out[0, n_row), zeroed.  -> the number of runs; valid and the sums by
// reference (the same in every lane)
template <bool EMIT>
__device__ __forceinline__ uint32_t krc_walk(const KrcArgs& P, uint32_t c, uint32_t f, uint32_t l, uint32_t lane, const KrcNums& N, uint32_t* out, uint32_t n_row,
                                             uint32_t flip, bool& bad, uint32_t& s_match, uint32_t& s_block, uint32_t& s_nm) {
  // the pieces before the links, the same in every lane; lane 0 writes
  KrcMachine<EMIT> U{0u, KRC_NONE, KRC_NONE, 0u, 0u, 0u, out, n_row, flip, lane == 0u};
  uint64_t o0;
  U.feed(KRC_S, N.hclip & KRC_LENMASK);
  uint32_t n = krc_row(P.en_off, P.n_en, 2ull * c, o0);
  U.row(P.en_ops, o0, n);
  uint32_t pos = krc_uniform(U.pos), prev = krc_uniform(U.op);
  uint32_t m_match = 0, m_block = 0, m_nm = 0;       // the member lanes' own sums
  bad = false;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t base = f; base <= l; base += 64u) {   // (l < m <= 2^24: base does not wrap)
    const uint32_t i = base + lane;
    const bool member = i > f && i <= l && P.chain[i] == (int32_t)c;
    uint32_t rn = 0;
    if (member) rn = krc_row(P.lk_off, P.n_lk, i, o0);
    if (__ballot(member && rn == 0u)) bad = true;
    // the piece by itself
    KrcMachine<false> M{0u, KRC_NONE, KRC_NONE, 0u, 0u, 0u, nullptr, 0u, 0u, false};
    if (member) M.row(P.lk_ops, o0, rn);
    m_match += M.s_match; m_block += M.s_block; m_nm += M.s_nm;
    const unsigned long long ne = __ballot(M.pos != 0u);
    if (!ne) continue;
    // the op before this piece: the last op of the nearest non-empty piece below, or the carried one
    const unsigned long long lower = ne & below;
    const uint32_t got = (uint32_t)__shfl((int)M.op, lower ? 63 - __builtin_clzll(lower) : 0);
    const uint32_t before = lower ? got : prev;
    const uint32_t merge = M.pos != 0u && M.first == before ? 1u : 0u;
    const uint32_t add = M.pos - merge;
    uint32_t incl = add;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, d); if (lane >= (uint32_t)d) incl += t; }
    if (EMIT && M.pos != 0u) {
      KrcMachine<true> W{pos + incl - add, before, KRC_NONE, 0u, 0u, 0u, out, n_row, flip, true};
      W.row(P.lk_ops, o0, rn);
    }
    pos += (uint32_t)__shfl((int)incl, 63);
    prev = krc_uniform((uint32_t)__shfl((int)M.op, 63 - __builtin_clzll(ne)));
    pos = krc_uniform(pos);
  }
  // the pieces behind the links
  KrcMachine<EMIT> V{pos, prev, KRC_NONE, 0u, 0u, 0u, out, n_row, flip, lane == 0u};
  V.feed(KCG_EQ, P.k);
  n = krc_row(P.en_off, P.n_en, 2ull * c + 1ull, o0);
  V.row(P.en_ops, o0, n);
  V.feed(KRC_S, N.tclip & KRC_LENMASK);
  s_match = U.s_match + V.s_match + krc_wave_sum(m_match);
  s_block = U.s_block + V.s_block + krc_wave_sum(m_block);
  s_nm = U.s_nm + V.s_nm + krc_wave_sum(m_nm);
  return krc_uniform(V.pos);
}

// the range conditions of a chain -> 0: nothing can be read through first / last; 1: the intervals can be written; 2: the row can be
// walked (the link rows are checked by the walk)
__device__ __forceinline__ uint32_t krc_chain(const KrcArgs& P, uint32_t c, const KrcNums& N, uint32_t& f, uint32_t& l) {
  f = krc_uniform(P.c_first[c]); l = krc_uniform(P.c_last[c]);
  if (f > l || l >= P.m) return 0u;
  if (P.chain[f] != (int32_t)c || P.chain[l] != (int32_t)c) return 0u;
  const uint32_t lo = N.lo, hi = N.hi;
  if (lo > P.qpos[f] || (uint64_t)P.qpos[l] + P.k > hi || hi - lo >= (uint32_t)KCG_MAXLEN) return 1u;
  return 2u;
}

__global__ __launch_bounds__(KRC_THREADS) void k_records_count(KrcArgs P, KrcOut O, uint32_t* __restrict__ runs) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KRC_WAVES;
  // lanes 0..8 write one of the chain's nine u32 numbers each: one store, and the nine pointers live in one register pair per lane
  uint32_t* const mine = lane == 0u ? O.qs : lane == 1u ? O.qe : lane == 2u ? O.rs : lane == 3u ? O.re : lane == 4u ? O.qlen : lane == 5u ? O.n_match
                       : lane == 6u ? O.n_block : lane == 7u ? O.nm : runs;
  uint8_t* const valid = O.valid;
  const uint32_t* const src = krc_src(P, lane);
  for (uint32_t c = krc_uniform(blockIdx.x * KRC_WAVES + (threadIdx.x >> 6)); c < P.n_chains; c += stride) {
    uint32_t f, l;
    const KrcNums N = krc_nums(src, c, lane);
    const uint32_t level = krc_chain(P, c, N, f, l);
    uint32_t qs = 0, qe = 0, rs = 0, re = 0;
    if (level) {
      const uint32_t rv = P.rev[f] & 1u, rf = P.rpos[f], rl = P.rpos[l];
      qs = P.qpos[f] - N.hq - N.lo; qe = P.qpos[l] + P.k + N.tq - N.lo;
      rs = min(rf, rl) - (rv ? N.tr : N.hr); re = max(rf, rl) + P.k + (rv ? N.hr : N.tr);
    }
    uint32_t n = 0, s_match = 0, s_block = 0, s_nm = 0;
    bool bad = true;
    if (level == 2u) n = krc_walk<false>(P, c, f, l, lane, N, nullptr, 0u, 0u, bad, s_match, s_block, s_nm);
    if (bad) { n = 0; s_match = 0; s_block = 0; s_nm = 0; }
    const uint32_t num = lane == 0u ? qs : lane == 1u ? qe : lane == 2u ? rs : lane == 3u ? re : lane == 4u ? N.hi - N.lo : lane == 5u ? s_match
                       : lane == 6u ? s_block : lane == 7u ? s_nm : n;
    if (lane < 9u) mine[c] = num;
    if (lane == 9u) valid[c] = bad ? 0 : 1;
  }
}

__global__ __launch_bounds__(KRC_THREADS) void k_records_emit(KrcArgs P, const uint64_t* __restrict__ offsets, uint64_t total, uint32_t* __restrict__ out_ops) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KRC_WAVES;
  const uint32_t* const src = krc_src(P, lane);
  for (uint32_t c = krc_uniform(blockIdx.x * KRC_WAVES + (threadIdx.x >> 6)); c < P.n_chains; c += stride) {
    const uint64_t o0 = offsets[c], o1 = offsets[c + 1];
    if (o1 <= o0 || o1 > total || o1 - o0 >= (1ull << 31)) continue;      // an empty row; or offsets that are not this call's
    uint32_t f, l;
    const KrcNums N = krc_nums(src, c, lane);
    if (krc_chain(P, c, N, f, l) != 2u) continue;
    bool bad;
    uint32_t a, b, d;
    krc_walk<true>(P, c, f, l, lane, N, out_ops + o0, (uint32_t)(o1 - o0), P.ref_order & P.rev[f] & 1u, bad, a, b, d);
  }
}

// ---- kh_cigar_text
#define KTX_THREADS 256
// bytes of one run: the decimal digits of its length (1..9: a length has 28 bits) and the op letter
__device__ __forceinline__ uint32_t ktx_bytes(uint32_t v) {
  const uint32_t l = v >> 4;
  return 2u + (l >= 10u) + (l >= 100u) + (l >= 1000u) + (l >= 10000u) + (l >= 100000u) + (l >= 1000000u) + (l >= 10000000u) + (l >= 100000000u);
}
__global__ __launch_bounds__(KTX_THREADS) void k_text_count(const uint32_t* __restrict__ ops, uint64_t n_ops, uint32_t* __restrict__ bytes) {
  const uint64_t stride = (uint64_t)gridDim.x * KTX_THREADS;
  for (uint64_t r = (uint64_t)blockIdx.x * KTX_THREADS + threadIdx.x; r < n_ops; r += stride) bytes[r] = ktx_bytes(ops[r]);
}
// bound i of the rows, clamped to [base, n_ops] with base = the clamped bound 0: its byte offset; total = that of bound n_rows
__global__ __launch_bounds__(KTX_THREADS) void k_text_rows(const uint64_t* __restrict__ offsets, uint64_t n_rows, uint64_t n_ops, const uint64_t* __restrict__ boff,
                                                           uint64_t* __restrict__ out_offsets, unsigned long long* __restrict__ total) {
  const uint64_t stride = (uint64_t)gridDim.x * KTX_THREADS;
  const uint64_t base = min(offsets[0], n_ops);
  for (uint64_t i = (uint64_t)blockIdx.x * KTX_THREADS + threadIdx.x; i <= n_rows; i += stride) {
    const uint64_t o = max(min(offsets[i], n_ops), base);
    const uint64_t v = boff[o] - boff[base];
    out_offsets[i] = v;
    if (i == n_rows) *total = v;
  }
}
__global__ __launch_bounds__(KTX_THREADS) void k_text_emit(const uint32_t* __restrict__ ops, const uint64_t* __restrict__ offsets, uint64_t n_rows, uint64_t n_ops,
                                                           const uint64_t* __restrict__ boff, uint64_t total, uint8_t* __restrict__ out_text) {
  const uint64_t stride = (uint64_t)gridDim.x * KTX_THREADS;
  const uint64_t base = min(offsets[0], n_ops), hi = max(min(offsets[n_rows], n_ops), base);
  for (uint64_t r = base + (uint64_t)blockIdx.x * KTX_THREADS + threadIdx.x; r < hi; r += stride) {
    const uint32_t v = ops[r], nb = ktx_bytes(v);
    const uint64_t at = boff[r] - boff[base];
    if (at + nb > total) continue;                                        // offsets that are not this call's
    uint32_t l = v >> 4;
    const uint32_t o = v & 15u;
    out_text[at + nb - 1u] = o < 9u ? (uint8_t)"MIDNSHP=X"[o] : (uint8_t)'?';
    for (uint32_t j = nb - 1u; j-- > 0u;) { out_text[at + j] = (uint8_t)('0' + l % 10u); l /= 10u; }
  }
}
