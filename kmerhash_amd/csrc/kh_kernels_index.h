// kh_kernels_index.h -- gfx950 device code of the k-mer position index (kh_index_* and kh_kmers_from_*_pos), included once by
// kmerhash_amd.hip after kh_kernels_values.h.  Prefix ki_ / k_index_ (and k_kmers_emit_pos, the sibling of k_kmers_emit).
//
// The index is a Robin Hood table of 64-bit keys whose VALUE is the key's rank among the live slots in slot order, plus a CSR:
// offsets u32[size + 1] and positions u32[total]; positions[offsets[r] .. offsets[r + 1]) are the occurrences of the key of rank r,
// ascending.  Build: counting insert (unchanged code) -> k_index_canon_runs (keys of one home bucket in key order) -> k_index_rank
// (slot-order rank, counts, rank into the slot) -> scan ->
// k_index_scatter (probe + cursor atomic + 4-byte write per pair) -> k_index_tile_sort (bitonic sort of fixed tiles in LDS under the
// composite key (segment in tile, position)) -> k_index_seg_radix (the segments that cross a tile boundary, one workgroup each).
// Lookup: k_index_lookup (begin, count per query) -> scan -> k_index_gather (balanced over output elements).  Wave64 everywhere.
#pragma once
#include "kh_kernels_values.h"

// ---------------------------------------------------------------------------------------------
// k-mers with the byte offset of their window: k_kmers_emit plus a second staging array.  The offset of the window that starts at base
// j of lane tid's word is tile0 + 16 tid + j; the tile-local part (< KH_KM_TILE) is staged as 16 bits next to the k-mer and both are
// written coalesced.
// ---------------------------------------------------------------------------------------------
template <bool CANON>
__global__ __launch_bounds__(KH_KM_THREADS) void k_kmers_emit_pos(const uint8_t* __restrict__ seq, uint64_t n, uint32_t k, const uint64_t* __restrict__ tile_off,
                                                                  uint64_t* __restrict__ out, uint32_t* __restrict__ out_pos) {
  typedef KhKm<1> M;
  __shared__ uint32_t words[KH_KM_TILE / 16 + M::HALO];
  __shared__ uint16_t invs[KH_KM_TILE / 16 + M::HALO];
  __shared__ uint32_t wtot[KH_KM_THREADS / 64];
  __shared__ uint64_t stage[KH_KM_TILE];
  __shared__ uint16_t spos[KH_KM_TILE];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t tile0 = (uint64_t)blockIdx.x * KH_KM_TILE;
  kh_km_pack_tile<M::HALO>(seq, n, tile0, words, invs);
  __syncthreads();
  const M::Win W = M::window(words, invs, tid);
  uint32_t vmask = 0;
#pragma unroll
  for (uint32_t j = 0; j < 16; ++j) vmask |= M::valid(W, j, k) ? (1u << j) : 0u;
  const uint32_t mine = (uint32_t)__popc(vmask);
  uint32_t incl = mine;
  for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); if (lane >= (uint32_t)off) incl += o; }
  if (lane == 63) wtot[wid] = incl;
  __syncthreads();
  uint32_t pos = incl - mine, total = 0;
#pragma unroll
  for (uint32_t w = 0; w < KH_KM_THREADS / 64; ++w) { const uint32_t c = wtot[w]; if (w < wid) pos += c; total += c; }
#pragma unroll
  for (uint32_t j = 0; j < 16; ++j) {
    if ((vmask >> j) & 1u) {
      const uint64_t fw = M::forward(W, j, k);
      uint64_t v = fw;
      if (CANON) { const uint64_t rc = kh_revcomp(fw, k); v = fw < rc ? fw : rc; }
      stage[pos] = v;
      spos[pos] = (uint16_t)(16u * tid + j);
      ++pos;
    }
  }
  __syncthreads();
  const uint64_t o = tile_off[blockIdx.x];
  for (uint32_t i = tid; i < total; i += KH_KM_THREADS) { out[o + i] = stage[i]; out_pos[o + i] = (uint32_t)(tile0 + spos[i]); }
}

// ---------------------------------------------------------------------------------------------
// (w,k)-minimizer sampling (kh_minimizers_from_sequence / _fastq; the definition is in include/kmerhash_amd.h): the tile scheme of
// k_kmers_count / k_kmers_emit_pos with a halo on BOTH sides.  A tile decides the picks among its KH_KM_TILE start offsets; the
// windows that can pick one of them start up to w - 1 offsets to its left and reach up to w - 1 offsets past its right end, so the
// tile hashes HW = ceil((w - 1) / 16) words of 16 offsets on either side as well (w = 10: 2 words on top of 256, w = 256: 32).
//   1. pack: the HW words left of the tile (non-bases in front of the text), then kh_km_pack_tile for the tile and what lies behind it.
//   2. hash once per offset: the order key kh_hash64<HASH>(emitted k-mer, seed) into LDS (hk, 8 B per offset, a row of 16 keys padded
//      by one so that the 16 consecutive stores of a lane spread over the banks) and arg[i] = i for a valid window, KM_MZ_NONE otherwise.
//   3. window minimum in O(log w) per offset: J = floor(log2 w) doubling steps turn arg[i] into the offset of the smallest (key, offset)
//      among [i, i + 2^J) -- or KM_MZ_NONE when one of them is no valid window --, in place (a lane holds its <= 18 results in registers
//      across the barrier).  The pick of the window that starts at s is the smaller of arg[s] and arg[s + w - 2^J] (two overlapping
//      ranges that cover [s, s + w)); the right one wins only with a strictly smaller key, so ties go to the leftmost offset, and a
//      window with an invalid offset (not full) picks nothing.  Work per offset: J + 1 steps of two 2-byte and two 8-byte LDS reads.
//   4. every full window marks its pick in a 4096-bit mask (LDS atomic or; a lane skips the atomic when the window before it -- the
//      lane before it -- picked the same offset).  Picks outside the tile belong to the neighbour tile, which finds them itself.
// LDS: 39168 (keys) + 9216 (arg) + 1160 + 580 (packed text) + 512 (marks) + 16 = 50652 B (50656 padded): three workgroups per CU,
// three waves per SIMD, which the launch bounds also hold the registers to.
// The count kernel sums the marks; the emit kernel stages the marked windows' k-mers over the keys (which are dead by then) and their
// tile-local offsets over arg, and writes both coalesced.  No hash and no flag reaches HBM: 1 B/base read per pass, 12 B per pair out.
// ---------------------------------------------------------------------------------------------
#define KM_MZ_WMAX 256
#define KM_MZ_HALO_WORDS ((KM_MZ_WMAX - 1 + 15) / 16)                       // 16
#define KM_MZ_WORDS (KH_KM_TILE / 16 + 2 * KM_MZ_HALO_WORDS)                 // 288 words of hashed offsets at most
#define KM_MZ_OFFS (16 * KM_MZ_WORDS)                                        // 4608
#define KM_MZ_PER ((KM_MZ_OFFS + KH_KM_THREADS - 1) / KH_KM_THREADS)         // 18
#define KM_MZ_NONE 0xFFFFu
#define KM_MZ_HK(i) ((i) + ((i) >> 4))
struct KmMzLds {
  uint64_t hk[KM_MZ_OFFS + KM_MZ_WORDS];            // order keys, 17 per word of 16 offsets; the emit stage afterwards
  uint16_t arg[KM_MZ_OFFS];                         // offset of the range minimum / KM_MZ_NONE; the staged offsets afterwards
  uint32_t words[KM_MZ_WORDS + KhKm<1>::HALO];
  uint16_t invs[KM_MZ_WORDS + KhKm<1>::HALO];
  uint32_t marks[KH_KM_TILE / 32];
  uint32_t wtot[KH_KM_THREADS / 64];
};
// leaves S.marks complete (bit q: the window at tile0 + q is a minimizer) and the workgroup synchronised; returns HW
template <int HASH, bool CANON>
__device__ __forceinline__ uint32_t km_mz_marks(const uint8_t* __restrict__ seq, uint64_t n, uint64_t tile0, uint32_t k, uint32_t w, uint64_t seed, KmMzLds& S) {
  typedef KhKm<1> M;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t hw = (w + 14u) >> 4, nw = KH_KM_TILE / 16 + 2 * hw, ne = 16 * nw;
  if (tid < hw) {                                                  // (tile0 > 0: tile0 >= KH_KM_TILE > 16 hw, and the 16 bytes lie inside the text)
    uint32_t word = 0, inv = 0xFFFFu;
    if (tile0) {
      const uint8_t* p = seq + (tile0 - 16ull * (hw - tid));
      inv = 0;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const uint32_t c = kh_dna_code(p[q]);
        word = (word << 2) | (c & 3u);
        inv = (inv << 1) | (c > 3u ? 1u : 0u);
      }
    }
    S.words[tid] = word; S.invs[tid] = (uint16_t)inv;
  }
  if (tid < KH_KM_TILE / 32) S.marks[tid] = 0;
  kh_km_pack_tile<KM_MZ_HALO_WORDS + M::HALO>(seq, n, tile0, S.words + hw, S.invs + hw);
  __syncthreads();
  for (uint32_t e = tid; e < nw; e += KH_KM_THREADS) {
    const M::Win W = M::window(S.words, S.invs, e);
#pragma unroll 4                                                   // (four hashes in flight; sixteen cost 170 registers and spills)
    for (uint32_t j = 0; j < 16; ++j) {
      const uint32_t i = 16 * e + j;
      S.hk[KM_MZ_HK(i)] = M::template hash_of_window<HASH, CANON>(W, j, k, seed);
      S.arg[i] = M::valid(W, j, k) ? (uint16_t)i : (uint16_t)KM_MZ_NONE;
    }
  }
  __syncthreads();
  const uint32_t J = 31u - (uint32_t)__clz(w);
  for (uint32_t s = 0; s < J; ++s) {
    const uint32_t step = 1u << s;
    uint32_t res[KM_MZ_PER];
#pragma unroll
    for (uint32_t r = 0; r < KM_MZ_PER; ++r) {
      const uint32_t i = tid + r * KH_KM_THREADS;
      uint32_t a = KM_MZ_NONE;
      if (i + step < ne) {
        a = S.arg[i];
        const uint32_t b = S.arg[i + step];
        if (b == KM_MZ_NONE) a = KM_MZ_NONE;
        else if (a != KM_MZ_NONE && S.hk[KM_MZ_HK(b)] < S.hk[KM_MZ_HK(a)]) a = b;
      }
      res[r] = a;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < KM_MZ_PER; ++r) {
      const uint32_t i = tid + r * KH_KM_THREADS;
      if (i < ne) S.arg[i] = (uint16_t)res[r];
    }
    __syncthreads();
  }
  const uint32_t back = w - (1u << J);
#pragma unroll
  for (uint32_t r = 0; r < KM_MZ_PER; ++r) {
    const uint32_t s = tid + r * KH_KM_THREADS;
    uint32_t p = KM_MZ_NONE;
    if (s + w <= ne) {
      p = S.arg[s];
      const uint32_t b = S.arg[s + back];
      if (b == KM_MZ_NONE) p = KM_MZ_NONE;
      else if (p != KM_MZ_NONE && S.hk[KM_MZ_HK(b)] < S.hk[KM_MZ_HK(p)]) p = b;
    }
    const uint32_t before = __shfl_up(p, 1, 64);
    const uint32_t q = p - 16u * hw;                               // (a pick left of the tile wraps past KH_KM_TILE)
    if (p != KM_MZ_NONE && q < KH_KM_TILE && (lane == 0 || before != p)) atomicOr(&S.marks[q >> 5], 1u << (q & 31u));
  }
  __syncthreads();
  return hw;
}
template <int HASH, bool CANON>
__global__ __launch_bounds__(KH_KM_THREADS, 3) void k_minimizers_count(const uint8_t* __restrict__ seq, uint64_t n, uint32_t k, uint32_t w, uint64_t seed,
                                                                    uint32_t* __restrict__ sums) {
  __shared__ KmMzLds S;
  km_mz_marks<HASH, CANON>(seq, n, (uint64_t)blockIdx.x * KH_KM_TILE, k, w, seed, S);
  uint32_t c = threadIdx.x < KH_KM_TILE / 32 ? (uint32_t)__popc(S.marks[threadIdx.x]) : 0u;
  c = kh_wave_sum(c);
  if ((threadIdx.x & 63) == 0) S.wtot[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = S.wtot[0] + S.wtot[1] + S.wtot[2] + S.wtot[3];
}
// out_pos[i] = pos_base + the window's byte offset (pos_base: the coordinate space of kh_index_append_from_minimizers)
template <int HASH, bool CANON>
__global__ __launch_bounds__(KH_KM_THREADS, 3) void k_minimizers_emit(const uint8_t* __restrict__ seq, uint64_t n, uint32_t k, uint32_t w, uint64_t seed,
                                                                   const uint64_t* __restrict__ tile_off, uint64_t* __restrict__ out, uint32_t* __restrict__ out_pos,
                                                                   uint32_t pos_base) {
  typedef KhKm<1> M;
  __shared__ KmMzLds S;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t tile0 = (uint64_t)blockIdx.x * KH_KM_TILE;
  const uint32_t hw = km_mz_marks<HASH, CANON>(seq, n, tile0, k, w, seed, S);
  const uint32_t pmask = (S.marks[tid >> 1] >> (16u * (tid & 1u))) & 0xFFFFu;      // the 16 windows of the lane's word
  const uint32_t mine = (uint32_t)__popc(pmask);
  uint32_t incl = mine;
  for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); if (lane >= (uint32_t)off) incl += o; }
  if (lane == 63) S.wtot[wid] = incl;
  __syncthreads();
  uint32_t pos = incl - mine, total = 0;
#pragma unroll
  for (uint32_t x = 0; x < KH_KM_THREADS / 64; ++x) { const uint32_t c = S.wtot[x]; if (x < wid) pos += c; total += c; }
  const M::Win W = M::window(S.words, S.invs, tid + hw);
  uint64_t* stage = S.hk;                                          // (every read of the keys lies before the barrier km_mz_marks ends with)
  uint16_t* spos = S.arg;
#pragma unroll
  for (uint32_t j = 0; j < 16; ++j) {
    if ((pmask >> j) & 1u) {
      const uint64_t fw = M::forward(W, j, k);
      stage[pos] = CANON ? kh_xf(fw, k) : fw;
      spos[pos] = (uint16_t)(16u * tid + j);
      ++pos;
    }
  }
  __syncthreads();
  const uint64_t o = tile_off[blockIdx.x];
  for (uint32_t i = tid; i < total; i += KH_KM_THREADS) { out[o + i] = stage[i]; out_pos[o + i] = pos_base + (uint32_t)(tile0 + spos[i]); }
}

// ---------------------------------------------------------------------------------------------
// closed-syncmer sampling (kh_syncmers[128]_from_sequence / _fastq, kh_[wide_]syncmer_mask; the definition is in include/kmerhash_amd.h):
// the k-mer at a valid window p is kept iff the smallest order key among its k - s + 1 s-mers (offsets p .. p + k - s) is the key of
// its first or of its last s-mer.  The tile scheme of the minimizer kernels with a halo on the RIGHT only: a tile decides its
// KH_KM_TILE start offsets and hashes the k - s <= 63 offsets behind them as well (HW = ceil((k - s) / 16) <= 4 words of 16).
//   1. pack: kh_km_pack_tile for the tile, the HW halo words and what the widest window cut needs behind them (KhKm<2>::HALO words for
//      the k-mer of the tile's last lane, KhKm<1>::HALO words for the s-mer of the last hashed offset: KM_SY_HALO_WORDS + 2 in all).
//   2. hash once per offset: the order key kh_hash64<HASH>(s-mer, seed) -- a KhKm<1> window of length s, its canonical form when CANON --
//      into LDS (rows of 16 keys padded by one, as the minimizer keys are) and arg[i] = i, or KM_MZ_NONE when the s bytes are not all bases.
//   3. range minimum by J = floor(log2(k - s + 1)) doubling steps on arg, keys untouched; the minimum over [p, p + k - s] is the smaller
//      of arg[p] and arg[p + k - s + 1 - 2^J] (two overlapping ranges).  A KM_MZ_NONE anywhere in the range gives KM_MZ_NONE, and that is
//      exactly "the k bytes from p are not all bases": no separate test of the k-mer's validity.
//   4. keep test: key[arg] == key[p] || key[arg] == key[p + k - s] (a tie with an inner s-mer keeps the k-mer, which makes the rule
//      exactly strand-symmetric).  A wave decides 64 consecutive offsets per round, so its ballot IS two words of the 4096-bit mask:
//      no LDS atomic.
// LDS: 35360 (keys: 4160 offsets, 17 per 16) + 8320 (arg) + 1048 + 524 (packed text, 262 words) + 512 (marks) + 16 = 45780 B (45784
// padded): three workgroups per CU, three waves per SIMD, which the launch bounds also hold the registers to (a fourth workgroup would
// need <= 40960 B; keys and arg alone are 43680).
// The count kernel sums the marks; it never looks at a k-mer, so it has no key-width parameter and serves both widths.  The emit kernel
// for 8-byte k-mers stages the kept k-mers over the dead keys and their tile-local offsets over arg and writes both coalesced; for
// 16-byte k-mers a full tile (poly-A keeps all 4096 windows) would be 64 KB, so they go straight out as kw_kmers_emit_pos writes them.
// No hash and no flag reaches HBM: 1 B per base read per pass, 12 B (8-byte k-mers) or 20 B (16-byte) per kept pair written.
// ---------------------------------------------------------------------------------------------
#define KM_SY_HALO_WORDS 4                                                   // ceil(63 / 16)
#define KM_SY_WORDS (KH_KM_TILE / 16 + KM_SY_HALO_WORDS)                     // 260 words of hashed offsets at most
#define KM_SY_OFFS (16 * KM_SY_WORDS)                                        // 4160
#define KM_SY_PER ((KM_SY_OFFS + KH_KM_THREADS - 1) / KH_KM_THREADS)         // 17
#define KM_SY_TEXT_HALO (KM_SY_HALO_WORDS + KhKm<1>::HALO)                   // 6 >= KhKm<2>::HALO
struct KmSyLds {
  uint64_t hk[KM_SY_OFFS + KM_SY_WORDS];            // order keys of the s-mers, 17 per word of 16 offsets; the emit stage afterwards (KW = 1)
  uint16_t arg[KM_SY_OFFS];                         // offset of the range minimum / KM_MZ_NONE; the staged offsets afterwards (KW = 1)
  uint32_t words[KH_KM_TILE / 16 + KM_SY_TEXT_HALO];
  uint16_t invs[KH_KM_TILE / 16 + KM_SY_TEXT_HALO];
  uint32_t marks[KH_KM_TILE / 32];
  uint32_t wtot[KH_KM_THREADS / 64];
};
// leaves S.marks complete (bit q: the k-mer of the window at tile0 + q is a closed syncmer) and the workgroup synchronised
template <int HASH, bool CANON>
__device__ __forceinline__ void km_sy_marks(const uint8_t* __restrict__ seq, uint64_t n, uint64_t tile0, uint32_t k, uint32_t s, uint64_t seed, KmSyLds& S) {
  typedef KhKm<1> M;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t span = k - s;                                       // 0..63: the last s-mer of the window at p starts at p + span
  const uint32_t nw = KH_KM_TILE / 16 + ((span + 15u) >> 4), ne = 16 * nw;
  kh_km_pack_tile<KM_SY_TEXT_HALO>(seq, n, tile0, S.words, S.invs);
  __syncthreads();
  for (uint32_t e = tid; e < nw; e += KH_KM_THREADS) {
    const M::Win W = M::window(S.words, S.invs, e);
#pragma unroll 4
    for (uint32_t j = 0; j < 16; ++j) {
      const uint32_t i = 16 * e + j;
      S.hk[KM_MZ_HK(i)] = M::template hash_of_window<HASH, CANON>(W, j, s, seed);
      S.arg[i] = M::valid(W, j, s) ? (uint16_t)i : (uint16_t)KM_MZ_NONE;
    }
  }
  __syncthreads();
  const uint32_t J = 31u - (uint32_t)__clz(span + 1u);
  for (uint32_t d = 0; d < J; ++d) {
    const uint32_t step = 1u << d;
    uint32_t res[KM_SY_PER];
#pragma unroll
    for (uint32_t r = 0; r < KM_SY_PER; ++r) {
      const uint32_t i = tid + r * KH_KM_THREADS;
      uint32_t a = KM_MZ_NONE;
      if (i + step < ne) {
        a = S.arg[i];
        const uint32_t b = S.arg[i + step];
        if (b == KM_MZ_NONE) a = KM_MZ_NONE;
        else if (a != KM_MZ_NONE && S.hk[KM_MZ_HK(b)] < S.hk[KM_MZ_HK(a)]) a = b;
      }
      res[r] = a;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < KM_SY_PER; ++r) {
      const uint32_t i = tid + r * KH_KM_THREADS;
      if (i < ne) S.arg[i] = (uint16_t)res[r];
    }
    __syncthreads();
  }
  const uint32_t back = span + 1u - (1u << J);
#pragma unroll
  for (uint32_t r = 0; r < KH_KM_TILE / KH_KM_THREADS; ++r) {
    const uint32_t p = tid + r * KH_KM_THREADS;                      // (p + span < ne: every read below lies inside the hashed offsets)
    const uint32_t a = S.arg[p], b = S.arg[p + back];
    bool keep = false;
    if (a != KM_MZ_NONE && b != KM_MZ_NONE) {
      const uint64_t ha = S.hk[KM_MZ_HK(a)], hb = S.hk[KM_MZ_HK(b)];
      const uint64_t m = hb < ha ? hb : ha;
      keep = S.hk[KM_MZ_HK(p)] == m || S.hk[KM_MZ_HK(p + span)] == m;
    }
    const unsigned long long bal = __ballot(keep);                   // lanes 0..63 <-> offsets r * 256 + 64 wid + lane
    if (lane == 0) { S.marks[8 * r + 2 * wid] = (uint32_t)bal; S.marks[8 * r + 2 * wid + 1] = (uint32_t)(bal >> 32); }
  }
  __syncthreads();
}
template <int HASH, bool CANON>
__global__ __launch_bounds__(KH_KM_THREADS, 3) void k_syncmers_count(const uint8_t* __restrict__ seq, uint64_t n, uint32_t k, uint32_t s, uint64_t seed,
                                                                  uint32_t* __restrict__ sums) {
  __shared__ KmSyLds S;
  km_sy_marks<HASH, CANON>(seq, n, (uint64_t)blockIdx.x * KH_KM_TILE, k, s, seed, S);
  uint32_t c = threadIdx.x < KH_KM_TILE / 32 ? (uint32_t)__popc(S.marks[threadIdx.x]) : 0u;
  c = kh_wave_sum(c);
  if ((threadIdx.x & 63) == 0) S.wtot[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) sums[blockIdx.x] = S.wtot[0] + S.wtot[1] + S.wtot[2] + S.wtot[3];
}
// out: u64[KW] per kept window ({w0, w1} for KW = 2); out_pos[i] = pos_base + the window's byte offset
template <int HASH, bool CANON, int KW>
__global__ __launch_bounds__(KH_KM_THREADS, 3) void k_syncmers_emit(const uint8_t* __restrict__ seq, uint64_t n, uint32_t k, uint32_t s, uint64_t seed,
                                                                 const uint64_t* __restrict__ tile_off, uint64_t* __restrict__ out, uint32_t* __restrict__ out_pos,
                                                                 uint32_t pos_base) {
  typedef KhKm<KW> M;
  __shared__ KmSyLds S;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t tile0 = (uint64_t)blockIdx.x * KH_KM_TILE;
  km_sy_marks<HASH, CANON>(seq, n, tile0, k, s, seed, S);
  const uint32_t pmask = (S.marks[tid >> 1] >> (16u * (tid & 1u))) & 0xFFFFu;      // the 16 windows of the lane's word
  const uint32_t mine = (uint32_t)__popc(pmask);
  uint32_t incl = mine;
  for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); if (lane >= (uint32_t)off) incl += o; }
  if (lane == 63) S.wtot[wid] = incl;
  __syncthreads();
  uint32_t pos = incl - mine, total = 0;
#pragma unroll
  for (uint32_t x = 0; x < KH_KM_THREADS / 64; ++x) { const uint32_t c = S.wtot[x]; if (x < wid) pos += c; total += c; }
  const typename M::Win W = M::window(S.words, S.invs, tid);
  const uint64_t o = tile_off[blockIdx.x];
  if constexpr (KW == 2) {
    for (uint32_t j = 0; j < 16; ++j) {
      if ((pmask >> j) & 1u) {
        uint64_t w0, w1;
        M::forward(W, j, k, &w0, &w1);
        if (CANON) kh_xf128(&w0, &w1, k);
        reinterpret_cast<ulonglong2*>(out)[o + pos] = make_ulonglong2(w0, w1);
        out_pos[o + pos] = pos_base + (uint32_t)(tile0 + 16u * tid + j);
        ++pos;
      }
    }
  } else {
    uint64_t* stage = S.hk;                                          // (every read of the keys lies before the barrier km_sy_marks ends with)
    uint16_t* spos = S.arg;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
      if ((pmask >> j) & 1u) {
        const uint64_t fw = M::forward(W, j, k);
        stage[pos] = CANON ? kh_xf(fw, k) : fw;
        spos[pos] = (uint16_t)(16u * tid + j);
        ++pos;
      }
    }
    __syncthreads();
    for (uint32_t i = tid; i < total; i += KH_KM_THREADS) { out[o + i] = stage[i]; out_pos[o + i] = pos_base + (uint32_t)(tile0 + spos[i]); }
  }
}
// the same test on a batch of packed k-mers (8-byte: keys u64[n]; 16-byte: keys u64[2n], {w0, w1}): out[i] = 1 iff key i is a closed
// syncmer.  One lane per key, the k - s + 1 s-mers cut from the key's registers (s <= 32: an s-mer is one word), no LDS.  Bits above
// the k-mer's 2k are ignored.  With CANON a key and its reverse complement see the same canonical s-mers in opposite order, and the
// rule is symmetric in first and last: the same answer, whichever strand's bit pattern the caller holds.
template <int HASH, bool CANON, int KW>
__global__ __launch_bounds__(256) void k_syncmer_mask(const uint64_t* __restrict__ keys, uint64_t n, uint32_t k, uint32_t s, uint64_t seed, uint8_t* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t smask = s >= 32 ? ~0ull : ((1ull << (2 * s)) - 1ull);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const uint64_t w0 = keys[KW * i], w1 = KW == 2 ? keys[KW * i + 1] : 0ull;
    uint64_t first = 0, last = 0, m = ~0ull;
    for (uint32_t sh = 2 * (k - s), j = 0; j <= k - s; ++j, sh -= 2) {            // s-mer j: bases j .. j + s - 1, sh = 2 (k - s - j)
      uint64_t x = sh >= 64 ? (w1 >> (sh - 64)) : sh ? ((w0 >> sh) | (w1 << (64 - sh))) : w0;
      x &= smask;
      const uint64_t h = kh_hash64<HASH>(CANON ? kh_xf(x, s) : x, seed);
      if (j == 0) first = h;
      last = h;
      m = h < m ? h : m;
    }
    out[i] = (first == m || last == m) ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------
// canonical slot order.  A Robin Hood table keeps its elements sorted by home bucket, but the order of the keys that SHARE a home bucket
// is whatever the insert made of it (in the reference: arrival order; in the counting insert here: the order LDS atomics gave, which
// differs from run to run).  The index promises a result that depends on the multiset of pairs only, so every run of slots with one
// home bucket is sorted by key, in place: the lane that owns the first slot of a run walks it (a run is shorter than 128 slots, nearly
// always 1 or 2) and selection-sorts (key, value); the info bytes are positional and stay.  Runs are disjoint: no two lanes touch a slot.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ki_in_run(const KhSlot* __restrict__ slots, uint64_t j, uint64_t mask, uint64_t home) {
  const uint32_t b = slots[j].info & 0xFFu;
  return b >= 0x80u && ((j - (b & 0x7Fu)) & mask) == home;
}
__global__ __launch_bounds__(256) void k_index_canon_runs(KhSlot* __restrict__ slots, uint64_t cap) {
  const uint64_t mask = cap - 1, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += stride) {
    const uint32_t b = slots[i].info & 0xFFu;
    if (b < 0x80u) continue;
    const uint64_t home = (i - (b & 0x7Fu)) & mask;
    if (ki_in_run(slots, (i - 1) & mask, mask, home)) continue;          // not the first slot of its run
    uint32_t len = 1;
    while (len < 128u && len < cap && ki_in_run(slots, (i + len) & mask, mask, home)) ++len;
    for (uint32_t a = 0; a + 1 < len; ++a) {
      KhSlot* sa = slots + ((i + a) & mask);
      uint64_t kmin = sa->key; uint32_t at = a;
      for (uint32_t c = a + 1; c < len; ++c) { const uint64_t kc = slots[(i + c) & mask].key; if (kc < kmin) { kmin = kc; at = c; } }
      if (at != a) {
        KhSlot* sm = slots + ((i + at) & mask);
        const uint64_t ka = sa->key; const uint32_t va = sa->val, vm = sm->val;
        sa->key = kmin; sa->val = vm; sm->key = ka; sm->val = va;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// rank pass over a Robin Hood table after the counting insert, on the tiling of k_values_tile_count / k_values_tile_emit (the tile
// sums come from k_values_tile_count<KV_RH> over the full value range): live slot -> rank r in slot order; counts[r] = the slot's
// value (the occurrences of its key), and the value becomes r.  Every slot belongs to one lane: plain stores.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KV_SEL_THREADS) void k_index_rank(KhSlot* __restrict__ slots, uint64_t cap, const uint64_t* __restrict__ tile_off,
                                                               uint32_t* __restrict__ counts) {
  __shared__ uint32_t wcnt[KV_SEL_ROWS * (KV_SEL_THREADS / 64)];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t tbase = (uint64_t)blockIdx.x * KV_SEL_TILE;
  KvItem it[KV_SEL_ROWS];
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + tid;
    it[j] = kv_ld<KV_RH>(slots, i < cap ? i : cap - 1);
  }
  uint32_t hit = 0, rank[KV_SEL_ROWS];
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + tid;
    const bool m = i < cap && kv_live<KV_RH>(it[j].info);
    const unsigned long long b = __ballot(m);
    rank[j] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[j * (KV_SEL_THREADS / 64) + wid] = (uint32_t)__popcll(b);
    hit |= m ? (1u << j) : 0u;
  }
  __syncthreads();
  const uint64_t obase = tile_off[blockIdx.x];
  uint32_t acc = 0;
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    uint32_t pre = 0;
#pragma unroll
    for (uint32_t w = 0; w < KV_SEL_THREADS / 64; ++w) { if (w == wid) pre = acc; acc += wcnt[j * (KV_SEL_THREADS / 64) + w]; }
    if ((hit >> j) & 1u) {
      const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + tid;
      const uint32_t r = (uint32_t)(obase + pre + rank[j]);
      counts[r] = it[j].val;
      slots[i].val = r;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// exclusive scan of n u32 counts into n + 1 offsets (u32: the CSR of the index; u64: the CSR of a query batch, whose total may pass
// 2^32), over any number of workgroups: tile sums (u64), one workgroup scans them in place, every tile scans itself again on top.
// ---------------------------------------------------------------------------------------------
#define KI_SCAN_THREADS 256
#define KI_SCAN_ITEMS 8
#define KI_SCAN_TILE (KI_SCAN_THREADS * KI_SCAN_ITEMS)
__device__ __forceinline__ unsigned long long ki_wave_incl(unsigned long long x, uint32_t lane) {
  for (int off = 1; off < 64; off <<= 1) { const unsigned long long o = __shfl_up(x, off, 64); if (lane >= (uint32_t)off) x += o; }
  return x;
}
__global__ __launch_bounds__(KI_SCAN_THREADS) void k_index_tile_sums(const uint32_t* __restrict__ in, uint64_t n, unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long wsum[KI_SCAN_THREADS / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint64_t i0 = (uint64_t)blockIdx.x * KI_SCAN_TILE + (uint64_t)tid * KI_SCAN_ITEMS;
  unsigned long long c = 0;
#pragma unroll
  for (int j = 0; j < KI_SCAN_ITEMS; ++j) c += i0 + j < n ? in[i0 + j] : 0u;
  c = ki_wave_incl(c, lane);
  if (lane == 63) wsum[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) { unsigned long long t = 0; for (uint32_t w = 0; w < KI_SCAN_THREADS / 64; ++w) t += wsum[w]; sums[blockIdx.x] = t; }
}
#define KI_SUMS_THREADS 512
// in place: sums[i] = sum of the entries before i, sums[nt] = the total
__global__ __launch_bounds__(KI_SUMS_THREADS) void k_index_scan_sums(unsigned long long* __restrict__ sums, uint64_t nt) {
  __shared__ unsigned long long wsum[KI_SUMS_THREADS / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  unsigned long long carry = 0;                                 // (workgroup-uniform)
  for (uint64_t base = 0; base < nt; base += KI_SUMS_THREADS) {
    const uint64_t i = base + tid;
    const unsigned long long v = i < nt ? sums[i] : 0ull;
    const unsigned long long incl = ki_wave_incl(v, lane);
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    unsigned long long pre = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < KI_SUMS_THREADS / 64; ++w) { const unsigned long long x = wsum[w]; if (w < wid) pre += x; tot += x; }
    if (i < nt) sums[i] = carry + pre + incl - v;
    carry += tot;
    __syncthreads();
  }
  if (tid == 0) sums[nt] = carry;
}
template <typename OUT>
__global__ __launch_bounds__(KI_SCAN_THREADS) void k_index_scan_apply(const uint32_t* __restrict__ in, uint64_t n, const unsigned long long* __restrict__ tile_off,
                                                                      OUT* __restrict__ out /* n + 1 */) {
  __shared__ unsigned long long wsum[KI_SCAN_THREADS / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t i0 = (uint64_t)blockIdx.x * KI_SCAN_TILE + (uint64_t)tid * KI_SCAN_ITEMS;
  uint32_t v[KI_SCAN_ITEMS];
  unsigned long long c = 0;
#pragma unroll
  for (int j = 0; j < KI_SCAN_ITEMS; ++j) { v[j] = i0 + j < n ? in[i0 + j] : 0u; c += v[j]; }
  const unsigned long long incl = ki_wave_incl(c, lane);
  if (lane == 63) wsum[wid] = incl;
  __syncthreads();
  unsigned long long ex = tile_off[blockIdx.x] + incl - c;
#pragma unroll
  for (uint32_t w = 0; w < KI_SCAN_THREADS / 64; ++w) if (w < wid) ex += wsum[w];
#pragma unroll
  for (int j = 0; j < KI_SCAN_ITEMS; ++j) { if (i0 + j < n) out[i0 + j] = (OUT)ex; ex += v[j]; }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) out[n] = (OUT)tile_off[gridDim.x];
}

// ---------------------------------------------------------------------------------------------
// scatter: every (key, pos) pair probes the table for its key's rank (kh_probe_items: four pairs per lane in flight, a 64-byte sector
// per round trip), takes the next place of that key's segment from its cursor (initialised from offsets) and writes the position
// there.  A hot k-mer makes the cursor atomic same-address; the order inside a segment is whatever the atomics gave and is restored
// by the two sort kernels below.
// ---------------------------------------------------------------------------------------------
#define KI_Q_TILE (KH_Q_THREADS * KH_Q_ITEMS)
template <int HASH>
__global__ __launch_bounds__(KH_Q_THREADS) void k_index_scatter(KhSlots T, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ pos, uint64_t n, KhSeed seed,
                                                                uint32_t* __restrict__ cursor, uint32_t* __restrict__ positions, uint64_t total) {
  for (uint64_t base = (uint64_t)blockIdx.x * KI_Q_TILE; base < n; base += (uint64_t)gridDim.x * KI_Q_TILE) {
    uint64_t key[KH_Q_ITEMS]; uint32_t r[KH_Q_ITEMS], p[KH_Q_ITEMS];
    uint32_t valid = 0;
#pragma unroll
    for (int j = 0; j < KH_Q_ITEMS; ++j) {
      const uint64_t i = base + (uint64_t)j * KH_Q_THREADS + threadIdx.x;
      key[j] = 0; r[j] = 0; p[j] = 0;
      if (i < n) { key[j] = keys[i]; p[j] = pos[i]; valid |= 1u << j; }
    }
    const uint32_t hit = kh_probe_items<KHK_RH, HASH, false>(T, key, valid, seed, r);
#pragma unroll
    for (int j = 0; j < KH_Q_ITEMS; ++j) {
      if ((hit >> j) & 1u) {
        const uint32_t dst = atomicAdd(&cursor[r[j]], 1u);
        if (dst < total) positions[dst] = p[j];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// tile sort: positions cut into fixed tiles of KI_SORT_TILE entries, a workgroup per tile.  The segment boundaries inside the tile come
// from offsets (head flags in LDS, a workgroup scan turns them into the segment index within the tile); the tile is loaded coalesced as
// (segment in tile << 32) | position, sorted with a bitonic network in LDS and written back: every segment that lies wholly inside a
// tile is sorted afterwards, with the same work whatever the segment lengths.  The segment that runs into the tile from the one before
// it crosses a tile boundary; the tile behind the FIRST boundary a segment crosses appends it to xlist (so each crossing segment, and
// with it every segment longer than a tile, is listed once) for k_index_seg_radix.
// ---------------------------------------------------------------------------------------------
#define KI_SORT_TILE 4096
#define KI_SORT_THREADS 512
#define KI_SORT_PER (KI_SORT_TILE / KI_SORT_THREADS)
__global__ __launch_bounds__(KI_SORT_THREADS) void k_index_tile_sort(uint32_t* __restrict__ positions, uint64_t total, const uint32_t* __restrict__ offsets, uint64_t nseg,
                                                                     uint32_t* __restrict__ xlist, uint32_t* __restrict__ xcount) {
  __shared__ uint64_t skey[KI_SORT_TILE];
  __shared__ uint32_t sseg[KI_SORT_TILE];
  __shared__ uint32_t wsum[KI_SORT_THREADS / 64];
  __shared__ uint64_t s_first;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t tile0 = (uint64_t)blockIdx.x * KI_SORT_TILE;
  const uint32_t m = (uint32_t)(total - tile0 < KI_SORT_TILE ? total - tile0 : KI_SORT_TILE);
  if (tid == 0) {
    uint64_t lo = 0, hi = nseg;                      // the last segment that starts at or before the tile's first entry
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (offsets[mid] <= tile0) lo = mid; else hi = mid; }
    s_first = lo;
    const uint64_t o = offsets[lo];
    if (o < tile0 && o + KI_SORT_TILE >= tile0) xlist[atomicAdd(xcount, 1u)] = (uint32_t)lo;
  }
  for (uint32_t i = tid; i < KI_SORT_TILE; i += KI_SORT_THREADS) sseg[i] = 0;
  __syncthreads();
  for (uint64_t s = s_first + 1 + tid; s < nseg; s += KI_SORT_THREADS) {      // (offsets ascend strictly: every key occurs at least once)
    const uint64_t o = offsets[s];
    if (o >= tile0 + m) break;
    sseg[o - tile0] = 1;
  }
  __syncthreads();
  uint32_t f[KI_SORT_PER], c = 0;
#pragma unroll
  for (int j = 0; j < KI_SORT_PER; ++j) { c += sseg[tid * KI_SORT_PER + j]; f[j] = c; }
  uint32_t incl = c;
  for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); if (lane >= (uint32_t)off) incl += o; }
  if (lane == 63) wsum[wid] = incl;
  __syncthreads();
  uint32_t pre = incl - c, heads = 0;
#pragma unroll
  for (uint32_t w = 0; w < KI_SORT_THREADS / 64; ++w) { const uint32_t x = wsum[w]; if (w < wid) pre += x; heads += x; }
  if (heads + 1 >= m) return;                      // (workgroup-uniform) a head at every entry but the first: no piece of a segment in this tile
                                                   // has two entries, there is nothing to order -- every tile of a text without repeats
#pragma unroll
  for (int j = 0; j < KI_SORT_PER; ++j) sseg[tid * KI_SORT_PER + j] = pre + f[j];
  __syncthreads();
  for (uint32_t i = tid; i < KI_SORT_TILE; i += KI_SORT_THREADS)
    skey[i] = i < m ? (((uint64_t)sseg[i] << 32) | positions[tile0 + i]) : ~0ull;
  __syncthreads();
  for (uint32_t k = 2; k <= KI_SORT_TILE; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t p = tid; p < KI_SORT_TILE / 2; p += KI_SORT_THREADS) {
        const uint32_t i = 2 * p - (p & (j - 1)), l = i + j;
        const uint64_t a = skey[i], b = skey[l];
        if ((a > b) == ((i & k) == 0)) { skey[i] = b; skey[l] = a; }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = tid; i < m; i += KI_SORT_THREADS) positions[tile0 + i] = (uint32_t)skey[i];
}

// ---------------------------------------------------------------------------------------------
// the listed segments, one workgroup each: a stable LSD radix sort of the 32-bit positions, 8 bits per pass, ping-pong between the
// segment's place in positions and the same place in scratch (u32[total]).  A pass: digit histogram in LDS, exclusive scan of the 256
// bins, then the segment in chunks of one entry per lane, in order -- a lane's place is bin start + same-digit entries of the waves
// before it in the chunk + same-digit lanes before it in its wave (eight ballots).  A pass whose digit is the same for the whole
// segment (the high bytes of positions in a short text) is skipped.
// ---------------------------------------------------------------------------------------------
#define KI_RADIX_THREADS 512
#define KI_RADIX_WAVES (KI_RADIX_THREADS / 64)
__global__ __launch_bounds__(KI_RADIX_THREADS) void k_index_seg_radix(uint32_t* __restrict__ positions, uint32_t* __restrict__ scratch, const uint32_t* __restrict__ offsets,
                                                                      const uint32_t* __restrict__ xlist, const uint32_t* __restrict__ xcount) {
  __shared__ uint32_t bin[256];
  __shared__ uint32_t wcnt[KI_RADIX_WAVES][256];
  __shared__ uint32_t wtot[4];
  __shared__ uint32_t s_same;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t nlist = *xcount;
  for (uint32_t e = blockIdx.x; e < nlist; e += gridDim.x) {
    const uint32_t s = xlist[e];
    const uint32_t b = offsets[s], len = offsets[s + 1] - b;
    uint32_t* src = positions + b;
    uint32_t* dst = scratch + b;
    for (uint32_t shift = 0; shift < 32; shift += 8) {
      if (tid < 256) bin[tid] = 0;
      for (uint32_t w = 0; w < KI_RADIX_WAVES; ++w) if (tid < 256) wcnt[w][tid] = 0;
      if (tid == 0) s_same = 0;
      __syncthreads();
      for (uint32_t i = tid; i < len; i += KI_RADIX_THREADS) atomicAdd(&bin[(src[i] >> shift) & 255u], 1u);
      __syncthreads();
      uint32_t v = 0, incl = 0;
      if (tid < 256) {
        v = bin[tid];
        if (v == len) s_same = 1;
        incl = v;
        for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); if (lane >= (uint32_t)off) incl += o; }
        if (lane == 63) wtot[wid] = incl;
      }
      __syncthreads();
      const bool same = s_same != 0;
      if (tid < 256) {
        uint32_t ex = incl - v;
        for (uint32_t w = 0; w < 4; ++w) if (w < wid) ex += wtot[w];
        bin[tid] = ex;
      }
      __syncthreads();
      if (same) continue;                                        // (workgroup-uniform)
      for (uint32_t c0 = 0; c0 < len; c0 += KI_RADIX_THREADS) {
        const uint32_t i = c0 + tid;
        const bool valid = i < len;
        const uint32_t x = valid ? src[i] : 0u;
        const uint32_t d = (x >> shift) & 255u;
        unsigned long long mask = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
          const bool on = (d >> bit) & 1u;
          const unsigned long long bb = __ballot(on);
          mask &= on ? bb : ~bb;
        }
        const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wcnt[wid][d] = (uint32_t)__popcll(mask);
        __syncthreads();
        if (valid) {
          uint32_t pre = 0;
#pragma unroll
          for (uint32_t w = 0; w < KI_RADIX_WAVES; ++w) if (w < wid) pre += wcnt[w][d];
          dst[bin[d] + pre + rank] = x;
        }
        __syncthreads();
        if (tid < 256) {
          uint32_t t = 0;
#pragma unroll
          for (uint32_t w = 0; w < KI_RADIX_WAVES; ++w) { t += wcnt[w][tid]; wcnt[w][tid] = 0; }
          bin[tid] += t;
        }
        __syncthreads();
      }
      uint32_t* sw = src; src = dst; dst = sw;
    }
    if (src != positions + b)
      for (uint32_t i = tid; i < len; i += KI_RADIX_THREADS) positions[b + i] = src[i];
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// lookup: (begin, count) of every query key -- one probe (the slot's value is the rank) and two adjacent offsets words; a miss is (0, 0).
// ---------------------------------------------------------------------------------------------
template <int HASH>
__global__ __launch_bounds__(KH_Q_THREADS) void k_index_lookup(KhSlots T, const uint64_t* __restrict__ q, uint64_t n, KhSeed seed, const uint32_t* __restrict__ offsets,
                                                               uint32_t* __restrict__ out_begin /* or null */, uint32_t* __restrict__ out_count) {
  for (uint64_t base = (uint64_t)blockIdx.x * KI_Q_TILE; base < n; base += (uint64_t)gridDim.x * KI_Q_TILE) {
    uint64_t key[KH_Q_ITEMS]; uint32_t r[KH_Q_ITEMS];
    uint32_t valid = 0;
#pragma unroll
    for (int j = 0; j < KH_Q_ITEMS; ++j) {
      const uint64_t i = base + (uint64_t)j * KH_Q_THREADS + threadIdx.x;
      key[j] = 0; r[j] = 0;
      if (i < n) { key[j] = q[i]; valid |= 1u << j; }
    }
    const uint32_t hit = kh_probe_items<KHK_RH, HASH, false>(T, key, valid, seed, r);
#pragma unroll
    for (int j = 0; j < KH_Q_ITEMS; ++j) {
      const uint64_t i = base + (uint64_t)j * KH_Q_THREADS + threadIdx.x;
      if ((valid >> j) & 1u) {
        uint32_t b = 0, c = 0;
        if ((hit >> j) & 1u) { b = offsets[r[j]]; c = offsets[r[j] + 1] - b; }
        if (out_begin) out_begin[i] = b;
        out_count[i] = c;
      }
    }
  }
}
// gather balanced over OUTPUT elements: output j finds its query by binary search in the query CSR (the last query whose offset is
// <= j: queries without hits share their offset with the next one and are passed over) and copies one position.  A query with 10^6
// hits is 10^6 independent lanes.
__global__ __launch_bounds__(256) void k_index_gather(const uint32_t* __restrict__ positions, const uint32_t* __restrict__ begin, const uint64_t* __restrict__ qoff,
                                                      uint64_t nq, uint64_t total, uint32_t* __restrict__ out) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride) {
    uint64_t lo = 0, hi = nq;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (qoff[mid] <= j) lo = mid; else hi = mid; }
    out[j] = positions[(uint64_t)begin[lo] + (j - qoff[lo])];
  }
}

// ---------------------------------------------------------------------------------------------
// mutation of a built index (kh_index_append* / kh_index_erase / kh_index_erase_counts, both key widths): the CSR is carried across a
// change of the key set.  The slot's value is the link -- it travels with its key through every insert, erase and re-layout of the
// table.  Append: k_index_stamp (value = old rank + 1) -> the table's own reducer insert with zero values (old keys keep the stamp, new
// keys read 0) -> canonical runs -> k_index_rank_carry (new rank into the slot, oldrank[new rank], counts[new rank] = length of the old
// segment) -> k_index_count_pairs (+1 per pair of the batch) -> scan -> k_index_move (old segments to the front of the new ones,
// cursors behind them) -> the build's scatter and sorts.  Erase: the table's own erase (the survivors keep their rank: no stamp) ->
// canonical runs -> k_index_rank_carry -> scan -> k_index_move.  The kernels that only read value and info are templates over the slot
// layout (KV_RH / KV_WIDE) and serve both widths; the probe of the batch has a sibling in kh_kernels_index_wide.h.
// ---------------------------------------------------------------------------------------------
#define KI_NEW_KEY 0xFFFFFFFFu
template <int LAY>
__global__ __launch_bounds__(KV_MARK_THREADS) void k_index_stamp(void* __restrict__ slots, uint64_t cap) {
  typedef typename KvSlot<LAY>::type Slot;
  Slot* S = static_cast<Slot*>(slots);
  const uint64_t span = (uint64_t)gridDim.x * KV_MARK_THREADS;
  for (uint64_t i0 = (uint64_t)blockIdx.x * KV_MARK_THREADS; i0 < cap; i0 += span * KV_MARK_ITEMS) {
    KvItem it[KV_MARK_ITEMS];
#pragma unroll
    for (int j = 0; j < KV_MARK_ITEMS; ++j) {
      const uint64_t i = i0 + (uint64_t)j * span + threadIdx.x;
      it[j] = kv_ld<LAY>(slots, i < cap ? i : cap - 1);
    }
#pragma unroll
    for (int j = 0; j < KV_MARK_ITEMS; ++j) {
      const uint64_t i = i0 + (uint64_t)j * span + threadIdx.x;
      if (i < cap && kv_live<LAY>(it[j].info)) S[i].val = it[j].val + 1u;          // (size < 2^32: rank + 1 fits)
    }
  }
}
// k_index_rank on either layout, for a table whose live values are old rank + bias (bias 1: stamped, 0 is a key the batch brought;
// bias 0: every key is an old one).  Nothing is assumed about the slot order of the survivors: a run that wrapped past the last slot can
// unwrap, keys of one home bucket change places -- the old rank is read from the slot, not counted.
template <int LAY>
__global__ __launch_bounds__(KV_SEL_THREADS) void k_index_rank_carry(void* __restrict__ slots, uint64_t cap, const uint64_t* __restrict__ tile_off,
                                                                     const uint32_t* __restrict__ old_off, uint64_t old_size, uint32_t bias, uint64_t new_size,
                                                                     uint32_t* __restrict__ counts, uint32_t* __restrict__ oldrank) {
  __shared__ uint32_t wcnt[KV_SEL_ROWS * (KV_SEL_THREADS / 64)];
  typedef typename KvSlot<LAY>::type Slot;
  Slot* S = static_cast<Slot*>(slots);
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t tbase = (uint64_t)blockIdx.x * KV_SEL_TILE;
  KvItem it[KV_SEL_ROWS];
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + tid;
    it[j] = kv_ld<LAY>(slots, i < cap ? i : cap - 1);
  }
  uint32_t hit = 0, rank[KV_SEL_ROWS];
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + tid;
    const bool m = i < cap && kv_live<LAY>(it[j].info);
    const unsigned long long b = __ballot(m);
    rank[j] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[j * (KV_SEL_THREADS / 64) + wid] = (uint32_t)__popcll(b);
    hit |= m ? (1u << j) : 0u;
  }
  __syncthreads();
  const uint64_t obase = tile_off[blockIdx.x];
  uint32_t acc = 0;
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    uint32_t pre = 0;
#pragma unroll
    for (uint32_t w = 0; w < KV_SEL_THREADS / 64; ++w) { if (w == wid) pre = acc; acc += wcnt[j * (KV_SEL_THREADS / 64) + w]; }
    if ((hit >> j) & 1u) {
      const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + tid;
      const uint64_t r = obase + pre + rank[j];
      const uint32_t v = it[j].val;
      uint32_t orank = KI_NEW_KEY, len = 0;
      if (v >= bias && (uint64_t)(v - bias) < old_size) { orank = v - bias; len = old_off[orank + 1] - old_off[orank]; }
      if (r < new_size) { counts[r] = len; oldrank[r] = orank; }
      S[i].val = (uint32_t)r;
    }
  }
}
// the batch counted onto the seeded counts: the probe of k_index_scatter, one atomic per pair
template <int HASH>
__global__ __launch_bounds__(KH_Q_THREADS) void k_index_count_pairs(KhSlots T, const uint64_t* __restrict__ keys, uint64_t n, KhSeed seed, uint32_t* __restrict__ counts,
                                                                    uint64_t nranks) {
  for (uint64_t base = (uint64_t)blockIdx.x * KI_Q_TILE; base < n; base += (uint64_t)gridDim.x * KI_Q_TILE) {
    uint64_t key[KH_Q_ITEMS]; uint32_t r[KH_Q_ITEMS];
    uint32_t valid = 0;
#pragma unroll
    for (int j = 0; j < KH_Q_ITEMS; ++j) {
      const uint64_t i = base + (uint64_t)j * KH_Q_THREADS + threadIdx.x;
      key[j] = 0; r[j] = 0;
      if (i < n) { key[j] = keys[i]; valid |= 1u << j; }
    }
    const uint32_t hit = kh_probe_items<KHK_RH, HASH, false>(T, key, valid, seed, r);
#pragma unroll
    for (int j = 0; j < KH_Q_ITEMS; ++j)
      if (((hit >> j) & 1u) && r[j] < nranks) atomicAdd(&counts[r[j]], 1u);
  }
}
// old segments into the new positions array, balanced over OUTPUT elements as k_index_gather is: output j finds its new segment by
// binary search in the new offsets (they ascend strictly: every key of the index occurs at least once) and, while it lies in the part
// the old segment fills, copies one position; a segment of 10^6 entries is 10^6 independent lanes.  The lane at the head of a segment
// sets the cursor the scatter continues from (cursor == null: an erase, nothing follows).
__global__ __launch_bounds__(256) void k_index_move(const uint32_t* __restrict__ old_pos, const uint32_t* __restrict__ old_off, uint64_t old_size, uint64_t old_total,
                                                    const uint32_t* __restrict__ new_off, const uint32_t* __restrict__ oldrank, uint64_t new_size, uint64_t new_total,
                                                    uint32_t* __restrict__ new_pos, uint32_t* __restrict__ cursor /* or null */) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < new_total; j += stride) {
    uint64_t lo = 0, hi = new_size;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (new_off[mid] <= j) lo = mid; else hi = mid; }
    const uint64_t w = j - new_off[lo];
    const uint32_t orank = oldrank[lo];
    uint32_t ob = 0, olen = 0;
    if (orank < old_size) { ob = old_off[orank]; olen = old_off[orank + 1] - ob; }
    if (w == 0 && cursor) cursor[lo] = new_off[lo] + olen;
    if (w < olen && (uint64_t)ob + w < old_total) new_pos[j] = old_pos[(uint64_t)ob + w];
  }
}
// window positions of an appended text into the caller's coordinate space
__global__ __launch_bounds__(256) void k_index_add_base(uint32_t* __restrict__ pos, uint64_t n, uint32_t base) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) pos[i] += base;
}
// ---------------------------------------------------------------------------------------------
// strand of a window position (kh_stamp_strand, a stranded index): rc(p) = 1 iff the reverse complement of the k bases at p is
// strictly smaller than the window -- the case in which the canonical front ends emit the reverse complement.  One lane per position.
// Base i of the reverse complement is 3 - code(text[p + k - 1 - i]); the first i at which it differs from code(text[p + i]) decides,
// and the pairs i >= ceil(k / 2) are the mirror images of the ones before: equal throughout the first half is a palindrome (rc = 0;
// an odd k has none: its middle base differs from its own complement).  out[i] = ((pos_base + p) << 1) | rc, or KH_POS_INVALID.
// CHECK: the public call -- p + k <= n and all k bytes are bases (the loop then runs its full length: both ends of every pair are
// tested, which covers the window), invalid windows counted into *n_invalid (one atomic per wave).  !CHECK: positions a front end
// emitted; the loop ends at the first difference, after 4/3 steps on average on random text.  The bound is tested in either form: no
// byte outside [text, text + n) is read whatever pos holds.  pos and out may be the same array (one lane reads and writes entry i).
// ---------------------------------------------------------------------------------------------
#define KI_POS_INVALID 0xFFFFFFFFu
template <bool CHECK>
__global__ __launch_bounds__(256) void k_pos_strand(const uint8_t* __restrict__ text, uint64_t n, uint32_t k, const uint32_t* pos, uint64_t m, uint32_t pos_base,
                                                    uint32_t* out, unsigned long long* __restrict__ n_invalid /* or null */) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint32_t half = (k + 1) >> 1;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
    const uint64_t p = pos[i];
    bool ok = p + k <= n;
    uint32_t rc = 0;
    if (ok) {
      const uint8_t* __restrict__ w = text + p;
      bool open = true;
      for (uint32_t j = 0; j < half; ++j) {
        const uint32_t a = kh_dna_code(w[j]), b = kh_dna_code(w[k - 1 - j]);
        if (CHECK && (a | b) > 3u) { ok = false; break; }
        if (open && a != 3u - b) {
          rc = 3u - b < a ? 1u : 0u;
          open = false;
          if (!CHECK) break;
        }
      }
    }
    out[i] = ok ? ((pos_base + (uint32_t)p) << 1) | rc : KI_POS_INVALID;
    if (CHECK && n_invalid) {
      const unsigned long long bad = __ballot(!ok);
      if (bad && (unsigned)__builtin_ctzll(bad) == (threadIdx.x & 63u)) atomicAdd(n_invalid, (unsigned long long)__popcll(bad));
    }
  }
}
// a CSR of hits (kh_index_find over stamped query positions) into the flat anchor list a chainer consumes, balanced over OUTPUT elements
// as k_index_gather is: output j finds its row by binary search over offsets (the last row that begins at or before j: empty rows share
// their offset with the row behind them and are passed over) and writes (query position, reference position, relative strand).
__global__ __launch_bounds__(256) void k_anchors_expand(const uint32_t* __restrict__ qpos, const uint64_t* __restrict__ offsets, uint64_t n,
                                                        const uint32_t* __restrict__ pos, uint64_t total, uint32_t* __restrict__ out_qpos,
                                                        uint32_t* __restrict__ out_rpos, uint8_t* __restrict__ out_rev) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += stride) {
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (offsets[mid] <= j) lo = mid; else hi = mid; }
    const uint32_t q = qpos[lo], r = pos[j];
    out_qpos[j] = q >> 1;
    out_rpos[j] = r >> 1;
    out_rev[j] = (uint8_t)((q ^ r) & 1u);
  }
}
// erase by occurrence count: k_values_tile_count / k_values_tile_emit with the predicate on the LENGTH OF THE KEY'S SEGMENT
// (offsets[rank + 1] - offsets[rank], the rank being the slot's value) instead of on the value, keys only.  Ranks follow the slot
// order, so the two offsets words of a wave's slots are neighbours.
template <int LAY>
__device__ __forceinline__ bool ki_len_match(const KvItem& it, const uint32_t* __restrict__ offsets, uint64_t size, uint32_t lo, uint32_t hi) {
  if (!kv_live<LAY>(it.info) || it.val >= size) return false;
  const uint32_t len = offsets[it.val + 1] - offsets[it.val];
  return len >= lo && len <= hi;
}
template <int LAY>
__global__ __launch_bounds__(KV_SEL_THREADS) void k_index_len_count(const void* __restrict__ slots, uint64_t cap, const uint32_t* __restrict__ offsets, uint64_t size,
                                                                    uint32_t lo, uint32_t hi, uint32_t* __restrict__ sums) {
  __shared__ uint32_t wsum[KV_SEL_THREADS / 64];
  const uint64_t tbase = (uint64_t)blockIdx.x * KV_SEL_TILE;
  KvItem it[KV_SEL_ROWS];
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + threadIdx.x;
    it[j] = kv_ld<LAY>(slots, i < cap ? i : cap - 1);
  }
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + threadIdx.x;
    c += (i < cap && ki_len_match<LAY>(it[j], offsets, size, lo, hi)) ? 1u : 0u;
  }
  c = kh_wave_sum(c);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (uint32_t w = 0; w < KV_SEL_THREADS / 64; ++w) tot += wsum[w];
    sums[blockIdx.x] = tot;
  }
}
template <int LAY>
__global__ __launch_bounds__(KV_SEL_THREADS) void k_index_len_emit(const void* __restrict__ slots, uint64_t cap, const uint32_t* __restrict__ offsets, uint64_t size,
                                                                   uint32_t lo, uint32_t hi, const uint64_t* __restrict__ tile_off, uint64_t* __restrict__ out_keys,
                                                                   uint64_t cap_out) {
  __shared__ uint32_t wcnt[KV_SEL_ROWS * (KV_SEL_THREADS / 64)];
  typedef typename KvSlot<LAY>::type Slot;
  const Slot* S = static_cast<const Slot*>(slots);
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t tbase = (uint64_t)blockIdx.x * KV_SEL_TILE;
  KvItem it[KV_SEL_ROWS];
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + tid;
    it[j] = kv_ld<LAY>(slots, i < cap ? i : cap - 1);
  }
  uint32_t hit = 0, rank[KV_SEL_ROWS];
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + tid;
    const bool m = i < cap && ki_len_match<LAY>(it[j], offsets, size, lo, hi);
    const unsigned long long b = __ballot(m);
    rank[j] = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[j * (KV_SEL_THREADS / 64) + wid] = (uint32_t)__popcll(b);
    hit |= m ? (1u << j) : 0u;
  }
  __syncthreads();
  const uint64_t obase = tile_off[blockIdx.x];
  uint32_t acc = 0;
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    uint32_t pre = 0;
#pragma unroll
    for (uint32_t w = 0; w < KV_SEL_THREADS / 64; ++w) { if (w == wid) pre = acc; acc += wcnt[j * (KV_SEL_THREADS / 64) + w]; }
    if ((hit >> j) & 1u) {
      const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + tid;
      const uint64_t x = obase + pre + rank[j];
      if (x >= cap_out) continue;
      if (LAY == KV_WIDE) {
        const uint4 k = *reinterpret_cast<const uint4*>(S + i);
        out_keys[2 * x] = (uint64_t)k.x | ((uint64_t)k.y << 32);
        out_keys[2 * x + 1] = (uint64_t)k.z | ((uint64_t)k.w << 32);
      } else {
        out_keys[x] = *reinterpret_cast<const uint64_t*>(S + i);
      }
    }
  }
}
