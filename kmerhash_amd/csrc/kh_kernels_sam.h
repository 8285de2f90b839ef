// kh_kernels_sam.h -- gfx950 device code of kh_record_diffs and kh_oriented_rows, included once by kmerhash_amd.hip after
// kh_kernels_records.h.  Prefixes k_diffs_ and k_orient_.
//
// kh_record_diffs walks a record row (the runs of kh_chain_records in reference order) along the two texts and writes which bases its
// X, I and D runs were: the short cs string or the MD string of SAM (definition: include/kmerhash_amd.h, model: tests/diffs_model.py).
//   k_diffs_count<KIND>  one wavefront per row, fixed grid, grid-stride over the rows; 64 runs per step, one coalesced load.  Every lane
//                        sizes its own run: the read bases and the reference bases it consumes and the bytes it prints.  Three wave
//                        prefix sums (64-bit: a step can hold 64 runs of 2^28) give the lane its cursors j and r and its byte offset;
//                        the sums of a step are carried in vector registers (the walk has scalars enough).  A lane whose run is no
//                        S I D = X, leaves the read or leaves the reference text spoils the row for the wave (one ballot).  MD: the
//                        number in front of an X or D run
//                        is the sum of the '=' lengths since the X or D run before it -- a segmented sum: the exclusive prefix sum E of
//                        the '=' lengths, minus E of the nearest X / D lane below (a ballot and one lane read), or plus the count
//                        carried across steps where there is none.  No text is read: the byte count follows from the runs alone.
//                        Writes ok and the row's bytes
//   k_diffs_emit<KIND>   the same walk over the rows that are ok; a lane prints its run at the row's offset + its prefix sum, base by
//                        base from the texts (an X or D run is a few bases; a '=' run prints digits only), lane 0 the closing number
//                        of MD.  Every byte is written inside the row's own byte range and below the total the host passes in
// No atomics, no LDS: the lanes of a wave own disjoint byte ranges.
//
// kh_oriented_rows copies byte ranges of a text into a byte CSR, reverse-strand rows back to front and, for bases, complemented.
//   k_orient_len   one lane per row: its clamped length; the index's scan (k_index_tile_sums / _scan_sums / _scan_apply) makes offsets
//   k_orient_copy  one wavefront per row: the bytes up to the first 8-byte boundary of the DESTINATION and those behind the last go
//                  one per lane; between them every lane moves whole words -- an 8-byte load from the source wherever it lies, for a
//                  reversed row a byte swap and a SWAR complement (A<->T, C<->G, case kept, anything else itself), one aligned
//                  8-byte store
// Every index that comes out of memory (row bounds, the scanned offsets, lo / hi, rs) is range-checked or clamped before it addresses
// anything.
#pragma once
#include <type_traits>
#include "kh_kernels_records.h"

#define KDF_THREADS 256
#define KDF_WAVES (KDF_THREADS / 64)
#define KDF_CS 0u
#define KDF_MD 1u
#define KDF_I 1u
#define KDF_D 2u

struct KdfArgs {
  const uint8_t* qtext; const uint8_t* rtext;
  const uint64_t* off; const uint32_t* ops;
  const uint8_t* valid; const uint8_t* rev; const uint32_t* q_lo; const uint32_t* q_hi; const uint32_t* rs;
  uint64_t nq, nr, n_ops;
  uint32_t ref_base, n_rows;
};

// the code of a text byte: A/a 0, C/c 1, G/g 2, T/t 3, anything else 4 (kh_chain_edits)
__device__ __forceinline__ uint32_t kdf_code(uint32_t b) {
  const uint32_t u = b & 0xdfu;
  return u == 0x41u ? 0u : u == 0x43u ? 1u : u == 0x47u ? 2u : u == 0x54u ? 3u : 4u;
}
// "acgtn"[c] and "ACGTN"[c], c = 0..4
__device__ __forceinline__ uint8_t kdf_lower(uint32_t c) { return (uint8_t)(0x6e74676361ull >> (8u * c)); }
__device__ __forceinline__ uint8_t kdf_upper(uint32_t c) { return (uint8_t)(0x4e54474341ull >> (8u * c)); }
// decimal digits of a u32 (1..10)
__device__ __forceinline__ uint32_t kdf_digits(uint32_t v) {
  return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
         (v >= 1000000000u);
}
__device__ __forceinline__ uint64_t kdf_uniform64(uint64_t v) {
  return ((uint64_t)krc_uniform((uint32_t)(v >> 32)) << 32) | krc_uniform((uint32_t)v);
}
// exclusive wave prefix sums; total = the sum over the wave, the same in every lane (kept in vector registers: the walk has scalars
// enough)
__device__ __forceinline__ uint64_t kdf_scan(uint64_t v, uint32_t lane, uint64_t& total) {
  uint64_t incl = v;
  for (int d = 1; d < 64; d <<= 1) { const uint64_t t = (uint64_t)__shfl_up((unsigned long long)incl, d); if (lane >= (uint32_t)d) incl += t; }
  total = (uint64_t)__shfl((unsigned long long)incl, 63);
  return incl - v;
}
__device__ __forceinline__ uint32_t kdf_scan(uint32_t v, uint32_t lane, uint32_t& total) {
  uint32_t incl = v;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, d); if (lane >= (uint32_t)d) incl += t; }
  total = (uint32_t)__shfl((int)incl, 63);
  return incl - v;
}

// the output of one row: bytes [0, n) at p; a byte beyond n is dropped
struct KdfOut {
  uint8_t* p; uint32_t n;
  __device__ __forceinline__ void put(uint32_t at, uint8_t b) const { if (at < n) p[at] = b; }
  // the nd digits of v at `at` (nd == 0: nothing).  Ten turns for every lane: a loop the wave does not diverge in
  __device__ __forceinline__ void number(uint32_t at, uint32_t v, uint32_t nd) const {
#pragma unroll 1
    for (uint32_t t = 0; t < 10u; ++t) { if (t < nd) put(at + (nd - 1u - t), (uint8_t)('0' + v % 10u)); v /= 10u; }
  }
};

// one row walked by one wave -> good; bytes = the length of its text.  The count pass (EMIT false) decides: its cursors are exact, 64
// bits wide, r in reference coordinates.  The emit pass walks rows the count pass found good, whose cursors and text fit 32 bits: its
// cursors are u32, r relative to ref_base, and every lane still checks the very values it addresses the texts with -- inputs that
// changed between the passes give a wrong text, never an access outside the arrays.  EMIT: the text goes to `out`
template <uint32_t KIND, bool EMIT>
__device__ __forceinline__ bool kdf_walk(const KdfArgs& P, uint32_t c, uint32_t lane, const KdfOut& out, uint64_t& bytes) {
  typedef typename std::conditional<EMIT, uint32_t, uint64_t>::type Cur;
  bytes = 0;
  if (!EMIT && !P.valid[c]) return false;           // (the emit pass is told by ok[])
  const uint64_t a = kdf_uniform64(min(P.off[c], P.n_ops)), b = kdf_uniform64(min(P.off[c + 1], P.n_ops));
  if (b <= a) return false;
  const uint32_t lo = P.q_lo[c], hi = P.q_hi[c], rv = krc_uniform(P.rev[c] & 1u);      // (lo, hi: the same in every lane, in vector registers)
  if (__ballot(lo > hi || (uint64_t)hi > P.nq)) return false;
  const uint32_t L = hi - lo, nrun = (uint32_t)(b - a);      // (n_ops <= 2^31)
  const uint64_t r_lo = EMIT ? 0ull : (uint64_t)P.ref_base, r_hi = r_lo + P.nr;
  Cur j = 0, r = EMIT ? (Cur)(krc_uniform(P.rs[c]) - P.ref_base) : (Cur)krc_uniform(P.rs[c]), at = 0;
  uint32_t n = 0;                                    // MD: the matches since the last X or D run, wrapping
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll 1
  for (uint32_t base = 0; base < nrun; base += 64u) {
    const uint32_t i = base + lane;
    const uint32_t v = i < nrun ? P.ops[a + i] : 0u, op = v & 15u, l = v >> 4;
    const bool live = l != 0u;
    const bool eq = live && op == KCG_EQ, x = live && op == KCG_X, ins = live && op == KDF_I, del = live && op == KDF_D, clip = live && op == KRC_S;
    const bool cq = eq || x || ins || clip, cr = eq || x || del;
    Cur tj, tr, tb;
    const Cur mj = j + kdf_scan((Cur)(cq ? l : 0u), lane, tj), mr = r + kdf_scan((Cur)(cr ? l : 0u), lane, tr);
    const bool bad = (live && !cq && !cr) || (cq && (uint64_t)mj + l > L) || (cr && ((uint64_t)mr < r_lo || (uint64_t)mr + l > r_hi));
    if (__ballot(bad)) return false;
    uint32_t nb, mn = 0, nd = 0;
    if (KIND == KDF_CS) {
      nd = kdf_digits(l);
      nb = eq ? 1u + nd : x ? 3u * l : (ins || del) ? 1u + l : 0u;
    } else {
      uint32_t te;
      const uint32_t E = kdf_scan(eq ? l : 0u, lane, te);
      const unsigned long long em = __ballot(x || del), lower = em & below;
      const uint32_t Ep = (uint32_t)__shfl((int)E, lower ? 63 - __builtin_clzll(lower) : 0);
      mn = lower ? E - Ep : n + E;
      const uint32_t Eq = (uint32_t)__shfl((int)E, em ? 63 - __builtin_clzll(em) : 0);
      n = krc_uniform(em ? te - Eq : n + te);
      nd = kdf_digits(mn);
      nb = x ? nd + 2u * l - 1u : del ? nd + 1u + l : 0u;
    }
    const Cur mb = at + kdf_scan((Cur)nb, lane, tb);
    if (EMIT) {
      // one shape for every run: a number (cs: behind the sign), a sign, then the bytes of the bases of an X, I or D run, one per turn:
      // cs X is '*', reference base, read base per base; MD X is a base, then '0' and a base.  What a lane is doing lives in a few
      // integers (vector registers), not in lane masks held across the loops (scalar pairs, of which the walk has none to spare)
      uint32_t p = (uint32_t)mb;
      const uint32_t qj = (uint32_t)mj, rr = (uint32_t)mr;
      const uint32_t xi = x ? 1u : 0u, mfix = ins ? 2u : 1u;
      const uint32_t sign = KIND == KDF_CS ? (eq ? ':' : ins ? '+' : del ? '-' : 0u) : (del ? '^' : 0u);
      const uint32_t ndn = (KIND == KDF_CS ? eq : (x || del)) ? nd : 0u;
      const uint32_t cnt = KIND == KDF_CS ? (x ? 3u * l : (ins || del) ? l : 0u) : (x ? 2u * l - 1u : del ? l : 0u);
      if (KIND == KDF_CS && sign) out.put(p++, (uint8_t)sign);
      out.number(p, KIND == KDF_CS ? l : mn, ndn);
      p += ndn;
      if (KIND == KDF_MD && sign) out.put(p++, (uint8_t)sign);
#pragma unroll 1
      for (uint32_t k = 0; k < cnt; ++k) {
        uint32_t t, m;                                 // the base, and what of it: 0 a filler, 1 the reference's, 2 the read's
        if (KIND == KDF_CS) { const uint32_t q3 = k / 3u; t = k - xi * (k - q3); m = mfix + xi * (k - 3u * q3 - mfix); }
        else { t = (k + xi) >> xi; m = 1u - xi * (k & 1u); }
        uint8_t ch = KIND == KDF_CS ? '*' : '0';
        if (m) {                                       // (inside the ranges the lane has checked)
          const uint8_t* src = m == 2u ? P.qtext + (rv ? (uint64_t)(hi - 1u - (qj + t)) : (uint64_t)lo + (qj + t)) : P.rtext + (rr + t);
          uint32_t code = kdf_code(*src);
          if (m == 2u && rv && code < 4u) code = 3u - code;
          ch = KIND == KDF_CS ? kdf_lower(code) : kdf_upper(code);
        }
        out.put(p + k, ch);
      }
    }
    j += tj; r += tr; at += tb;
  }
  if ((uint64_t)j != L) return false;
  if (KIND == KDF_MD) {
    const uint32_t nd = kdf_digits(n);
    if (EMIT && lane == 0u) out.number((uint32_t)at, n, nd);
    at += nd;
  }
  bytes = at;
  return true;
}

template <uint32_t KIND>
__global__ __launch_bounds__(KDF_THREADS) void k_diffs_count(KdfArgs P, uint8_t* __restrict__ ok, uint32_t* __restrict__ nbytes) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KDF_WAVES;
  for (uint32_t c = krc_uniform(blockIdx.x * KDF_WAVES + (threadIdx.x >> 6)); c < P.n_rows; c += stride) {
    uint64_t bytes;
    bool good = kdf_walk<KIND, false>(P, c, lane, KdfOut{nullptr, 0}, bytes);
    if (bytes >> 32) good = false;                  // (a text of 4 GiB: the scan counts in u32)
    if (lane == 0u) { ok[c] = good ? 1 : 0; nbytes[c] = good ? (uint32_t)bytes : 0u; }
  }
}
template <uint32_t KIND>
__global__ __launch_bounds__(KDF_THREADS) void k_diffs_emit(KdfArgs P, const uint8_t* __restrict__ ok, const uint64_t* __restrict__ offsets, uint64_t total,
                                                            uint8_t* __restrict__ out_text) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KDF_WAVES;
  for (uint32_t c = krc_uniform(blockIdx.x * KDF_WAVES + (threadIdx.x >> 6)); c < P.n_rows; c += stride) {
    const uint64_t o0 = kdf_uniform64(offsets[c]), o1 = kdf_uniform64(offsets[c + 1]);
    if (!ok[c] || o1 <= o0 || o1 > total || (o1 - o0) >> 32) continue;    // a row without text; or offsets that are not this call's
    uint64_t bytes;
    kdf_walk<KIND, true>(P, c, lane, KdfOut{out_text + o0, (uint32_t)(o1 - o0)}, bytes);
  }
}

// ---- kh_oriented_rows
#define KOR_THREADS 256
#define KOR_WAVES (KOR_THREADS / 64)
// A<->T, C<->G in every byte, the case kept; any other byte stays itself
__device__ __forceinline__ uint64_t kor_complement(uint64_t w) {
  const uint64_t u = w & KED_B(0xdf);
  const uint64_t at = ~(ked_nonzero(u ^ KED_B(0x41)) & ked_nonzero(u ^ KED_B(0x54))) & KED_B(0x80);
  const uint64_t cg = ~(ked_nonzero(u ^ KED_B(0x43)) & ked_nonzero(u ^ KED_B(0x47))) & KED_B(0x80);
  return w ^ ((at >> 7) * 0x15u) ^ ((cg >> 7) * 0x04u);
}
__device__ __forceinline__ uint8_t kor_complement1(uint8_t b) {
  const uint32_t u = b & 0xdfu;
  return (u == 0x41u || u == 0x54u) ? (uint8_t)(b ^ 0x15u) : (u == 0x43u || u == 0x47u) ? (uint8_t)(b ^ 0x04u) : b;
}
__global__ __launch_bounds__(KOR_THREADS) void k_orient_len(const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, uint64_t n_rows, uint64_t n,
                                                            uint32_t* __restrict__ len) {
  const uint64_t stride = (uint64_t)gridDim.x * KOR_THREADS;
  for (uint64_t c = (uint64_t)blockIdx.x * KOR_THREADS + threadIdx.x; c < n_rows; c += stride) {
    const uint64_t a = min((uint64_t)lo[c], n), b = min((uint64_t)hi[c], n);
    len[c] = b > a ? (uint32_t)(b - a) : 0u;         // (lo and hi are u32: a length fits)
  }
}
__global__ __launch_bounds__(KOR_THREADS) void k_orient_copy(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                                             const uint8_t* __restrict__ rev, uint32_t n_rows, uint32_t complement, const uint64_t* __restrict__ offsets,
                                                             uint64_t total, uint8_t* __restrict__ out_text) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KOR_WAVES;
  for (uint32_t c = krc_uniform(blockIdx.x * KOR_WAVES + (threadIdx.x >> 6)); c < n_rows; c += stride) {
    const uint64_t a = kdf_uniform64(min((uint64_t)lo[c], n)), b = kdf_uniform64(min((uint64_t)hi[c], n));
    const uint64_t o0 = kdf_uniform64(offsets[c]), o1 = kdf_uniform64(offsets[c + 1]);
    if (b <= a || o1 > total || o1 < o0 || o1 - o0 != b - a) continue;    // an empty row; or offsets that are not this call's
    const uint64_t len = b - a;
    const uint32_t rv = krc_uniform(rev[c] & 1u);
    const bool comp = rv && complement;
    uint8_t* const dst = out_text + o0;
    const uint64_t head = min(len, (uint64_t)((0u - (uint32_t)(uintptr_t)dst) & 7u)), nw = (len - head) >> 3, tail = head + (nw << 3);
    // the bytes before the first and behind the last whole word of the destination: at most 7 each, one per lane
    if (lane < 14u) {
      const uint64_t t = lane < 7u ? lane : tail + (lane - 7u);
      if (lane < 7u ? t < head : t < len) {
        const uint8_t x = rv ? text[b - 1u - t] : text[a + t];
        dst[t] = comp ? kor_complement1(x) : x;
      }
    }
    for (uint64_t w = lane; w < nw; w += 64u) {
      const uint64_t t = head + (w << 3);
      uint64_t x;
      __builtin_memcpy(&x, rv ? text + (b - t - 8u) : text + (a + t), 8);
      if (rv) x = __builtin_bswap64(x);
      if (comp) x = kor_complement(x);
      *reinterpret_cast<uint64_t*>(dst + t) = x;
    }
  }
}
