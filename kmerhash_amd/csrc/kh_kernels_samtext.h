// kh_kernels_samtext.h -- gfx950 device code of kh_sam_lines, included once by kmerhash_amd.hip after kh_kernels_rescue.h.  Prefix k_samtext_
// (helpers kst_).
//
// kh_sam_lines turns line columns and byte CSRs into the text of SAM alignment lines (definition: include/kmerhash_amd.h, model:
// tests/samtext_model.py).  A line is KST_PIECES pieces in a fixed order; a piece is a literal of at most 8 bytes (the tab in front of a
// field, a tag's name, a '*' or '=' that stands for a field, the tp letter, the closing line feed) followed by a body: nothing, the
// decimal digits of a number, or a row of a CSR.
//   kst_piece        lane p sizes piece p of a line: it loads the piece's column entry and, for a CSR piece, the two offsets of its row
//                    -- one gather for all fields instead of eight dependent scalar chains.  Both kernels go through it, so the two
//                    passes cannot disagree about a length.  The CSRs and the columns reach it as two tables in the kernel arguments
//                    that a lane indexes by its piece
//   k_samtext_count  one wavefront per line, fixed grid, grid-stride over the lines: the wave sum of the piece lengths.  Row lengths
//                    and digit counts only; no text is read
//   k_samtext_emit   the same walk; one wave prefix sum gives the pieces their places.  Every lane writes its own literal and digits
//                    (at most 8 + 11 bytes); then the eight CSR pieces are copied one after the other by the whole wave, the
//                    8-byte-word way of k_orient_copy: a line starts at any residue mod 8 and no piece is aligned to its source, so
//                    the bytes up to the first 8-byte boundary of the DESTINATION and those behind the last go one per lane and
//                    between them every lane moves whole words -- an 8-byte load from the source wherever it lies, one aligned
//                    8-byte store
// No atomics, no LDS: the pieces of a line and the lines of a call own disjoint byte ranges.
// Every row index and every offset that comes out of memory is range-checked or clamped before it addresses anything -- the lanes that
// own no piece index entry 0 of the argument tables, never beyond them -- and the emit pass
// writes a line only where the offsets it is given hold exactly the bytes it is about to write, below the total the host passes in.
#pragma once
#include "kh_kernels_sam.h"

#define KST_THREADS 256
#define KST_WAVES (KST_THREADS / 64)
#define KST_PIECES 19u
#define KST_TAGS_BASE 1u      // KH_SAMTAG_*
#define KST_TAGS_S2 2u
#define KST_TAGS_MD 4u
#define KST_TAGS_CS 8u
#define KST_ROW_SAME (-2)     // KH_SAM_RNEXT_SAME

struct KstCsr { const uint64_t* off; const uint8_t* txt; uint64_t n_rows, n_bytes; };
// the CSRs and the line columns as two tables, so that a lane picks its own by index: the tables stay in the kernel-argument segment
// and are read from there, instead of filling a hundred scalar registers
#define KST_CSR_NAMES 0u
#define KST_CSR_TNAMES 1u
#define KST_CSR_CIGAR 2u
#define KST_CSR_SEQ 3u
#define KST_CSR_QUAL 4u
#define KST_CSR_MD 5u
#define KST_CSR_CS 6u
#define KST_CSRS 7u
// columns in the order of the entry point's arguments: l_name l_flag l_rname l_pos l_mapq l_cigar l_rnext l_pnext l_tlen l_seq l_qual
// l_tags l_nm l_tp l_cm l_s1 l_s2 l_md l_cs
#define KST_COL_MAPQ 4u
#define KST_COL_TAGS 11u
#define KST_COL_TP 13u
#define KST_COLS 19u
struct KstArgs {
  KstCsr csr[KST_CSRS];
  const void* col[KST_COLS];
  uint32_t n_lines;
};

// what stands for a CSR field whose row is missing: a name-like field (QNAME, RNAME, CIGAR, RNEXT) prints '*' for a row outside its CSR
// and an empty row as it is; SEQ and QUAL print '*' for an empty row too; a tag's value (MD, cs) is empty where there is no row
#define KST_NAME 0u
#define KST_SEQ 1u
#define KST_TAG 2u
#define KST_NUM 3u          // no CSR field: digits
#define KST_LIT 4u          // no body at all

// up to 8 bytes of text as a word, the first byte lowest
__device__ __forceinline__ constexpr uint64_t kst_lit(const char* s) {
  uint64_t w = 0;
  for (uint32_t t = 0; s[t]; ++t) w |= (uint64_t)(uint8_t)s[t] << (8u * t);
  return w;
}

// piece p of line i, sized: the literal (lit, nlit bytes), a '-' (neg) and nd digits of mag, or blen bytes at src
struct KstPiece {
  uint64_t lit; const uint8_t* src;
  uint32_t nlit, mag, nd, blen; bool neg;
  __device__ __forceinline__ uint32_t bytes() const { return nlit + (neg ? 1u : 0u) + nd + blen; }
};
// what piece p is made of: which literal, which column, which CSR, under which tag bit (0: always)
struct KstWhich { uint64_t lit; uint32_t nlit, col, cid, kind, bit; bool sgn; };
__device__ __forceinline__ KstWhich kst_which(uint32_t p) {
  KstWhich w{kst_lit("\t"), 1, p < KST_COLS ? p : 0u, 0, KST_NUM, 0, false};      // (an idle lane, p >= KST_PIECES, must index inside the tables too)
  switch (p) {
    case 0: w.lit = 0; w.nlit = 0; w.kind = KST_NAME; w.cid = KST_CSR_NAMES; break;
    case 2: w.kind = KST_NAME; w.cid = KST_CSR_TNAMES; break;
    case 5: w.kind = KST_NAME; w.cid = KST_CSR_CIGAR; break;
    case 6: w.kind = KST_NAME; w.cid = KST_CSR_TNAMES; break;
    case 8: w.sgn = true; break;
    case 9: w.kind = KST_SEQ; w.cid = KST_CSR_SEQ; break;
    case 10: w.kind = KST_SEQ; w.cid = KST_CSR_QUAL; break;
    case 11: w.lit = kst_lit("\tNM:i:"); w.nlit = 6; w.col = 12; w.bit = KST_TAGS_BASE; break;
    case 12: w.lit = kst_lit("\ttp:A:"); w.nlit = 6; w.col = KST_COL_TP; w.bit = KST_TAGS_BASE; w.kind = KST_LIT; break;
    case 13: w.lit = kst_lit("\tcm:i:"); w.nlit = 6; w.col = 14; w.bit = KST_TAGS_BASE; break;
    case 14: w.lit = kst_lit("\ts1:i:"); w.nlit = 6; w.col = 15; w.bit = KST_TAGS_BASE; w.sgn = true; break;
    case 15: w.lit = kst_lit("\ts2:i:"); w.nlit = 6; w.col = 16; w.bit = KST_TAGS_S2; w.sgn = true; break;
    case 16: w.lit = kst_lit("\tMD:Z:"); w.nlit = 6; w.col = 17; w.bit = KST_TAGS_MD; w.kind = KST_TAG; w.cid = KST_CSR_MD; break;
    case 17: w.lit = kst_lit("\tcs:Z:"); w.nlit = 6; w.col = 18; w.bit = KST_TAGS_CS; w.kind = KST_TAG; w.cid = KST_CSR_CS; break;
    case 18: w.lit = kst_lit("\n"); w.col = 0; w.kind = KST_LIT; break;
    default: break;      // 1 FLAG, 3 POS, 4 MAPQ, 7 PNEXT: a tab and an unsigned number
  }
  return w;
}
// piece p of line i from its column cp and its CSR C (the kernels pick both out of the argument tables themselves: a table handed on
// by reference would be copied to private memory first)
__device__ __forceinline__ KstPiece kst_piece(const KstWhich& w, const KstCsr& C, const void* cp, uint32_t i, uint32_t p, uint32_t tags) {
  KstPiece q{0, nullptr, 0, 0, 0, 0, false};
  if (p >= KST_PIECES || (w.bit && !(tags & w.bit))) return q;
  q.lit = w.lit; q.nlit = w.nlit;
  if (w.col == KST_COL_MAPQ || w.col == KST_COL_TP) {      // the two byte columns
    const uint32_t v = static_cast<const uint8_t*>(cp)[i];
    if (w.col == KST_COL_TP) { q.lit |= (uint64_t)v << 48; q.nlit = 7; }
    else { q.mag = v; q.nd = kdf_digits(v); }
  } else if (w.kind == KST_NUM) {
    const uint32_t v = static_cast<const uint32_t*>(cp)[i];
    q.neg = w.sgn && (int32_t)v < 0;
    q.mag = q.neg ? 0u - v : v;
    q.nd = kdf_digits(q.mag);
  } else if (w.kind != KST_LIT) {
    const int32_t r = static_cast<const int32_t*>(cp)[i];
    // row r of the CSR, clamped to its text (the entry point bounds n_bytes: a length fits 32 bits)
    bool inside = false; uint64_t a = 0;
    if (C.off != nullptr && r >= 0 && (uint64_t)r < C.n_rows) {
      const uint64_t x = min(C.off[r], C.n_bytes), y = min(C.off[(uint64_t)r + 1u], C.n_bytes);
      inside = true; a = x;
      q.blen = y > x ? (uint32_t)(y - x) : 0u;
    }
    q.src = C.txt + a;
    const bool same = p == 6u && r == KST_ROW_SAME;
    if (same || (w.kind == KST_NAME && !inside) || (w.kind == KST_SEQ && q.blen == 0u)) {
      q.lit |= (uint64_t)(same ? '=' : '*') << (8u * q.nlit); ++q.nlit; q.blen = 0;
    }
  }
  return q;
}

__global__ __launch_bounds__(KST_THREADS) void k_samtext_count(const KstArgs P, uint32_t* __restrict__ bytes) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KST_WAVES;
  const KstWhich w = kst_which(lane);
  const KstCsr C = P.csr[w.cid];
  const void* const cp = P.col[w.col];
  const uint8_t* const l_tags = static_cast<const uint8_t*>(P.col[KST_COL_TAGS]);
  for (uint32_t i = krc_uniform(blockIdx.x * KST_WAVES + (threadIdx.x >> 6)); i < P.n_lines; i += stride) {
    const uint32_t n = krc_wave_sum(kst_piece(w, C, cp, i, lane, krc_uniform(l_tags[i])).bytes());
    if (lane == 0u) bytes[i] = n;
  }
}

// len bytes from src to dst by one wave; len is the same in every lane
__device__ __forceinline__ void kst_copy(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t lane) {
  const uint32_t head = min(len, (0u - (uint32_t)(uintptr_t)dst) & 7u), nw = (len - head) >> 3, tail = head + (nw << 3);
  // the bytes before the first and behind the last whole word of the destination: at most 7 each, one per lane
  if (lane < 14u) {
    const uint32_t t = lane < 7u ? lane : tail + (lane - 7u);
    if (lane < 7u ? t < head : t < len) dst[t] = src[t];
  }
  for (uint32_t w = lane; w < nw; w += 64u) {
    const uint32_t t = head + (w << 3);
    uint64_t x;
    __builtin_memcpy(&x, src + t, 8);
    *reinterpret_cast<uint64_t*>(dst + t) = x;
  }
}

__global__ __launch_bounds__(KST_THREADS) void k_samtext_emit(const KstArgs P, const uint64_t* __restrict__ offsets, uint64_t total, uint8_t* __restrict__ out_text) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KST_WAVES;
  const KstWhich w = kst_which(lane);
  const KstCsr C = P.csr[w.cid];
  const void* const cp = P.col[w.col];
  const uint8_t* const l_tags = static_cast<const uint8_t*>(P.col[KST_COL_TAGS]);
  for (uint32_t i = krc_uniform(blockIdx.x * KST_WAVES + (threadIdx.x >> 6)); i < P.n_lines; i += stride) {
    const uint64_t o0 = kdf_uniform64(offsets[i]), o1 = kdf_uniform64(offsets[i + 1]);
    if (o1 > total || o1 <= o0) continue;      // offsets that are not this call's
    const KstPiece q = kst_piece(w, C, cp, i, lane, krc_uniform(l_tags[i]));
    uint32_t sum;
    const uint32_t at = kdf_scan(q.bytes(), lane, sum);
    if ((uint64_t)sum != o1 - o0) continue;    // columns or rows that changed since the count pass: nothing is written
    uint8_t* const dst = out_text + o0;
    const KdfOut out{dst, sum};
#pragma unroll 1
    for (uint32_t t = 0; t < 8u; ++t) { if (t < q.nlit) out.put(at + t, (uint8_t)(q.lit >> (8u * t))); }
    if (q.neg) out.put(at + q.nlit, (uint8_t)'-');
    out.number(at + q.nlit + (q.neg ? 1u : 0u), q.mag, q.nd);
    // the CSR pieces, one after the other by the whole wave
    const uint32_t body = at + q.nlit;
    constexpr uint32_t rows[8] = {0u, 2u, 5u, 6u, 9u, 10u, 16u, 17u};
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
      const uint32_t len = krc_uniform((uint32_t)__shfl((int)q.blen, (int)rows[k]));
      if (len == 0u) continue;
      const uint32_t to = (uint32_t)__shfl((int)body, (int)rows[k]);
      const uint8_t* const from = reinterpret_cast<const uint8_t*>((uintptr_t)__shfl((unsigned long long)(uintptr_t)q.src, (int)rows[k]));
      kst_copy(dst + to, from, len, lane);
    }
  }
}
