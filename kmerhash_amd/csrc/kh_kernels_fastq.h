// kh_kernels_fastq.h -- gfx950 device code of kh_fastq_records and kh_pack_rows, included once by kmerhash_amd.hip after
// kh_kernels_samtext.h.  Prefixes k_fastq_line_ / k_fastq_records and k_pack_ (helpers kfq_).
//
// kh_fastq_records gives the record structure of a FASTQ text (definition: include/kmerhash_amd.h, model: tests/fastq_model.py).  The
// line number of a byte is the number of '\n' before it, the rule of k_fastq_mask: k_newline_tile_sums and k_scan_u32_to_u64 (kh_kernels.h)
// give every tile of KH_CMP_TILE bytes the number of its first line, then
//   k_fastq_line_ends  the shape of k_fastq_mask: a workgroup per tile, a lane per 8 bytes (one 8-byte load where the text is 8-byte
//                      aligned, bytes otherwise and at the end of the text), an in-tile prefix sum; the lane writes line_end[j], the
//                      offset of newline j, for the newlines among its bytes
//   k_fastq_records    one lane per record, fixed grid, grid-stride: five neighbouring line ends bound the four lines, a '\r' in front
//                      of a line's end is dropped, the first bytes of the lines are tested and the name is walked to its first byte
//                      <= 0x20 -- serially, by the one lane: names are tens of bytes and the columns of a record are 24 bytes, so the
//                      walk is short beside the 4 lines the two kernels before it read.  The record count is not known to the host when
//                      the kernel is queued: every lane derives it from the scanned total of newlines and the last byte of the text, and
//                      lane 0 of the grid writes it, the tail lines and (all lanes, one atomic per wave) the bad records to `counts`
// kh_pack_rows copies byte rows of a text to given places of an output.
//   k_pack_rows        one wavefront per row, fixed grid, grid-stride; the copy is kst_copy (kh_kernels_samtext.h), the 8-byte-word way
//                      of k_orient_copy: bytes up to the first 8-byte boundary of the DESTINATION and behind the last go one per lane,
//                      between them every lane moves whole words, 64 per step, a longer row loops
// No LDS beyond the four wave totals of k_fastq_line_ends.  Every offset that comes out of memory (a line end, lo / hi / dst) is
// range-checked or clamped before it addresses anything; every store of k_pack_rows lies below out_n.
#pragma once
#include "kh_kernels_samtext.h"

#define KFQ_THREADS 256
#define KFQ_WAVES (KFQ_THREADS / 64)
#define KFQ_STRIP_MATE 1u     // KH_FASTQ_STRIP_MATE
#define KFQ_NO_AT 1u          // KH_FASTQ_NO_AT ... the bits of status
#define KFQ_NO_PLUS 2u
#define KFQ_LENGTHS 4u
#define KFQ_NO_NAME 8u

__global__ __launch_bounds__(256) void k_fastq_line_ends(const uint8_t* __restrict__ text, uint64_t n, const uint64_t* __restrict__ tile_off,
                                                         uint32_t* __restrict__ line_end, uint64_t cap_lines) {
  __shared__ uint32_t wtot[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * KH_CMP_TILE + (uint64_t)tid * 8;
  uint8_t c[8];
  uint32_t mine = 0;
  if (base + 8 <= n && (reinterpret_cast<uintptr_t>(text) & 7u) == 0) {
    const uint64_t w = *reinterpret_cast<const uint64_t*>(text + base);
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = (uint8_t)(w >> (8 * j));
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = base + j < n ? text[base + j] : (uint8_t)0;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) mine += c[j] == '\n' ? 1u : 0u;
  uint32_t incl = mine;
  for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); if (lane >= (uint32_t)off) incl += o; }
  if (lane == 63) wtot[wid] = incl;
  __syncthreads();
  uint64_t line = tile_off[blockIdx.x] + (incl - mine);
  for (uint32_t w = 0; w < wid; ++w) line += wtot[w];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (c[j] == '\n') {      // (a byte beyond the text was read as 0)
      if (line < cap_lines) line_end[line] = (uint32_t)(base + j);
      ++line;
    }
  }
}

struct KfqArgs {
  const uint8_t* text; const uint32_t* line_end; const uint64_t* n_newlines;      // the scanned total: tile_off[tiles]
  uint32_t *name_lo, *name_hi, *seq_lo, *seq_hi, *qual_lo; uint8_t* status;       // all five columns or none; status or not
  uint32_t* counts;                                                               // [0] records, [1] bad records (zeroed before), [2] tail lines
  uint64_t n, cap_lines, cap;
  uint32_t flags;
};
// line j of `lines`: [a, b) without the newline and without one '\r' in front of it
__device__ __forceinline__ void kfq_line(const KfqArgs& P, uint64_t j, uint64_t newlines, uint32_t& a, uint32_t& b) {
  a = j == 0 ? 0u : P.line_end[j - 1] + 1u;
  b = j < newlines ? P.line_end[j] : (uint32_t)P.n;
  if (b > a && P.text[b - 1u] == '\r') --b;
}
__global__ __launch_bounds__(KFQ_THREADS) void k_fastq_records(const KfqArgs P) {
  // a non-empty remainder behind the last newline is a last line
  const uint64_t newlines = *P.n_newlines;
  const uint64_t lines = newlines + ((P.n > 0 && P.text[P.n - 1] != '\n') ? 1u : 0u);
  const uint64_t n_rec = lines >> 2;
  const uint64_t gid = (uint64_t)blockIdx.x * KFQ_THREADS + threadIdx.x, stride = (uint64_t)gridDim.x * KFQ_THREADS;
  if (newlines > P.cap_lines) {      // line_end holds cap_lines entries, sized for `cap` records: there are more, only their number is told
    if (gid == 0) P.counts[0] = (uint32_t)n_rec;
    return;
  }
  if (gid == 0) {
    uint32_t tail = 0;
    for (uint64_t j = n_rec << 2; j < lines; ++j) { uint32_t a, b; kfq_line(P, j, newlines, a, b); tail += b > a ? 1u : 0u; }
    P.counts[0] = (uint32_t)n_rec; P.counts[2] = tail;
  }
  const bool emit = P.seq_lo != nullptr && n_rec <= P.cap;      // more records than the caller has room for: the columns stay untouched
  uint32_t bad = 0;
  for (uint64_t r = gid; r < n_rec; r += stride) {
    uint32_t h0, h1, s0, s1, p0, p1, q0, q1;
    kfq_line(P, 4 * r, newlines, h0, h1); kfq_line(P, 4 * r + 1, newlines, s0, s1); kfq_line(P, 4 * r + 2, newlines, p0, p1); kfq_line(P, 4 * r + 3, newlines, q0, q1);
    uint32_t st = 0;
    const bool at = h1 > h0 && P.text[h0] == '@';
    if (!at) st |= KFQ_NO_AT;
    if (!(p1 > p0 && P.text[p0] == '+')) st |= KFQ_NO_PLUS;
    if (q1 - q0 != s1 - s0) st |= KFQ_LENGTHS;
    const uint32_t nlo = h0 + (at ? 1u : 0u);
    uint32_t nhi = nlo;
    while (nhi < h1 && P.text[nhi] > 0x20u) ++nhi;
    if ((P.flags & KFQ_STRIP_MATE) && nhi - nlo > 2u && P.text[nhi - 2u] == '/' && (P.text[nhi - 1u] == '1' || P.text[nhi - 1u] == '2')) nhi -= 2u;
    if (nhi == nlo) st |= KFQ_NO_NAME;
    if (st) { s1 = s0; q0 = s0; ++bad; }      // kept, as an empty read
    if (emit) {
      P.name_lo[r] = nlo; P.name_hi[r] = nhi; P.seq_lo[r] = s0; P.seq_hi[r] = s1; P.qual_lo[r] = q0;
      if (P.status) P.status[r] = (uint8_t)st;
    }
  }
  bad = krc_wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(&P.counts[1], bad);
}

__global__ __launch_bounds__(KFQ_THREADS) void k_pack_rows(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
                                                           const uint64_t* __restrict__ dst, uint32_t n_rows, int sep, uint8_t* __restrict__ out, uint64_t out_n) {
  const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * KFQ_WAVES;
  for (uint32_t i = krc_uniform(blockIdx.x * KFQ_WAVES + (threadIdx.x >> 6)); i < n_rows; i += stride) {
    const uint32_t a = krc_uniform(lo[i]), b = krc_uniform(hi[i]);
    const uint64_t d = kdf_uniform64(dst[i]);
    if (d >= out_n) continue;
    const uint32_t len = (a <= b && (uint64_t)b <= n) ? b - a : 0u;      // a row out of the text is an empty row
    const uint32_t room = (uint32_t)min((uint64_t)len, out_n - d);      // (out_n < 2^32)
    if (room) kst_copy(out + d, text + a, room, lane);
    if (sep >= 0 && lane == 0u && d + len < out_n) out[d + len] = (uint8_t)sep;
  }
}
