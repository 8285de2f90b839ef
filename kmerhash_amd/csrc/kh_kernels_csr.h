// kh_kernels_csr.h -- gfx950 device code of kh_csr_unpermute, included once by kmerhash_amd.hip after kh_kernels_index.h.  Prefix k_csr_.
//
// A CSR that arrives in a permuted order (counts_perm[j] and its segment belong to query origin[j]) is put back into query order:
//   scan(counts_perm) -> begin_perm        the index's scan kernels, unchanged (k_index_tile_sums / _scan_sums / _scan_apply<u32>)
//   k_csr_scatter                          counts and segment begins to their query (below)
//   scan(out_counts)  -> out_offsets       the same scan kernels (k_index_scan_apply<u64>)
//   k_index_gather                         unchanged: output element j finds its query by binary search in out_offsets and copies
//                                          pos_perm[begin_q[query] + (j - out_offsets[query])] -- balanced over OUTPUT elements
// so the only new device code is the scatter.  Wave64, plain vector loads and stores, no LDS.
#pragma once
#include "kh_kernels_index.h"

// out_counts[origin[j]] = counts_perm[j] and begin_q[origin[j]] = begin_perm[j].  origin is a permutation of 0..n-1 (precondition): every
// destination has one writer, plain stores.  Reads are coalesced, the two 4-byte stores go wherever origin sends them.  An origin outside
// 0..n-1 breaks the precondition; it is dropped here so that nothing is written outside the two arrays.
#define KC_THREADS 256
__global__ __launch_bounds__(KC_THREADS) void k_csr_scatter(const uint32_t* __restrict__ counts_perm, const uint32_t* __restrict__ begin_perm,
                                                            const uint32_t* __restrict__ origin, uint64_t n, uint32_t* __restrict__ out_counts,
                                                            uint32_t* __restrict__ begin_q) {
  const uint64_t stride = (uint64_t)gridDim.x * KC_THREADS;
  for (uint64_t j = (uint64_t)blockIdx.x * KC_THREADS + threadIdx.x; j < n; j += stride) {
    const uint32_t o = origin[j], c = counts_perm[j], b = begin_perm[j];
    if (o < n) { out_counts[o] = c; begin_q[o] = b; }
  }
}
