// kh_kernels_values.h -- gfx950 device code of the value-range operations (kh_value_histogram / kh_select_values / kh_erase_values and
// their kh_wide_ forms), included once by kmerhash_amd.hip after kh_kernels_wide.h.  Prefix kv_ / k_value(s)_.
//
// Every kernel is ONE streaming pass over the slot array of a table of any of the three layouts (KV_RH / KV_LP: 16-byte slots of the
// 64-bit tables; KV_WIDE: 32-byte slots of the 16-byte-key table), one slot per access, several accesses of a lane in flight.  The
// predicate is the closed range lo <= value <= hi on the UNSIGNED 32-bit value of an occupied slot (an LP tombstone is not occupied).
#pragma once
#include "kh_kernels_wide.h"

enum { KV_RH = 0, KV_LP = 1, KV_WIDE = 2 };
#define KV_MAX_BINS 16384u

template <int LAY> struct KvSlot {};
template <> struct KvSlot<KV_RH> { typedef KhSlot type; };
template <> struct KvSlot<KV_LP> { typedef KhSlot type; };
template <> struct KvSlot<KV_WIDE> { typedef KwSlot type; };

struct KvItem { uint32_t val, info; };
// value + info word of slot i: the 16-byte slot itself, or the second half of the 32-byte slot's live bytes
template <int LAY>
__device__ __forceinline__ KvItem kv_ld(const void* __restrict__ slots, uint64_t i) {
  KvItem r;
  if (LAY == KV_WIDE) {
    const uint2 b = *reinterpret_cast<const uint2*>(static_cast<const char*>(slots) + i * sizeof(KwSlot) + 16);
    r.val = b.x; r.info = b.y;
  } else {
    const uint4 w = kh_slot_ld(static_cast<const KhSlot*>(slots) + i);
    r.val = w.z; r.info = w.w;
  }
  return r;
}
template <int LAY>
__device__ __forceinline__ bool kv_live(uint32_t info) {
  const uint32_t b = info & 0xFFu;
  return LAY == KV_LP ? b < 0x40u : b >= 0x80u;
}
template <int LAY>
__device__ __forceinline__ bool kv_match(const KvItem& it, uint32_t lo, uint32_t hi) { return kv_live<LAY>(it.info) && it.val >= lo && it.val <= hi; }

// ---------------------------------------------------------------------------------------------
// spectrum: per-workgroup counters in dynamic LDS (nbins x 4 B), one global add per non-zero bin at the end.  A k-mer spectrum piles
// nearly every element into one or two bins: the lanes of a wave that hold the leader's bin are counted with a ballot and added by ONE
// LDS atomic, twice over (the two heaviest bins of the wave in the common case); only what is left adds lane by lane.  A wave whose
// 64 values are equal issues one ds_add instead of 64 to one address.
// ---------------------------------------------------------------------------------------------
#define KV_HIST_THREADS 512
#define KV_HIST_ITEMS 4
__device__ __forceinline__ void kv_wave_add(uint32_t* bins, uint32_t bin, bool active) {
  const uint32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int round = 0; round < 2; ++round) {
    const unsigned long long act = __ballot(active);
    if (!act) return;                                   // (wave-uniform)
    const uint32_t leader = (uint32_t)__ffsll((long long)act) - 1u;
    const uint32_t b0 = __shfl(bin, (int)leader, 64);
    const bool same = active && bin == b0;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(&bins[b0], (uint32_t)__popcll(m));
    if (same) active = false;
  }
  if (active) atomicAdd(&bins[bin], 1u);
}
template <int LAY>
__global__ __launch_bounds__(KV_HIST_THREADS) void k_value_hist(const void* __restrict__ slots, uint64_t cap, uint32_t nbins,
                                                                unsigned long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t kv_bins[];
  for (uint32_t b = threadIdx.x; b < nbins; b += KV_HIST_THREADS) kv_bins[b] = 0;
  __syncthreads();
  const uint64_t span = (uint64_t)gridDim.x * KV_HIST_THREADS;
  const uint32_t last = nbins - 1u;
  for (uint64_t i0 = (uint64_t)blockIdx.x * KV_HIST_THREADS; i0 < cap; i0 += span * KV_HIST_ITEMS) {      // (i0: workgroup-uniform)
    KvItem it[KV_HIST_ITEMS];
#pragma unroll
    for (int j = 0; j < KV_HIST_ITEMS; ++j) {            // clamped, not predicated: the loads stay in flight together
      const uint64_t i = i0 + (uint64_t)j * span + threadIdx.x;
      it[j] = kv_ld<LAY>(slots, i < cap ? i : cap - 1);
    }
#pragma unroll
    for (int j = 0; j < KV_HIST_ITEMS; ++j) {
      const uint64_t i = i0 + (uint64_t)j * span + threadIdx.x;
      kv_wave_add(kv_bins, it[j].val < last ? it[j].val : last, i < cap && kv_live<LAY>(it[j].info));
    }
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nbins; b += KV_HIST_THREADS) {
    const uint32_t c = kv_bins[b];
    if (c) atomicAdd(&out[b], (unsigned long long)c);
  }
}

// ---------------------------------------------------------------------------------------------
// erase by value: the marks pass.  RH (both key widths): KH_INFO_ERASE_MARK on the matching occupied slots -- the re-layout that
// follows drops them (rebuild(..., drop_marked)); LP: the tombstone byte in place, as k_erase_mark writes it.  Every slot belongs to
// one lane, so the info word is written with a plain store; the marks are counted in registers, one atomic per workgroup.
// ---------------------------------------------------------------------------------------------
#define KV_MARK_THREADS 256
#define KV_MARK_ITEMS 4
template <int LAY>
__global__ __launch_bounds__(KV_MARK_THREADS) void k_values_mark(void* __restrict__ slots, uint64_t cap, uint32_t lo, uint32_t hi,
                                                                 unsigned long long* __restrict__ n_marked) {
  __shared__ uint32_t s_mine[KV_MARK_THREADS / 64];
  typedef typename KvSlot<LAY>::type Slot;
  Slot* S = static_cast<Slot*>(slots);
  const uint64_t span = (uint64_t)gridDim.x * KV_MARK_THREADS;
  uint32_t mine = 0;
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
      if (i < cap && kv_match<LAY>(it[j], lo, hi) && !(LAY != KV_LP && (it[j].info & KH_INFO_ERASE_MARK))) {
        S[i].info = LAY == KV_LP ? (it[j].info | 0x80u) : (it[j].info | KH_INFO_ERASE_MARK);
        ++mine;
      }
    }
  }
  mine = kh_wave_sum(mine);
  if ((threadIdx.x & 63) == 0) s_mine[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t tot = 0;
    for (uint32_t w = 0; w < KV_MARK_THREADS / 64; ++w) tot += s_mine[w];
    if (tot) atomicAdd(n_marked, (unsigned long long)tot);
  }
}

// ---------------------------------------------------------------------------------------------
// select by value, in slot order (the order of to_vector): tiles of KV_SEL_TILE slots, a workgroup per tile, the tile as KV_SEL_ROWS
// rows of 256 consecutive slots (lane t holds slot 256 j + t of every row j: each load of a wave is one contiguous run).
// k_values_tile_count gives the matches per tile; after k_scan_u32_to_u64 the host knows the total BEFORE anything is written (a
// caller's buffer that is too small is never touched); k_values_tile_emit reads the tile again, ranks the matches of a row with a
// ballot per wave, the (row, wave) counts with a short scan through LDS, and writes (key, value) straight to its place.
// ---------------------------------------------------------------------------------------------
#define KV_SEL_THREADS 256
#define KV_SEL_ROWS 8
#define KV_SEL_TILE (KV_SEL_THREADS * KV_SEL_ROWS)
template <int LAY>
__global__ __launch_bounds__(KV_SEL_THREADS) void k_values_tile_count(const void* __restrict__ slots, uint64_t cap, uint32_t lo, uint32_t hi,
                                                                      uint32_t* __restrict__ sums) {
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
    c += (i < cap && kv_match<LAY>(it[j], lo, hi)) ? 1u : 0u;
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
__global__ __launch_bounds__(KV_SEL_THREADS) void k_values_tile_emit(const void* __restrict__ slots, uint64_t cap, uint32_t lo, uint32_t hi,
                                                                     const uint64_t* __restrict__ tile_off, uint64_t* __restrict__ out_keys,
                                                                     uint32_t* __restrict__ out_vals) {
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
    const bool m = i < cap && kv_match<LAY>(it[j], lo, hi);
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
      if (LAY == KV_WIDE) {
        const uint4 k = *reinterpret_cast<const uint4*>(S + i);
        out_keys[2 * x] = (uint64_t)k.x | ((uint64_t)k.y << 32);
        out_keys[2 * x + 1] = (uint64_t)k.z | ((uint64_t)k.w << 32);
      } else {
        out_keys[x] = *reinterpret_cast<const uint64_t*>(S + i);
      }
      if (out_vals) out_vals[x] = it[j].val;
    }
  }
}
