// kh_kernels_index_wide.h -- gfx950 device code of the position index over 16-byte k-mers (kh_wide_index_* and kh_kmers128_from_*_pos),
// included once by kmerhash_amd.hip after kh_kernels_index.h.  Prefix kw_index_ (and kw_kmers_emit_pos, the sibling of kw_kmers_emit).
//
// The wide index is the index of kh_kernels_index.h on the wide Robin Hood table (kh_kernels_wide.h: 32-byte slots {w0, w1, val, info}):
// the kernels that touch a slot or cut a window are here, the key-width-independent half -- k_index_tile_sums / _scan_sums / _scan_apply,
// k_index_tile_sort, k_index_seg_radix, k_index_gather -- is used as it is.  Build: wide counting insert (unchanged code) ->
// kw_index_canon_runs (keys of one home bucket in ascending order of (w1 << 64) | w0) -> k_values_tile_count<KV_WIDE> + kw_index_rank
// (slot-order rank, counts, rank into the slot) -> scan -> kw_index_scatter (two-slot probe + cursor atomic + 4-byte write per pair) ->
// tile sort -> segment radix.  Lookup: kw_index_lookup -> scan -> k_index_gather.  Wave64 everywhere; no kernel waits on another
// workgroup, every loop is bounded (probe distance < 128, run length < 128).
#pragma once
#include "kh_kernels_index.h"

// ---------------------------------------------------------------------------------------------
// 16-byte k-mers with the byte offset of their window: kw_kmers_emit plus one 4-byte store per window.  Written straight out, not staged:
// a tile of 4096 k-mers is 64 KB of LDS for the k-mers alone (one workgroup per CU, one wave per SIMD), against 1.6 KB here; a lane's
// windows are consecutive in the output, so its sixteen 16-byte stores fill whole 64-byte sectors and its sixteen offsets one.
// ---------------------------------------------------------------------------------------------
template <bool CANON>
__global__ __launch_bounds__(KH_KM_THREADS) void kw_kmers_emit_pos(const uint8_t* __restrict__ seq, uint64_t n, uint32_t k, const uint64_t* __restrict__ tile_off,
                                                                   uint64_t* __restrict__ out, uint32_t* __restrict__ out_pos) {
  typedef KhKm<2> M;
  __shared__ uint32_t words[KH_KM_TILE / 16 + M::HALO];
  __shared__ uint16_t invs[KH_KM_TILE / 16 + M::HALO];
  __shared__ uint32_t wtot[KH_KM_THREADS / 64];
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
  uint64_t pos = tile_off[blockIdx.x] + (incl - mine);
  for (uint32_t w = 0; w < wid; ++w) pos += wtot[w];
  for (uint32_t j = 0; j < 16; ++j) {
    if ((vmask >> j) & 1u) {
      uint64_t w0, w1;
      M::forward(W, j, k, &w0, &w1);
      if (CANON) kh_xf128(&w0, &w1, k);
      reinterpret_cast<ulonglong2*>(out)[pos] = make_ulonglong2(w0, w1);
      out_pos[pos] = (uint32_t)(tile0 + 16u * tid + j);
      ++pos;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// canonical slot order (k_index_canon_runs on KwSlot): the lane that owns the first slot of a run of equal home bucket walks it (shorter
// than 128 slots and than the table) and selection-sorts (w0, w1, val) by the 128-bit key, w1 the major word; the info bytes are
// positional and stay.  Runs are disjoint: no two lanes touch a slot.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool kw_index_in_run(const KwSlot* __restrict__ slots, uint64_t j, uint64_t mask, uint64_t home) {
  const uint32_t b = slots[j].info & 0xFFu;
  return b >= 0x80u && ((j - (b & 0x7Fu)) & mask) == home;
}
__global__ __launch_bounds__(256) void kw_index_canon_runs(KwSlot* __restrict__ slots, uint64_t cap) {
  const uint64_t mask = cap - 1, stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += stride) {
    const uint32_t b = slots[i].info & 0xFFu;
    if (b < 0x80u) continue;
    const uint64_t home = (i - (b & 0x7Fu)) & mask;
    if (kw_index_in_run(slots, (i - 1) & mask, mask, home)) continue;          // not the first slot of its run
    uint32_t len = 1;
    while (len < 128u && len < cap && kw_index_in_run(slots, (i + len) & mask, mask, home)) ++len;
    for (uint32_t a = 0; a + 1 < len; ++a) {
      KwSlot* sa = slots + ((i + a) & mask);
      uint64_t m0 = sa->w0, m1 = sa->w1; uint32_t at = a;
      for (uint32_t c = a + 1; c < len; ++c) {
        const KwSlot* sc = slots + ((i + c) & mask);
        const uint64_t c0 = sc->w0, c1 = sc->w1;
        if (c1 < m1 || (c1 == m1 && c0 < m0)) { m0 = c0; m1 = c1; at = c; }
      }
      if (at != a) {
        KwSlot* sm = slots + ((i + at) & mask);
        const uint64_t a0 = sa->w0, a1 = sa->w1; const uint32_t va = sa->val, vm = sm->val;
        sa->w0 = m0; sa->w1 = m1; sa->val = vm; sm->w0 = a0; sm->w1 = a1; sm->val = va;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// rank pass (k_index_rank on the KV_WIDE tiling; the tile sums come from k_values_tile_count<KV_WIDE> over the full value range): live
// slot -> rank r in slot order; counts[r] = the slot's value, and the value becomes r.  Every slot belongs to one lane: plain stores.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KV_SEL_THREADS) void kw_index_rank(KwSlot* __restrict__ slots, uint64_t cap, const uint64_t* __restrict__ tile_off,
                                                                uint32_t* __restrict__ counts) {
  __shared__ uint32_t wcnt[KV_SEL_ROWS * (KV_SEL_THREADS / 64)];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t tbase = (uint64_t)blockIdx.x * KV_SEL_TILE;
  KvItem it[KV_SEL_ROWS];
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + tid;
    it[j] = kv_ld<KV_WIDE>(slots, i < cap ? i : cap - 1);
  }
  uint32_t hit = 0, rank[KV_SEL_ROWS];
#pragma unroll
  for (int j = 0; j < KV_SEL_ROWS; ++j) {
    const uint64_t i = tbase + (uint64_t)j * KV_SEL_THREADS + tid;
    const bool m = i < cap && kv_live<KV_WIDE>(it[j].info);
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
// the probe of scatter and lookup: the KW_Q_ITEMS keys of a lane, the two-slot step of kw_find (one 64-byte sector when the home is
// even) of all of them requested before the first is looked at, the rare longer probes continued one by one by kw_find_pos (bounded by
// probe distance 127).  Returns the bit mask of hits, val[j] of the hits (after a build: the key's rank).
// ---------------------------------------------------------------------------------------------
#define KW_INDEX_Q_TILE (KW_Q_THREADS * KW_Q_ITEMS)
template <int HASH>
__device__ __forceinline__ uint32_t kw_index_probe_items(const KwSlots& T, const uint64_t (&w0)[KW_Q_ITEMS], const uint64_t (&w1)[KW_Q_ITEMS], uint32_t valid,
                                                         uint64_t seed, uint32_t (&val)[KW_Q_ITEMS]) {
  const uint64_t mask = T.cap - 1;
  uint64_t home[KW_Q_ITEMS];
  KwLive a[KW_Q_ITEMS], b[KW_Q_ITEMS];
#pragma unroll
  for (int j = 0; j < KW_Q_ITEMS; ++j) home[j] = ((valid >> j) & 1u) ? (kw_hash<HASH>(w0[j], w1[j], seed) & mask) : 0ull;
#pragma unroll
  for (int j = 0; j < KW_Q_ITEMS; ++j) { a[j] = kw_slot_ld(T.s + home[j]); b[j] = kw_slot_ld(T.s + ((home[j] + 1) & mask)); }
  uint32_t hit = 0;
#pragma unroll
  for (int j = 0; j < KW_Q_ITEMS; ++j) {
    if (!((valid >> j) & 1u)) continue;
    const uint32_t ia = a[j].info & 0xFFu, ib = b[j].info & 0xFFu;
    if (ia == 0x80u && a[j].w0 == w0[j] && a[j].w1 == w1[j]) { hit |= 1u << j; val[j] = a[j].val; }
    else if (ia >= 0x80u && ib == 0x81u && b[j].w0 == w0[j] && b[j].w1 == w1[j]) { hit |= 1u << j; val[j] = b[j].val; }
    else if (ia >= 0x80u && ib >= 0x81u) {          // the key may sit further out
      uint32_t v = 0;
      if (kw_find_pos(T.s, mask, home[j], w0[j], w1[j], &v) != KH_NONE) { hit |= 1u << j; val[j] = v; }
    }
  }
  return hit;
}

// ---------------------------------------------------------------------------------------------
// scatter: every (key, pos) pair probes the table for its key's rank, takes the next place of that key's segment from its cursor
// (initialised from offsets) and writes the position there.  The order inside a segment is whatever the atomics gave and is restored by
// k_index_tile_sort / k_index_seg_radix.
// ---------------------------------------------------------------------------------------------
template <int HASH>
__global__ __launch_bounds__(KW_Q_THREADS) void kw_index_scatter(KwSlots T, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ pos, uint64_t n, uint64_t seed,
                                                                 uint32_t* __restrict__ cursor, uint32_t* __restrict__ positions, uint64_t total, uint64_t nranks) {
  for (uint64_t base = (uint64_t)blockIdx.x * KW_INDEX_Q_TILE; base < n; base += (uint64_t)gridDim.x * KW_INDEX_Q_TILE) {
    uint64_t w0[KW_Q_ITEMS], w1[KW_Q_ITEMS]; uint32_t r[KW_Q_ITEMS], p[KW_Q_ITEMS];
    uint32_t valid = 0;
#pragma unroll
    for (int j = 0; j < KW_Q_ITEMS; ++j) {
      const uint64_t i = base + (uint64_t)j * KW_Q_THREADS + threadIdx.x;
      w0[j] = 0; w1[j] = 0; r[j] = 0; p[j] = 0;
      if (i < n) {
        const uint4 k = reinterpret_cast<const uint4*>(keys)[i];
        w0[j] = (uint64_t)k.x | ((uint64_t)k.y << 32); w1[j] = (uint64_t)k.z | ((uint64_t)k.w << 32);
        p[j] = pos[i]; valid |= 1u << j;
      }
    }
    const uint32_t hit = kw_index_probe_items<HASH>(T, w0, w1, valid, seed, r);
#pragma unroll
    for (int j = 0; j < KW_Q_ITEMS; ++j) {
      if (((hit >> j) & 1u) && r[j] < nranks) {
        const uint32_t dst = atomicAdd(&cursor[r[j]], 1u);
        if (dst < total) positions[dst] = p[j];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// lookup: (begin, count) of every query key -- one probe (the slot's value is the rank) and two adjacent offsets words; a miss is (0, 0).
// ---------------------------------------------------------------------------------------------
template <int HASH>
__global__ __launch_bounds__(KW_Q_THREADS) void kw_index_lookup(KwSlots T, const uint64_t* __restrict__ q, uint64_t n, uint64_t seed, const uint32_t* __restrict__ offsets,
                                                                uint64_t nranks, uint32_t* __restrict__ out_begin /* or null */, uint32_t* __restrict__ out_count) {
  for (uint64_t base = (uint64_t)blockIdx.x * KW_INDEX_Q_TILE; base < n; base += (uint64_t)gridDim.x * KW_INDEX_Q_TILE) {
    uint64_t w0[KW_Q_ITEMS], w1[KW_Q_ITEMS]; uint32_t r[KW_Q_ITEMS];
    uint32_t valid = 0;
#pragma unroll
    for (int j = 0; j < KW_Q_ITEMS; ++j) {
      const uint64_t i = base + (uint64_t)j * KW_Q_THREADS + threadIdx.x;
      w0[j] = 0; w1[j] = 0; r[j] = 0;
      if (i < n) {
        const uint4 k = reinterpret_cast<const uint4*>(q)[i];
        w0[j] = (uint64_t)k.x | ((uint64_t)k.y << 32); w1[j] = (uint64_t)k.z | ((uint64_t)k.w << 32);
        valid |= 1u << j;
      }
    }
    const uint32_t hit = kw_index_probe_items<HASH>(T, w0, w1, valid, seed, r);
#pragma unroll
    for (int j = 0; j < KW_Q_ITEMS; ++j) {
      const uint64_t i = base + (uint64_t)j * KW_Q_THREADS + threadIdx.x;
      if ((valid >> j) & 1u) {
        uint32_t b = 0, c = 0;
        if (((hit >> j) & 1u) && r[j] < nranks) { b = offsets[r[j]]; c = offsets[r[j] + 1] - b; }
        if (out_begin) out_begin[i] = b;
        out_count[i] = c;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// append (see kh_kernels_index.h): the batch counted onto the seeded counts -- the probe of kw_index_scatter, one atomic per pair.  The
// other kernels of append and erase read value and info only and are k_index_*<KV_WIDE>.
// ---------------------------------------------------------------------------------------------
template <int HASH>
__global__ __launch_bounds__(KW_Q_THREADS) void kw_index_count_pairs(KwSlots T, const uint64_t* __restrict__ keys, uint64_t n, uint64_t seed, uint32_t* __restrict__ counts,
                                                                     uint64_t nranks) {
  for (uint64_t base = (uint64_t)blockIdx.x * KW_INDEX_Q_TILE; base < n; base += (uint64_t)gridDim.x * KW_INDEX_Q_TILE) {
    uint64_t w0[KW_Q_ITEMS], w1[KW_Q_ITEMS]; uint32_t r[KW_Q_ITEMS];
    uint32_t valid = 0;
#pragma unroll
    for (int j = 0; j < KW_Q_ITEMS; ++j) {
      const uint64_t i = base + (uint64_t)j * KW_Q_THREADS + threadIdx.x;
      w0[j] = 0; w1[j] = 0; r[j] = 0;
      if (i < n) {
        const uint4 k = reinterpret_cast<const uint4*>(keys)[i];
        w0[j] = (uint64_t)k.x | ((uint64_t)k.y << 32); w1[j] = (uint64_t)k.z | ((uint64_t)k.w << 32);
        valid |= 1u << j;
      }
    }
    const uint32_t hit = kw_index_probe_items<HASH>(T, w0, w1, valid, seed, r);
#pragma unroll
    for (int j = 0; j < KW_Q_ITEMS; ++j)
      if (((hit >> j) & 1u) && r[j] < nranks) atomicAdd(&counts[r[j]], 1u);
  }
}
