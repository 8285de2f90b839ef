// kh_kernels_wide.h -- gfx950 device code of the wide-key (16-byte key) Robin Hood table, included once by kmerhash_amd.hip after
// kh_kernels.h.  Prefix kw_.  The front end around the table is not here: batched hashing, the shard partition, the HyperLogLog update
// and the k-mer window count are the key-width-generic kernels of kh_kernels.h instantiated with KW = 2 (KhKey<2>, KhKm<2>); this file
// adds what differs for 16-byte k-mers (kw_kmers_emit) and the fused text-to-estimate pass over both widths (k_hll_from_text).
//
// Key: {u64 w0, u64 w1} (the memory image of a 16-byte POD key, hashed as 16 bytes: kh_hash128 in kh_hash.h).  Slot: 32 bytes
// {u64 w0, u64 w1, u32 val, u32 info, u64 pad}, 32-byte aligned -- a 64-byte sector holds two slots, a probe reads the 24 live bytes
// of a slot with one dwordx4 and one dwordx2 load.  The low byte of `info` is the reference's RH info byte (0x00 empty, 0x80|distance),
// bit 8 the erase mark of a batch erase (KH_INFO_ERASE_MARK), as in the 64-bit table.
//
// The kernels follow the 64-bit table's GENERAL path: a mutating batch is partitioned by bit-reversed chunk id of the
// partitioning capacity (kw_part_count / k_scan_u32_to_u64 / kw_part_scatter, 24-byte records {w0, w1, idx<<32|val}); one workgroup
// per partition folds its duplicates in LDS and tests the distinct keys against the current table (kw_dedup: the only probes at
// random into HBM); the host decides the capacity; every chunk of the new table is laid out in canonical Robin Hood order into a
// fresh buffer (kw_chunk_count -> k_chunk_carry -> kw_chunk_place, each destination slot written once).  Reads (kw_find) probe two
// slots -- one 64-byte sector when the home is even -- per step, four queries per lane in flight.
#pragma once
#include "kh_kernels.h"

struct __align__(32) KwSlot { uint64_t w0, w1; uint32_t val, info; uint64_t pad; };
struct KwSlots {
  KwSlot* s;
  uint64_t cap;   // power of two
};
struct KwRec { uint64_t w0, w1, iv; };         // partition record: key, stream position << 32 | value

struct KwLive { uint64_t w0, w1; uint32_t val, info; };
__device__ __forceinline__ KwLive kw_slot_ld(const KwSlot* p) {
  const uint4 a = *reinterpret_cast<const uint4*>(p);
  const uint2 b = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(p) + 16);
  KwLive r;
  r.w0 = (uint64_t)a.x | ((uint64_t)a.y << 32); r.w1 = (uint64_t)a.z | ((uint64_t)a.w << 32); r.val = b.x; r.info = b.y;
  return r;
}
__device__ __forceinline__ void kw_slot_st(KwSlot* p, uint64_t w0, uint64_t w1, uint32_t val, uint32_t info) {
  uint4 a, b;
  a.x = (uint32_t)w0; a.y = (uint32_t)(w0 >> 32); a.z = (uint32_t)w1; a.w = (uint32_t)(w1 >> 32);
  b.x = val; b.y = info; b.z = 0; b.w = 0;
  reinterpret_cast<uint4*>(p)[0] = a;
  reinterpret_cast<uint4*>(p)[1] = b;
}
template <int HASH>
__device__ __forceinline__ uint64_t kw_hash(uint64_t w0, uint64_t w1, uint64_t seed) { return kh_hash128<HASH>(w0, w1, seed); }

// Robin Hood find_pos (hashmap_robinhood.hpp:1058-1095) on 32-byte slots, two slots per step
__device__ __forceinline__ uint64_t kw_find_pos(const KwSlot* __restrict__ slots, uint64_t mask, uint64_t home, uint64_t w0, uint64_t w1,
                                                uint32_t* val_out) {
  uint64_t i = home;
  for (uint32_t reprobe = 0x80u; reprobe < 0x100u; reprobe += 2u) {
    const KwLive a = kw_slot_ld(slots + i);
    const KwLive b = kw_slot_ld(slots + ((i + 1) & mask));
    const uint32_t ia = a.info & 0xFFu, ib = b.info & 0xFFu;
    if (reprobe > ia) return KH_NONE;
    if (reprobe == ia && a.w0 == w0 && a.w1 == w1) { *val_out = a.val; return i; }
    if (reprobe + 1u > ib || reprobe + 1u >= 0x100u) return KH_NONE;
    if (reprobe + 1u == ib && b.w0 == w0 && b.w1 == w1) { *val_out = b.val; return (i + 1) & mask; }
    i = (i + 2) & mask;
  }
  return KH_NONE;
}

__global__ void kw_fill_empty(KwSlots T) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < T.cap; i += (uint64_t)gridDim.x * blockDim.x) kw_slot_st(T.s + i, 0, 0, 0, 0);
}
__global__ void kw_poison(KwSlots T) {      // test hook: destination buffers start as garbage
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < T.cap; i += (uint64_t)gridDim.x * blockDim.x)
    kw_slot_st(T.s + i, 0xDEADBEEFDEADBEEFull, 0xDEADBEEFDEADBEEFull, 0xDEADBEEFu, 0x000000A5u);
}

// ---------------------------------------------------------------------------------------------
// partition by chunk: exact offsets (count, scan, scatter).  The order of the records inside a partition is not kept: every
// record carries its stream position, and the fold below resolves first-wins by the smallest position.  A wave whose 64 keys
// all go to one partition (a key repeated many times) reserves with one atomic.
// ---------------------------------------------------------------------------------------------
#define KW_PART_THREADS 256
__device__ __forceinline__ uint32_t kw_wave_reserve(uint32_t q, bool active, unsigned long long* cnt64, uint32_t* cnt32) {
  const uint32_t lane = threadIdx.x & 63;
  const unsigned long long act = __ballot(active);
  if (!act) return 0;
  const uint32_t leader = (uint32_t)__ffsll((long long)act) - 1u;
  const uint32_t q0 = __shfl(q, (int)leader, 64);
  const bool all_same = __ballot(active && q != q0) == 0ull;
  if (all_same) {
    uint64_t base = 0;
    if (lane == leader) base = cnt64 ? atomicAdd(&cnt64[q0], (unsigned long long)__popcll(act)) : atomicAdd(&cnt32[q0], (uint32_t)__popcll(act));
    base = __shfl(base, (int)leader, 64);
    return (uint32_t)base + (uint32_t)__popcll(act & ((1ull << lane) - 1ull));
  }
  if (!active) return 0;
  return cnt64 ? (uint32_t)atomicAdd(&cnt64[q], 1ull) : atomicAdd(&cnt32[q], 1u);
}
template <int HASH>
__global__ __launch_bounds__(KW_PART_THREADS) void kw_part_count(const uint64_t* __restrict__ keys, uint64_t n, uint64_t seed, uint32_t PB,
                                                                 uint32_t* __restrict__ cnt) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {
    const uint64_t i = i0 + threadIdx.x;
    uint32_t q = 0;
    if (i < n) { const uint4 k = reinterpret_cast<const uint4*>(keys)[i];
                 q = kh_part_q(kw_hash<HASH>((uint64_t)k.x | ((uint64_t)k.y << 32), (uint64_t)k.z | ((uint64_t)k.w << 32), seed), PB); }
    kw_wave_reserve(q, i < n, nullptr, cnt);
  }
}
// (vals == nullptr: every value is vconst; pos0: the stream position of keys[0] -- a piece of a streamed insert)
template <int HASH>
__global__ __launch_bounds__(KW_PART_THREADS) void kw_part_scatter(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t vconst,
                                                                   uint64_t n, uint64_t seed, uint32_t PB, unsigned long long* __restrict__ cursor,
                                                                   KwRec* __restrict__ rec, uint32_t pos0 = 0) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {
    const uint64_t i = i0 + threadIdx.x;
    uint64_t w0 = 0, w1 = 0; uint32_t q = 0, v = vconst;
    if (i < n) {
      const uint4 k = reinterpret_cast<const uint4*>(keys)[i];
      w0 = (uint64_t)k.x | ((uint64_t)k.y << 32); w1 = (uint64_t)k.z | ((uint64_t)k.w << 32);
      q = kh_part_q(kw_hash<HASH>(w0, w1, seed), PB);
      if (vals) v = vals[i];
    }
    const uint32_t pos = kw_wave_reserve(q, i < n, cursor, nullptr);
    if (i < n) { KwRec r; r.w0 = w0; r.w1 = w1; r.iv = ((uint64_t)(pos0 + (uint32_t)i) << 32) | v; rec[pos] = r; }
  }
}

// ---------------------------------------------------------------------------------------------
// kw_dedup: one workgroup per partition.  The partition's records stream through LDS in sub-tiles of one record per lane; the
// distinct keys found so far stay at the front of the staging arrays (D of them), a sub-tile is appended behind them and folded into
// an LDS index set that compares all 128 bits (the record that claims a set entry is the key's representative; every other
// occurrence merges its idx|val word into it with one 64-bit LDS atomic: min = first value wins, add = std::plus), and the sub-tile's
// new representatives are compacted behind the old ones.  One pass over the records whatever their multiplicity -- a key repeated
// 10^6 times stays ONE entry.  Only when a partition holds more than KW_DM - KW_DD_THREADS distinct keys are they split into R classes
// by a second hash and the records are swept once per class.  The distinct keys are then tested against the current table (the only
// random HBM probes) and listed: new keys at off[q] + j (nk/nv); with std::plus, the (slot, sum) pairs of keys the table already holds
// at off[q] + j (us/uv), added by kw_apply_reduce once nothing can discard the attempt.  Any other Reducer (rop: min, max, or) folds with
// one 32-bit LDS atomic on the value word of idx|val and is listed the same way.
// LDS: 3 x 8 B x KW_DM staging + 4 B x KW_HS set = 64 KB + a few words: two 512-lane workgroups per CU (4 waves per SIMD).
// ---------------------------------------------------------------------------------------------
#define KW_DD_THREADS 512
#define KW_DM 2048u
#define KW_HS 4096u
struct KwDedupParams {
  const KwRec* rec; const uint64_t* off;       // partition q = rec[off[q], off[q+1])
  KwSlots T; uint64_t seed; int table_empty; int mode;      // KH_DEDUP_FIRST / KH_DEDUP_PLUS
  int rop;                                                   // KH_DEDUP_PLUS: the Reducer (KH_ROP_*)
  uint64_t* nk; uint32_t* nv; uint32_t* cnt_new;            // new distinct keys (2 words each) + value
  uint64_t* us; uint32_t* uv; uint32_t* cnt_upd;            // std::plus: existing keys' slot + sum
  unsigned long long* max_idx_plus1;
  uint32_t* flags;
};
__device__ __forceinline__ uint32_t kw_set_hash(uint64_t w0, uint64_t w1) { return (uint32_t)kh_fmix64(w0 ^ kh_fmix64(w1 + 0x9E3779B97F4A7C15ull)); }
template <int HASH>
__global__ __launch_bounds__(KW_DD_THREADS) void kw_dedup(KwDedupParams P) {
  __shared__ uint64_t l0[KW_DM], l1[KW_DM], liv[KW_DM];
  __shared__ uint32_t set[KW_HS];
  __shared__ uint32_t s_cnt, s_out, s_upd, s_max;
  const uint32_t tid = threadIdx.x, q = blockIdx.x;
  const uint64_t beg = P.off[q];
  const uint32_t m = (uint32_t)(P.off[q + 1] - beg);
  const KwRec* R0 = P.rec + beg;
  const uint64_t mask = P.T.cap - 1;
  const int fold = kh_fold_mode(P.mode, P.rop);      // (uniform over the launch: the fold below branches on a scalar)
  if (m == 0) { if (tid == 0) { P.cnt_new[q] = 0; if (P.cnt_upd) P.cnt_upd[q] = 0; } return; }
  for (uint32_t R = 1;; R *= 2) {
    if (tid == 0) { s_out = 0; s_upd = 0; s_max = 0; }
    bool over = false;                 // (workgroup-uniform: D is)
    for (uint32_t r = 0; r < R && !over; ++r) {
      for (uint32_t s = tid; s < KW_HS; s += KW_DD_THREADS) set[s] = 0;
      uint32_t D = 0;
      __syncthreads();
      for (uint32_t pos = 0; pos < m; pos += KW_DD_THREADS) {
        if (D + KW_DD_THREADS > KW_DM) { over = true; break; }
        const uint32_t i = pos + tid;
        KwRec rr; rr.w0 = 0; rr.w1 = 0; rr.iv = 0;
        bool take = false;
        if (i < m) { rr = R0[i]; take = R == 1 || (kw_set_hash(rr.w1, rr.w0) >> 7) % R == r; }
        if (tid == 0) s_cnt = D;
        __syncthreads();
        const uint32_t x = kh_wave_append(take, &s_cnt);
        if (take) { l0[x] = rr.w0; l1[x] = rr.w1; liv[x] = rr.iv; }
        __syncthreads();
        // fold: claim a set entry or merge into the key's representative
        bool rep = false; uint32_t myslot = 0;
        if (take) {
          uint32_t slot = kw_set_hash(rr.w0, rr.w1) & (KW_HS - 1);
          for (;;) {
            const uint32_t cur = atomicCAS(&set[slot], 0u, x + 1u);
            if (cur == 0) { rep = true; myslot = slot; break; }
            const uint32_t o = cur - 1u;
            if (l0[o] == rr.w0 && l1[o] == rr.w1) {
              if (fold == KH_DEDUP_PLUS) atomicAdd((unsigned long long*)&liv[o], (unsigned long long)(rr.iv & 0xFFFFFFFFull));
              else if (fold == KH_DEDUP_FIRST) atomicMin((unsigned long long*)&liv[o], (unsigned long long)rr.iv);
              else {       // value word alone (low word, little endian); the index word stays the representative's
                uint32_t* const vw = reinterpret_cast<uint32_t*>(&liv[o]);
                if (fold == KH_FOLD_MIN) atomicMin(vw, (uint32_t)rr.iv);
                else if (fold == KH_FOLD_MAX) atomicMax(vw, (uint32_t)rr.iv);
                else atomicOr(vw, (uint32_t)rr.iv);
              }
              break;
            }
            slot = (slot + 1) & (KW_HS - 1);
          }
        }
        __syncthreads();
        // compact this sub-tile's representatives behind the D older ones (their set entries follow them)
        uint64_t iv = 0;
        if (rep) iv = liv[x];
        if (tid == 0) s_cnt = D;
        __syncthreads();
        const uint32_t nx = kh_wave_append(rep, &s_cnt);
        __syncthreads();
        if (rep) { l0[nx] = rr.w0; l1[nx] = rr.w1; liv[nx] = iv; set[myslot] = nx + 1u; }
        D = s_cnt;
        __syncthreads();
      }
      if (over) break;
      // the distinct keys of this class: membership test, then the lists
      uint32_t my_max = 0;
      for (uint32_t x0 = 0; x0 < D; x0 += KW_DD_THREADS) {
        const uint32_t x = x0 + tid;
        bool emit = false, upd = false;
        uint64_t w0 = 0, w1 = 0, iv = 0, at = KH_NONE;
        if (x < D) {
          w0 = l0[x]; w1 = l1[x]; iv = liv[x];
          uint32_t cv = 0;
          if (!P.table_empty) at = kw_find_pos(P.T.s, mask, kw_hash<HASH>(w0, w1, P.seed) & mask, w0, w1, &cv);
          upd = at != KH_NONE && P.mode == KH_DEDUP_PLUS;
          emit = at == KH_NONE;
        }
        const uint32_t up = kh_wave_append(upd, &s_upd);
        if (upd) { P.us[beg + up] = at; P.uv[beg + up] = (uint32_t)iv; }
        const uint32_t op = kh_wave_append(emit, &s_out);
        if (emit) {
          P.nk[2 * (beg + op)] = w0; P.nk[2 * (beg + op) + 1] = w1; P.nv[beg + op] = (uint32_t)iv;
          const uint32_t ix = (uint32_t)(iv >> 32) + 1u;
          my_max = ix > my_max ? ix : my_max;
        }
      }
      my_max = kh_wave_max(my_max);
      if ((tid & 63) == 0 && my_max) atomicMax(&s_max, my_max);
      __syncthreads();
    }
    __syncthreads();
    if (!over) break;
    if (R > 2 * m + 2) { if (tid == 0) atomicOr(&P.flags[KH_FLAG_INTERNAL], 1u); break; }
    __syncthreads();
  }
  if (tid == 0) {
    P.cnt_new[q] = s_out;
    if (P.cnt_upd) P.cnt_upd[q] = s_upd;
    if (s_out && P.mode == KH_DEDUP_FIRST) atomicMax(P.max_idx_plus1, (unsigned long long)s_max);
  }
}
// the Reducer applied to keys the table already holds.  std::plus: sign +1 adds the listed sums, -1 takes them back (the re-layout that
// followed failed).  min / max / or cannot be taken back from the result: sign +1 stores op(stored, listed reduction) and leaves the
// PREVIOUS stored value in the list entry it consumed; sign -1 stores those back.  Every slot is in at most one entry: no race.
__global__ void kw_apply_reduce(KwSlot* __restrict__ slots, const uint64_t* __restrict__ off, const uint32_t* __restrict__ cnt_upd,
                                const uint64_t* __restrict__ us, uint32_t* __restrict__ uv, uint32_t nparts, int sign, int rop) {
  for (uint32_t q = blockIdx.x; q < nparts; q += gridDim.x) {
    const uint64_t b = off[q];
    const uint32_t c = cnt_upd[q];
    for (uint32_t j = threadIdx.x; j < c; j += blockDim.x) {
      const uint32_t d = uv[b + j];
      const uint64_t at = us[b + j];
      if (rop == KH_ROP_PLUS) slots[at].val += sign > 0 ? d : (0u - d);
      else if (sign > 0) { const uint32_t old = slots[at].val; slots[at].val = kh_reduce(old, d, rop); uv[b + j] = old; }
      else slots[at].val = d;
    }
  }
}
// the per-partition lists of new keys gathered into one dense list (partition order)
__global__ void kw_gather_new(const uint64_t* __restrict__ part_off, const uint64_t* __restrict__ noff, const uint64_t* __restrict__ nk,
                              const uint32_t* __restrict__ nv, uint64_t* __restrict__ ck, uint32_t* __restrict__ cv) {
  const uint32_t q = blockIdx.x;
  const uint64_t src = part_off[q], dst = noff[q];
  const uint32_t c = (uint32_t)(noff[q + 1] - dst);
  for (uint32_t i = threadIdx.x; i < c; i += blockDim.x) {
    ck[2 * (dst + i)] = nk[2 * (src + i)]; ck[2 * (dst + i) + 1] = nk[2 * (src + i) + 1]; cv[dst + i] = nv[src + i];
  }
}

// ---------------------------------------------------------------------------------------------
// re-layout into a fresh buffer: kw_chunk_count (home counts + the chunk's (max,+) summary) -> k_chunk_carry (key-agnostic, shared
// with the 64-bit table) -> kw_chunk_place (the chunk's slice assembled in LDS and streamed out; every destination slot written once)
// ---------------------------------------------------------------------------------------------
struct KwRebuildParams {
  KwSlots Old; int drop_marked; KwSlots New;
  const uint64_t* ck; const uint32_t* cv;   // new distinct elements (2 words per key), grouped by partition
  const uint64_t* noff;                     // [nparts+1] start of every partition's list (null: no new elements)
  const uint32_t* ncnt;                     // per-partition list length; null: dense lists (length = noff[q+1]-noff[q])
  uint32_t PB;
  uint64_t seed;
  uint16_t* homecnt; long long* sumA; long long* sumN; const long long* xcarry;
  uint32_t* flags;
};
// f(w0, w1, val, home_new) for every live element of the OLD table whose new home lies in new chunk c (cf. kh_for_each_old)
template <int HASH, typename F>
__device__ __forceinline__ void kw_for_each_old(const KwRebuildParams& P, uint32_t c, F f) {
  if (P.Old.cap == 0) return;
  const uint64_t cap_o = P.Old.cap, mask_o = cap_o - 1, mask_n = P.New.cap - 1;
  const uint32_t nch_o = cap_o > KH_L ? (uint32_t)(cap_o >> KH_LB) : 1u;
  const uint32_t nch_n = P.New.cap > KH_L ? (uint32_t)(P.New.cap >> KH_LB) : 1u;
  const uint32_t Lo = cap_o > KH_L ? KH_L : (uint32_t)cap_o;
  uint32_t o = nch_o >= nch_n ? c : (c & (nch_o - 1));
  const uint32_t ostep = nch_o >= nch_n ? nch_n : nch_o;
  for (; o < nch_o; o += ostep) {
    const uint64_t S = (uint64_t)o * Lo;
    const uint64_t beyond = cap_o - Lo;
    const uint64_t len = (uint64_t)Lo + (beyond < 128u ? beyond : 128u);      // Robin Hood: probe distance <= 127
    for (uint64_t t = threadIdx.x; t < len; t += KW_DD_THREADS) {
      const KwLive w = kw_slot_ld(P.Old.s + ((S + t) & mask_o));
      if ((w.info & 0xFFu) < 0x80u) continue;
      if (P.drop_marked && (w.info & KH_INFO_ERASE_MARK)) continue;
      const uint64_t h = kw_hash<HASH>(w.w0, w.w1, P.seed);
      if ((uint32_t)((h & mask_o) >> KH_LB) != o) continue;
      if ((uint32_t)((h & mask_n) >> KH_LB) != c) continue;
      f(w.w0, w.w1, w.val, h & mask_n);
    }
    if (nch_o < nch_n) break;
  }
}
template <int HASH, typename F>
__device__ __forceinline__ void kw_for_each_new(const KwRebuildParams& P, uint32_t c, F f) {
  if (!P.noff) return;
  const uint64_t mask_n = P.New.cap - 1;
  const uint32_t nch_n = P.New.cap > KH_L ? (uint32_t)(P.New.cap >> KH_LB) : 1u;
  const uint32_t k = kh_log2u(nch_n);
  const uint32_t span_bits = P.PB - k;
  const uint32_t q0 = k ? ((__brev(c) >> (32 - k)) << span_bits) : 0u;
  const uint32_t q1 = q0 + (1u << span_bits);
  if (!P.ncnt) {
    const uint64_t b = P.noff[q0], e = P.noff[q1];
    for (uint64_t i = b + threadIdx.x; i < e; i += KW_DD_THREADS) {
      const uint64_t w0 = P.ck[2 * i], w1 = P.ck[2 * i + 1];
      f(w0, w1, P.cv[i], kw_hash<HASH>(w0, w1, P.seed) & mask_n);
    }
  } else {
    for (uint32_t q = q0; q < q1; ++q) {
      const uint64_t b = P.noff[q];
      const uint32_t n = P.ncnt[q];
      for (uint32_t i = threadIdx.x; i < n; i += KW_DD_THREADS) {
        const uint64_t w0 = P.ck[2 * (b + i)], w1 = P.ck[2 * (b + i) + 1];
        f(w0, w1, P.cv[b + i], kw_hash<HASH>(w0, w1, P.seed) & mask_n);
      }
    }
  }
}
#define KW_HOMES_PER_THREAD (KH_L / KW_DD_THREADS)
template <int HASH>
__global__ __launch_bounds__(KW_DD_THREADS) void kw_chunk_count(KwRebuildParams P) {
  __shared__ uint32_t cnt[KH_L];
  __shared__ KhMP s_wtot[KW_DD_THREADS / 64];
  const uint32_t tid = threadIdx.x, c = blockIdx.x;
  const uint32_t Ln = P.New.cap > KH_L ? KH_L : (uint32_t)P.New.cap;
  const uint64_t Sc = (uint64_t)c * Ln;
  for (uint32_t i = tid; i < KH_L; i += KW_DD_THREADS) cnt[i] = 0;
  __syncthreads();
  kw_for_each_old<HASH>(P, c, [&](uint64_t, uint64_t, uint32_t, uint64_t hn) { atomicAdd(&cnt[hn - Sc], 1u); });
  kw_for_each_new<HASH>(P, c, [&](uint64_t, uint64_t, uint32_t, uint64_t hn) { atomicAdd(&cnt[hn - Sc], 1u); });
  __syncthreads();
  KhMP v; v.A = KH_MP_NEG; v.n = 0;
#pragma unroll
  for (uint32_t j = 0; j < KW_HOMES_PER_THREAD; ++j) {
    const uint32_t b = tid * KW_HOMES_PER_THREAD + j;
    if (b < Ln) {
      uint32_t cb = cnt[b];
      if (cb > 0xFFFFu) { atomicOr(&P.flags[KH_FLAG_COUNT_OVERFLOW], 1u); cb = 0xFFFFu; }
      P.homecnt[Sc + b] = (uint16_t)cb;
      KhMP h; h.A = (long long)b + cb; h.n = cb;
      v = kh_mp_combine(v, h);
    }
  }
  KhMP total;
  kh_block_scan_mp(v, s_wtot, &total);
  if (tid == 0) { P.sumA[c] = (long long)Sc + total.A; P.sumN[c] = total.n; }
}
// LDS: (16 + 4 + 1) B x (KH_L + KH_SPILL) staging + 2 x 4 B x KH_L cursors = 56.4 KB: two workgroups per CU
template <int HASH>
__global__ __launch_bounds__(KW_DD_THREADS) void kw_chunk_place(KwRebuildParams P) {
  __shared__ uint64_t s0[KH_L + KH_SPILL], s1[KH_L + KH_SPILL];
  __shared__ uint32_t sval[KH_L + KH_SPILL];
  __shared__ uint32_t sinfo_w[(KH_L + KH_SPILL) / 4];
  __shared__ uint32_t fill[KH_L];
  __shared__ uint32_t start[KH_L];
  __shared__ long long s_pend;
  __shared__ KhMP s_wtot[KW_DD_THREADS / 64];
  uint8_t* sinfo = reinterpret_cast<uint8_t*>(sinfo_w);
  const uint32_t tid = threadIdx.x, c = blockIdx.x;
  const uint32_t Ln = P.New.cap > KH_L ? KH_L : (uint32_t)P.New.cap;
  const uint64_t Sc = (uint64_t)c * Ln, mask_n = P.New.cap - 1;
  for (uint32_t i = tid; i < KH_L + KH_SPILL; i += KW_DD_THREADS) { s0[i] = 0; s1[i] = 0; sval[i] = 0; }
  for (uint32_t i = tid; i < (KH_L + KH_SPILL) / 4; i += KW_DD_THREADS) sinfo_w[i] = 0;
  uint32_t cb[KW_HOMES_PER_THREAD];
  KhMP v; v.A = KH_MP_NEG; v.n = 0;
#pragma unroll
  for (uint32_t j = 0; j < KW_HOMES_PER_THREAD; ++j) {
    const uint32_t b = tid * KW_HOMES_PER_THREAD + j;
    cb[j] = b < Ln ? P.homecnt[Sc + b] : 0u;
    if (b < Ln) { KhMP h; h.A = (long long)b + cb[j]; h.n = cb[j]; v = kh_mp_combine(v, h); }
    fill[b] = 0;
  }
  const KhMP excl = kh_block_scan_mp(v, s_wtot, nullptr);
  const long long xr = P.xcarry[c] - (long long)Sc;
  long long p = excl.A > xr + excl.n ? excl.A : xr + excl.n;
#pragma unroll
  for (uint32_t j = 0; j < KW_HOMES_PER_THREAD; ++j) {
    const uint32_t b = tid * KW_HOMES_PER_THREAD + j;
    if (b < Ln) {
      const long long st = p > (long long)b ? p : (long long)b;
      start[b] = (uint32_t)st;
      p = st + cb[j];
    }
  }
  if (tid == KW_DD_THREADS - 1) s_pend = p;
  __syncthreads();
  auto place = [&](uint64_t w0, uint64_t w1, uint32_t val, uint64_t hn) {
    const uint32_t b = (uint32_t)(hn - Sc);
    const uint32_t r = atomicAdd(&fill[b], 1u);
    const uint32_t prel = start[b] + r;
    uint32_t dist = prel - b;
    if (dist > 127u) { atomicOr(&P.flags[KH_FLAG_PROBE_OVERFLOW], 1u); dist = 127u; }
    const uint8_t ib = (uint8_t)(0x80u | dist);
    if (prel < KH_L + KH_SPILL) { s0[prel] = w0; s1[prel] = w1; sval[prel] = val; sinfo[prel] = ib; }
    else kw_slot_st(P.New.s + ((Sc + prel) & mask_n), w0, w1, val, ib);
  };
  kw_for_each_old<HASH>(P, c, place);
  kw_for_each_new<HASH>(P, c, place);
  __syncthreads();
  long long pend = s_pend;
  if (pend < (long long)Ln) pend = Ln;
  const uint32_t lo = xr > 0 ? (uint32_t)xr : 0u;
  const uint32_t hi = pend < (long long)(KH_L + KH_SPILL) ? (uint32_t)pend : (KH_L + KH_SPILL);
  for (uint32_t x = lo + tid; x < hi; x += KW_DD_THREADS) kw_slot_st(P.New.s + ((Sc + x) & mask_n), s0[x], s1[x], sval[x], sinfo[x]);
}

// ---------------------------------------------------------------------------------------------
// batch erase, fall-back form of the 64-bit table: mark the hits (first mark of a slot counts), then the re-layout drops them
// ---------------------------------------------------------------------------------------------
template <int HASH>
__global__ __launch_bounds__(256) void kw_erase_mark(KwSlots T, const uint64_t* __restrict__ q, uint64_t n, uint64_t seed,
                                                     unsigned long long* __restrict__ n_marked) {
  const uint64_t mask = T.cap - 1;
  uint32_t c = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t w0 = q[2 * i], w1 = q[2 * i + 1];
    uint32_t v;
    const uint64_t at = kw_find_pos(T.s, mask, kw_hash<HASH>(w0, w1, seed) & mask, w0, w1, &v);
    if (at != KH_NONE && !(atomicOr(&T.s[at].info, KH_INFO_ERASE_MARK) & KH_INFO_ERASE_MARK)) ++c;
  }
  c = kh_wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(n_marked, (unsigned long long)c);
}
__global__ void kw_clear_marks(KwSlots T) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < T.cap; i += (uint64_t)gridDim.x * blockDim.x) T.s[i].info &= 0xFFu;
}

// ---------------------------------------------------------------------------------------------
// kw_find: every lane owns KW_Q_ITEMS queries (strided by the grid, coalesced); the first two-slot step of all of them is requested
// before any is looked at, the rare longer probes continue one by one.  OUT: per-query value + found flag (the flags also feed the
// compaction of find(Iter,Iter)), or 0/1 counts.
// ---------------------------------------------------------------------------------------------
#define KW_Q_THREADS 256
#define KW_Q_ITEMS 4
enum { KW_FIND_VALS = 0, KW_FIND_COUNT = 1 };
template <int HASH, int OUT>
__global__ __launch_bounds__(KW_Q_THREADS) void kw_find(KwSlots T, const uint64_t* __restrict__ q, uint64_t n, uint64_t seed,
                                                        uint32_t* __restrict__ out_vals, uint8_t* __restrict__ out_found,
                                                        unsigned long long* __restrict__ n_found) {
  const uint64_t mask = T.cap - 1;
  const uint64_t span = (uint64_t)gridDim.x * KW_Q_THREADS;
  uint32_t hits = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * KW_Q_THREADS + threadIdx.x; base < n; base += span * KW_Q_ITEMS) {
    uint64_t w0[KW_Q_ITEMS], w1[KW_Q_ITEMS], home[KW_Q_ITEMS];
    KwLive a[KW_Q_ITEMS], b[KW_Q_ITEMS];
#pragma unroll
    for (int j = 0; j < KW_Q_ITEMS; ++j) {
      const uint64_t i = base + j * span;
      w0[j] = 0; w1[j] = 0; home[j] = 0;
      if (i < n) { const uint4 k = reinterpret_cast<const uint4*>(q)[i];
                   w0[j] = (uint64_t)k.x | ((uint64_t)k.y << 32); w1[j] = (uint64_t)k.z | ((uint64_t)k.w << 32);
                   home[j] = kw_hash<HASH>(w0[j], w1[j], seed) & mask; }
    }
#pragma unroll
    for (int j = 0; j < KW_Q_ITEMS; ++j) { a[j] = kw_slot_ld(T.s + home[j]); b[j] = kw_slot_ld(T.s + ((home[j] + 1) & mask)); }
#pragma unroll
    for (int j = 0; j < KW_Q_ITEMS; ++j) {
      const uint64_t i = base + j * span;
      if (i >= n) continue;
      const uint32_t ia = a[j].info & 0xFFu, ib = b[j].info & 0xFFu;
      bool found = false; uint32_t val = 0;
      if (ia == 0x80u && a[j].w0 == w0[j] && a[j].w1 == w1[j]) { found = true; val = a[j].val; }
      else if (ia >= 0x80u && ib == 0x81u && b[j].w0 == w0[j] && b[j].w1 == w1[j]) { found = true; val = b[j].val; }
      else if (ia >= 0x80u && ib >= 0x81u) {          // the key may sit further out
        const uint64_t at = kw_find_pos(T.s, mask, home[j], w0[j], w1[j], &val);
        found = at != KH_NONE;
      }
      if (OUT == KW_FIND_VALS) { out_found[i] = found ? 1 : 0; if (found && out_vals) out_vals[i] = val; }
      else out_found[i] = found ? 1 : 0;
      hits += found ? 1u : 0u;
    }
  }
  if (n_found) {
    hits = kh_wave_sum(hits);
    if ((threadIdx.x & 63) == 0 && hits) atomicAdd(n_found, (unsigned long long)hits);
  }
}
// compaction of flagged queries (find(Iter,Iter) in query order, to_vector): tiles of KH_CMP_TILE after k_flag_tile_sums +
// k_scan_u32_to_u64; lane t owns 8 consecutive entries
__global__ __launch_bounds__(256) void kw_compact(const uint8_t* __restrict__ flags, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                  uint64_t n, const uint64_t* __restrict__ tile_off, uint64_t* __restrict__ out_keys, uint32_t* __restrict__ out_vals) {
  __shared__ uint32_t wtot[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * KH_CMP_TILE + (uint64_t)tid * 8;
  uint32_t fm = 0;
  for (int j = 0; j < 8; ++j) if (base + j < n && flags[base + j]) fm |= 1u << j;
  const uint32_t c = (uint32_t)__popc(fm);
  uint32_t incl = c;
  for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(incl, off, 64); if (lane >= (uint32_t)off) incl += o; }
  if (lane == 63) wtot[wid] = incl;
  __syncthreads();
  uint64_t x = tile_off[blockIdx.x] + incl - c;
  for (uint32_t w = 0; w < wid; ++w) x += wtot[w];
  for (int j = 0; j < 8; ++j) {
    if ((fm >> j) & 1u) {
      out_keys[2 * x] = keys[2 * (base + j)]; out_keys[2 * x + 1] = keys[2 * (base + j) + 1];
      if (out_vals) out_vals[x] = vals[base + j];
      ++x;
    }
  }
}
// SoA view of the table for the exports: keys (2 words) / values / info bytes / occupied flags; any output may be null
__global__ void kw_unpack_slots(const KwSlot* __restrict__ slots, uint64_t cap, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                uint8_t* __restrict__ info, uint8_t* __restrict__ flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * blockDim.x) {
    const KwLive w = kw_slot_ld(slots + i);
    if (keys) { keys[2 * i] = w.w0; keys[2 * i + 1] = w.w1; }
    if (vals) vals[i] = w.val;
    if (info) info[i] = (uint8_t)(w.info & 0xFFu);
    if (flags) flags[i] = (w.info & 0xFFu) >= 0x80u ? 1 : 0;
  }
}
__global__ void kw_disp_hist(const KwSlot* __restrict__ slots, uint64_t cap, unsigned long long* __restrict__ out128) {
  __shared__ uint32_t h[128];
  if (threadIdx.x < 128) h[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t b = slots[i].info & 0xFFu;
    if (b >= 0x80u) atomicAdd(&h[b & 0x7Fu], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 128 && h[threadIdx.x]) atomicAdd(&out128[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------
// 128-bit k-mers (k = 1..64): the second pass of the k-mer front end (kh_kernels.h: tile layout, KhKm<2> windows, k_kmers_count<2>, scan)
// for 16-byte k-mers: every lane writes its windows straight to their place, one 16-byte store each (k_kmers_emit stages its tile in LDS).
// ---------------------------------------------------------------------------------------------
template <bool CANON>
__global__ __launch_bounds__(KH_KM_THREADS) void kw_kmers_emit(const uint8_t* __restrict__ seq, uint64_t n, uint32_t k, const uint64_t* __restrict__ tile_off,
                                                               uint64_t* __restrict__ out) {
  typedef KhKm<2> M;
  __shared__ uint32_t words[KH_KM_TILE / 16 + M::HALO];
  __shared__ uint16_t invs[KH_KM_TILE / 16 + M::HALO];
  __shared__ uint32_t wtot[KH_KM_THREADS / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  kh_km_pack_tile<M::HALO>(seq, n, (uint64_t)blockIdx.x * KH_KM_TILE, words, invs);
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
      reinterpret_cast<ulonglong2*>(out)[pos++] = make_ulonglong2(w0, w1);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// HyperLogLog straight from text: text -> tile (kh_km_pack_tile) -> the 16 windows of the lane's word -> validity -> forward k-mer ->
// canonical form -> hash (KhKm<KW>::hash_of_window) -> register (kh_hll_put, as k_hll_update does it).  Reads 1 B per base and writes
// nothing but the 2^precision registers: the k-mers (8 or 16 B per window) never reach HBM.  Workgroups are persistent: the host launches
// min(tiles, KH_HLL_TEXT_WGS_PER_CU x CUs) of them, each loops grid-stride over the 4096-position tiles, keeps its registers in LDS over
// ALL its tiles and merges them into the global registers once at the end (a merge per tile would cost up to one global atomic per
// window).  LDS per workgroup: 4 x 2^precision B of registers (16 KB at the default precision 12, 32 KB at 13) + 1.6 KB of tile words,
// so four 256-lane workgroups fit a CU (4 waves per SIMD, <= 128 VGPRs) at every precision that uses LDS; above 13 the registers are
// updated in global memory.  No workgroup waits for another: a grid that is not fully resident is merely slower.
// KW = 1: k = 1..32, the hash of the 8-byte k-mer (what k_hll_update makes of k_kmers_emit's output); KW = 2: k = 33..64, the hash of the
// 16-byte k-mer {w0, w1} (of kw_kmers_emit's output).  n_windows (may be null): += the number of valid windows.
// ---------------------------------------------------------------------------------------------
#define KH_HLL_TEXT_WGS_PER_CU 4
template <int HASH, int KW, bool CANON>
__global__ __launch_bounds__(KH_KM_THREADS, 4) void k_hll_from_text(const uint8_t* __restrict__ seq, uint64_t n, uint32_t k, uint64_t seed, KhHllRegs R,
                                                                    unsigned long long* __restrict__ n_windows) {
  typedef KhKm<KW> M;
  extern __shared__ __align__(16) uint32_t kh_dyn_smem[];
  __shared__ uint32_t words[KH_KM_TILE / 16 + M::HALO];
  __shared__ uint16_t invs[KH_KM_TILE / 16 + M::HALO];
  __shared__ uint32_t wsum[KH_KM_THREADS / 64];
  kh_hll_lds_clear(R, kh_dyn_smem);
  const uint64_t lzc_mask = ~0ull >> (64 - R.precision - R.ignored);
  const uint64_t ntiles = (n + KH_KM_TILE - 1) / KH_KM_TILE;
  uint32_t cnt = 0;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();      // the previous tile's words have been read (first tile: the LDS registers are zero)
    kh_km_pack_tile<M::HALO>(seq, n, tile * KH_KM_TILE, words, invs);
    __syncthreads();
    const typename M::Win W = M::window(words, invs, threadIdx.x);
    uint32_t vmask = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) vmask |= M::valid(W, j, k) ? (1u << j) : 0u;
    cnt += (uint32_t)__popc(vmask);
    for (uint32_t j = 0; j < 16; ++j)
      if ((vmask >> j) & 1u) kh_hll_put(R, kh_dyn_smem, lzc_mask, M::template hash_of_window<HASH, CANON>(W, j, k, seed));
  }
  kh_hll_lds_flush(R, kh_dyn_smem);
  if (n_windows) {      // valid windows: summed per wave, one 64-bit atomic per workgroup
    cnt = kh_wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long tot = 0;
      for (uint32_t w = 0; w < KH_KM_THREADS / 64; ++w) tot += wsum[w];
      if (tot) atomicAdd(n_windows, tot);
    }
  }
}
