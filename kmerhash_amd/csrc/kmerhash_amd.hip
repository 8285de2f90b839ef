// kmerhash_amd.hip -- host side of libkmerhash_amd.so: table state machine + C-ABI (include/kmerhash_amd.h).
//
// Host logic restates the reference's *observable* contract (sizes, float load thresholds, the
// doubling/halving rules, first-value-wins) around the chunked GPU kernels of kh_kernels.h:
//   insert  : sample -> partition the batch by chunk -> one-launch build (k_build_fused; speculates that the capacity the
//             reference's rule yields is the predicted one) or, when a speculation fails, LDS de-dup + membership test (k_dedup)
//             -> exact capacity decision (hashmap_robinhood.hpp:530 rule, evaluated in closed form) -> chunk rebuild into a
//             fresh buffer.  The old buffer stays valid until the new one is complete, so a failing batch (probe distance >= 128)
//             leaves the table untouched.  Batches of up to 16 keys and mid-size batches are applied in place.
//   erase   : RH partitions the erase keys by chunk and drops them inside a one-launch re-layout (fall-back: mark hits, re-lay
//             out without them); LP writes tombstones in place.
//   find/count : sector probing with in-launch compaction (k_find).
//   by value : spectrum, selection and erase over a closed value range, one streaming pass over the slots each (kh_kernels_values.h).
//   index   : kh_index, all occurrences per k-mer: counting insert -> slot-order ranks + CSR offsets -> scatter -> segment sort (kh_kernels_index.h).
//             kh_windex: the same host code on a wide table (kh_index::kw == 2) and the kernels that touch a 32-byte slot (kh_kernels_index_wide.h).
//   csr     : kh_csr_unpermute, a CSR that arrives in a permuted order back into query order: the index's scans and gather around one scatter (kh_kernels_csr.h).
//   chain   : kh_chain_anchors, collinear chains per segment from flat anchors: a wavefront per segment, the last 64 anchors in registers (kh_kernels_chain.h).
//   edits   : kh_chain_edits, edit distance of every link of every kept chain: a lane per anchor, then a wavefront per unsettled link (kh_kernels_edits.h).
//   cigars  : kh_chain_cigars, the alignment operations of every link as run-length rows of a CSR: the same wavefront pass with a traceback (kh_kernels_cigar.h).
//   pair    : kh_pair_chains, the concordant chain pair of two mates, proper flag, pair quality and template length: a wavefront per pair (kh_kernels_pair.h).
//   select  : kh_chain_select, primary / secondary chains per read and a mapping quality: a wavefront per read, a workgroup for a read of more than 64 chains (kh_kernels_select.h).
//   records : kh_chain_records, one run-length row and one line of numbers per chain from the link rows, end rows and clips: a wavefront per chain; kh_cigar_text, a run CSR as text (kh_kernels_records.h).
//   targets : kh_anchor_targets, the anchors of every read regrouped by the target (contig) they fall in: a lane per anchor, then a wavefront per read (kh_kernels_targets.h).
//   sam     : kh_record_diffs, the cs or MD string of every record row: a wavefront per row along the two texts; kh_oriented_rows, byte ranges copied as they stand or back to front and complemented (kh_kernels_sam.h).
//   samtext : kh_sam_lines, the text of SAM alignment lines from line columns and byte CSRs: a wavefront per line and a lane per field in both passes, the lengths by a wave sum, the places by a wave prefix sum (kh_kernels_samtext.h).
//   fastq   : kh_fastq_records, the record structure of a FASTQ text: the line counting of kh_kmers_from_fastq, the offset of every newline, then a lane per record; kh_pack_rows, byte rows gathered to given places: a wavefront per row (kh_kernels_fastq.h).
//   ends    : kh_chain_ends, both ends of every kept chain extended to the ends of its read or to a soft clip: a wavefront per end, target free, stop by score (kh_kernels_ends.h).
#include "kh_kernels.h"
#include "kh_kernels_wide.h"
#include "kh_kernels_values.h"
#include "kh_kernels_index.h"
#include "kh_kernels_index_wide.h"
#include "kh_kernels_csr.h"
#include "kh_kernels_chain.h"
#include "kh_kernels_edits.h"
#include "kh_kernels_cigar.h"
#include "kh_kernels_ends.h"
#include "kh_kernels_select.h"
#include "kh_kernels_records.h"
#include "kh_kernels_targets.h"
#include "kh_kernels_sam.h"
#include "kh_kernels_pair.h"
#include "kh_kernels_rescue.h"
#include "kh_kernels_samtext.h"
#include "kh_kernels_fastq.h"
#include "kh_part_sizing.h"
#include "kh_scratch.h"
#include "../../include/kmerhash_amd.h"

#include <string>
#include <vector>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <unordered_map>

#define KH_VERSION_STR "kmerhash_amd 0.1 (gfx950)"

// ---- process-wide device memory cache -------------------------------------------------------------
// hipMalloc/hipFree of multi-GB buffers cost milliseconds to hundreds of milliseconds and synchronise the
// device; tables are typically created, filled and destroyed in a loop (one per benchmark repeat, one per
// file batch), so freed table buffers and workspaces are kept and handed out again (best fit).
namespace {
struct DevPool {
  std::mutex m;
  std::multimap<size_t, void*> free_;                 // size -> block
  std::unordered_map<void*, size_t> size_of;          // every live or cached block
  size_t cached = 0;
};
DevPool g_pool[16];
const size_t kPoolGranule = size_t(2) << 20;

// INVARIANT: no HIP call is made while P.m is held.  Scratch::release takes P.m on a runtime thread, in stream order, so a holder
// that sat in a synchronising call (hipFree waits for the streams of the device) would wait for the stream, the stream for the host
// function, the host function for the lock.  The blocks leave the maps under the lock and go to the driver after it is dropped.
void pool_trim(int dev) {
  DevPool& P = g_pool[dev & 15];
  std::vector<void*> drop;
  {
    std::lock_guard<std::mutex> g(P.m);
    drop.reserve(P.free_.size());
    for (auto& kv : P.free_) { drop.push_back(kv.second); P.size_of.erase(kv.second); }
    P.free_.clear();
    P.cached = 0;
  }
  for (void* p : drop) hipFree(p);
}
hipError_t pool_alloc(int dev, size_t bytes, void** out) {
  DevPool& P = g_pool[dev & 15];
  bytes = (bytes + kPoolGranule - 1) / kPoolGranule * kPoolGranule;
  {
    std::lock_guard<std::mutex> g(P.m);
    auto it = P.free_.lower_bound(bytes);
    if (it != P.free_.end() && it->first <= bytes + bytes / 4 + (size_t(16) << 20)) {
      *out = it->second;
      P.cached -= it->first;
      P.free_.erase(it);
      return hipSuccess;
    }
  }
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {            // give cached blocks back to the driver and retry once
    (void)hipGetLastError();
    pool_trim(dev);
    e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
  }
  std::lock_guard<std::mutex> g(P.m);
  P.size_of[p] = bytes;
  *out = p;
  return hipSuccess;
}
void pool_free(int dev, void* p) {
  if (!p) return;
  DevPool& P = g_pool[dev & 15];
  {
    std::lock_guard<std::mutex> g(P.m);
    auto it = P.size_of.find(p);
    if (it != P.size_of.end()) {
      P.free_.insert(std::make_pair(it->second, p));
      P.cached += it->second;
      return;
    }
  }
  hipFree(p);      // (not a pooled block; outside the lock: see the invariant at pool_trim)
}
// pinned host scratch blocks (512 B, one per table) and profiling events are recycled too: hipHostFree synchronises the
// device (0.2 ms per table destroyed, 4% of a benchmark step)
struct HostPool { std::mutex m; std::vector<uint64_t*> pinned; std::vector<hipEvent_t> events[16]; };   // events: per device
HostPool g_host;
uint64_t* pinned_get() {
  { std::lock_guard<std::mutex> g(g_host.m);
    if (!g_host.pinned.empty()) { uint64_t* p = g_host.pinned.back(); g_host.pinned.pop_back(); return p; } }
  uint64_t* p = nullptr;
  if (hipHostMalloc(reinterpret_cast<void**>(&p), 64 * sizeof(uint64_t)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}
void pinned_put(uint64_t* p) { if (p) { std::lock_guard<std::mutex> g(g_host.m); g_host.pinned.push_back(p); } }
hipEvent_t event_get(int dev) {      // the caller has made `dev` current
  { std::lock_guard<std::mutex> g(g_host.m);
    auto& v = g_host.events[dev & 15];
    if (!v.empty()) { hipEvent_t e = v.back(); v.pop_back(); return e; } }
  hipEvent_t e = nullptr;
  hipEventCreate(&e);
  return e;
}
void event_put(int dev, hipEvent_t e) { if (e) { std::lock_guard<std::mutex> g(g_host.m); g_host.events[dev & 15].push_back(e); } }
}  // namespace

namespace {

struct ProfRec { const char* name; hipEvent_t a, b; };

struct Block { char* p; size_t cap; };

}  // namespace

// histogram-free layout shared by the pieces of a streamed insert: every piece appends to the SAME slots (cursors, overflow flag
// and the final buffer live across the feeds), so that the build at the end sees one source
struct SlackShared { unsigned long long* cur2; uint64_t* starts; uint32_t* ovf; uint64_t slot; };
// a slot buffer of either key width: typed (KhSlots / KwSlots) where it is made and where a kernel is launched -- narrow() / wide()
struct SlotBuf {
  void* p; uint64_t cap;
  SlotBuf() : p(nullptr), cap(0) {}
  SlotBuf(KhSlots s) : p(s.s), cap(s.cap) {}
  SlotBuf(KwSlots s) : p(s.s), cap(s.cap) {}
};
// state of a table of either key width (kh_wtable below: the same state with 32-byte slots)
struct kh_table {
  int kind = KHK_RH, hash = 0, device = 0;
  KhSeed seed = KhSeed{0, 0u};      // storage hash seed + key transform (kh_set_key_transform)
  hipStream_t stream = nullptr;
  float min_lf = 0.f, max_lf = 0.f;
  uint64_t min_load = 0, max_load = 0, lsize = 0;
  uint32_t slot_bytes = sizeof(KhSlot);      // sizeof(KwSlot): a wide table
  SlotBuf cur, spare;
  // workspace arena (grow-only, reset per operation)
  std::vector<Block> blocks;
  size_t blk = 0, off = 0;
  uint64_t* hpin = nullptr;   // pinned host scratch (64 x u64)
  std::string err;
  // streamed insert (kh_insert_begin / feed / end)
  struct {
    bool active, fallback, nodup; int mode;       // nodup: a sample of the FIRST feed found no duplicate key (the build then skips its fold, speculatively)
    // KH_INS_REPEATABLE: the caller can feed the same pieces again, so the speculative forms are allowed: histogram-free partition
    // into slots shared by all pieces (one source for the build), 12-byte records when the sample found no duplicate
    bool repeatable, slack, rec12;
    SlackShared sh;
    uint64_t n_total, fed, cap_u; uint32_t PB;
    ulonglong2 *tmp, *fin;
    KhSrcSet S;
    uint64_t* stage_k; uint32_t* stage_v;
    // wide table: the pieces fed so far (device pointers: the caller's, or workspace copies of host pieces) and the per-partition
    // counters every feed's kw_part_count adds to
    const uint64_t* wk[KH_MAX_SRC]; const uint32_t* wv[KH_MAX_SRC]; uint64_t wn[KH_MAX_SRC]; uint32_t wsrc; uint32_t* wcnt;
  } ins = {};
  uint32_t* part_overflow = nullptr;      // device flag of the histogram-free partition feeding the operation in flight (or null)
  double batch_vf = 1.0;                  // variance factor E[m^2]/E[m] the duplicate sample gave for the batch in flight (1: no duplicate seen)
  bool batch_nodup = false;               // a sample of the batch in flight found no duplicate key (k_sample_dups)
  // optimistic attempt in flight (insert_core): queued behind the sample without reading it.  sample_dups: the sample's device word, which
  // the kernels of the attempt test and launch_fused brings to the host; fused_blk: launch_fused's control block, zeroed by the same fill
  // as the sample set (fused_blk_bytes long)
  uint32_t* sample_dups = nullptr;
  char* fused_blk = nullptr; size_t fused_blk_bytes = 0;
  bool prof = false;
  std::vector<ProfRec> recs;
  std::vector<std::pair<std::string, std::pair<double, uint64_t> > > prof_acc;
};
struct kh_wtable : kh_table {};      // a distinct handle type for the C header; its kernels differ (kh_kernels_wide.h), its host state does not

namespace {

inline uint64_t next_pow2(uint64_t x) {   // math_utils.hpp:64-69 (x<=1 -> 1)
  if (x <= 1) return 1;
  return uint64_t(1) << (64 - __builtin_clzll(x - 1));
}
inline uint64_t threshold(uint64_t buckets, float lf) {   // hashmap_robinhood.hpp:263,269: float arithmetic
  return static_cast<uint64_t>(static_cast<float>(buckets) * lf);
}
inline uint32_t log2u(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }

kh_status fail(kh_table* t, kh_status s, const std::string& msg) {
  if (t) t->err = msg;
  return s;
}
// the one mapping of a HIP error to a status
inline kh_status hip_status(hipError_t e) { return e == hipSuccess ? KH_OK : e == hipErrorOutOfMemory ? KH_ERR_NOMEM : KH_ERR_HIP; }
kh_status hip_fail(kh_table* t, const char* call, hipError_t e) {
  if (t) t->err = std::string(call) + ": " + hipGetErrorString(e);
  return hip_status(e);
}
// The wide-key alignment rule (kmerhash_amd.h, "wide keys"): the kernels read a 16-byte key with one dwordx4 load, so an entry point
// refuses a device array of 16-byte keys that is not 16-byte aligned before it launches or changes anything.  kw: 64-bit words per key
// (8-byte keys pass); host arrays pass at any alignment, they are staged into aligned device memory.
inline bool wide_keys_aligned(uint32_t kw, const void* keys, kh_mem where) {
  return kw != 2 || where != KH_MEM_DEVICE || (reinterpret_cast<uintptr_t>(keys) & 15u) == 0;
}
const char* const kWideKeysMisaligned = "a device array of 16-byte keys must be 16-byte aligned";
// HIPCHK: in a function with a table `t` in scope, whose error text it sets; HIPCHK0: where there is no table
#define HIPCHK_T(table, call)                                                                          \
  do {                                                                                                 \
    hipError_t e__ = (call);                                                                           \
    if (e__ != hipSuccess) return hip_fail(table, #call, e__);                                         \
  } while (0)
#define HIPCHK(call) HIPCHK_T(t, call)
#define HIPCHK0(call) HIPCHK_T(nullptr, call)

inline int cu_count(int device) {
  int ncu = 256;
  hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
  return ncu > 0 ? ncu : 256;
}
inline int cu_count(const kh_table* t) { return cu_count(t->device); }

// ---- scratch of one handle-free call ---------------------------------------------------------------
// Bound to (device, stream), which the caller has made current.  The call describes its block once, as a function of the scratch
// (layout(): kh_scratch.h's two passes), with take() for temporaries and in() / out() for arrays that live where `where` says: device
// memory is used as it is, host memory gets a carved copy -- in() queues the copy in, copy_back() the copy out.  The first HIP error
// sticks and turns the later copies into no-ops.  finish(), also run by the destructor on every early return, waits for the stream
// if a block or a host copy of this call may still be in use, returns the blocks to the pool and maps the error.
class Scratch {
 public:
  Scratch(int device, hipStream_t stream) : device_(device), stream_(stream) {}
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() { finish(); }

  hipError_t error() const { return err_; }
  bool ok() const { return err_ == hipSuccess; }
  void check(hipError_t e) { if (err_ == hipSuccess) err_ = e; }
  // after kernel launches: their launch error, and the blocks are in use again
  bool launched() { check(hipGetLastError()); busy_ = true; return ok(); }

  // a pooled block of its own (null: the error is set)
  void* alloc(size_t bytes) {
    void* p = nullptr;
    if (ok() && nblk_ == kMaxBlocks) err_ = hipErrorInvalidValue;
    if (ok()) err_ = pool_alloc(device_, bytes, &p);
    if (!ok()) return nullptr;
    blk_[nblk_++] = p;
    busy_ = true;
    return p;
  }
  // the bytes `layout` takes; the same layout over a block the caller owns (a persistent workspace); both over a pooled block
  template <typename F> size_t measure(F&& layout) { car_ = KhCarver(); layout(*this); return car_.size(); }
  template <typename F> void carve(void* base, F&& layout) { car_ = KhCarver(base); layout(*this); }
  template <typename F> bool layout(F&& layout) {
    const size_t bytes = measure(layout);
    void* p = bytes ? alloc(bytes) : nullptr;
    if (bytes && !p) return false;
    carve(p, layout);      // (no bytes: nothing is staged, the caller's pointers pass through)
    return ok();
  }
  // inside a layout function
  template <typename T> T* take(uint64_t count) { return car_.take<T>(count); }
  template <typename T> const T* in(const T* p, uint64_t count, kh_mem where) {
    if (where != KH_MEM_HOST) return p;
    T* d = car_.take<T>(count);
    if (d) copy(d, p, count * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  template <typename T> T* out(T* p, uint64_t count, kh_mem where) {
    if (where != KH_MEM_HOST) return p;
    T* d = car_.take<T>(count);
    if (d && nout_ == kMaxOut) check(hipErrorInvalidValue);
    else if (d) outs_[nout_++] = Out{p, d};
    return d;
  }
  // an array the call reads AND writes (kh_pack_rows fills some bytes of it): a host array is copied in as well
  template <typename T> T* inout(T* p, uint64_t count, kh_mem where) {
    T* d = out(p, count, where);
    if (d && where == KH_MEM_HOST) copy(d, p, count * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  // the first `count` elements of what out() returned as `d`, back to the host array it stands for (device memory: nothing to do)
  template <typename T> void copy_back(const T* d, uint64_t count) {
    for (int i = 0; i < nout_ && count; ++i)
      if (outs_[i].dev == d) { copy(outs_[i].host, d, count * sizeof(T), hipMemcpyDeviceToHost); return; }
  }
  // device values into host variables of the call
  template <typename T> void read(T* host, const T* dev, uint64_t count = 1) { copy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost); }
  void zero(void* p, size_t bytes) { if (ok()) { err_ = hipMemsetAsync(p, 0, bytes, stream_); busy_ = true; } }
  // waits for everything queued so far (a total the host needs before it goes on)
  bool sync() {
    check(hipStreamSynchronize(stream_));
    busy_ = pending_ = false;
    return ok();
  }
  // the first block leaves the scratch: the caller owns it now and returns it with pool_free
  void* keep() {
    void* p = nblk_ ? blk_[0] : nullptr;
    for (int i = 1; i < nblk_; ++i) blk_[i - 1] = blk_[i];
    if (nblk_) --nblk_;
    return p;
  }
  kh_status finish() {
    if (pending_ || (nblk_ && busy_)) sync();
    for (int i = 0; i < nblk_; ++i) pool_free(device_, blk_[i]);
    nblk_ = 0; nout_ = 0; busy_ = pending_ = false;
    return hip_status(err_);
  }
  // finish() for a call that must not wait for its stream: when only kernels of this call use the blocks (no host copy is pending), a
  // host function queued behind them returns the blocks to the pool; anything else, or a stream that refuses the function, is finish()
  kh_status finish_queued() {
    if (!ok() || pending_ || !nblk_ || !busy_) return finish();
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;      // a captured host node would hand the block back on every replay
    if (hipStreamIsCapturing(stream_, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return finish(); }
    Release* r = new Release;
    r->device = device_; r->n = nblk_;
    for (int i = 0; i < nblk_; ++i) r->blk[i] = blk_[i];
    if (hipLaunchHostFunc(stream_, &Scratch::release, r) != hipSuccess) { (void)hipGetLastError(); delete r; return finish(); }
    nblk_ = 0; nout_ = 0; busy_ = false;
    return KH_OK;
  }

 private:
  struct Release { int device, n; void* blk[4]; };
  // On a runtime thread, in stream order: it must neither call HIP nor wait for anyone who does.  pool_free of a pooled block only
  // takes the pool's mutex, and no holder of that mutex calls HIP (the invariant at pool_trim); every block here came from pool_alloc.
  static void release(void* arg) {
    Release* r = static_cast<Release*>(arg);
    for (int i = 0; i < r->n; ++i) pool_free(r->device, r->blk[i]);
    delete r;
  }
  void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (ok()) { err_ = hipMemcpyAsync(dst, src, bytes, kind, stream_); pending_ = true; }
  }
  static const int kMaxBlocks = 4, kMaxOut = 16;
  struct Out { void* host; const void* dev; };
  int device_; hipStream_t stream_;
  hipError_t err_ = hipSuccess;
  KhCarver car_;
  void* blk_[kMaxBlocks]; int nblk_ = 0;
  Out outs_[kMaxOut]; int nout_ = 0;
  bool busy_ = false;         // work that may use a block has been queued since the last wait
  bool pending_ = false;      // a copy from or to host memory has been queued since the last wait
};

// ---- the shared halves of a count-scan-emit call ------------------------------------------------------
// Such a call writes fixed outputs and the offsets of a CSR, learns the CSR's total with one host wait and, given room, emits the rows.
// empty_rows: the front of a call with nothing to do -- `n_entries` zero offsets, at once in host memory, as one queued memset in device
// memory (the only case that touches the device).
inline kh_status empty_rows(uint64_t* out_offsets, uint64_t n_entries, kh_mem where, int device, hipStream_t stream) {
  if (where == KH_MEM_HOST) { memset(out_offsets, 0, n_entries * sizeof(uint64_t)); return KH_OK; }
  HIPCHK0(hipSetDevice(device));
  HIPCHK0(hipMemsetAsync(out_offsets, 0, n_entries * sizeof(uint64_t), stream));
  return KH_OK;
}
// emit_total: the tail, entered with the read of `total` and the copy-backs of the first pass queued (`total` is the host variable that
// read fills: it holds the count only after the wait, hence the reference).  The one host wait of a device call; *n_total is set before
// anything can be refused; without an output or rows the call is over; a total beyond `cap` is refused with nothing of `out` touched;
// else `out` gets a block of its own where it is host memory, emit(device rows) launches the call's emit kernels, and the rows are
// copied back and the blocks returned in stream order.
template <typename T, typename Emit>
kh_status emit_total(Scratch& s, const unsigned long long& total, T* out, uint64_t cap, uint64_t* n_total, kh_mem where, Emit&& emit) {
  if (!s.sync()) return s.finish();
  *n_total = total;
  if (!out || total == 0) return s.finish();
  if (total > cap) { s.finish(); return KH_ERR_INVALID; }
  T* drows = nullptr;
  if (!s.layout([&](Scratch& c) { drows = c.out(out, total, where); })) return s.finish();
  emit(drows);
  s.launched();
  s.copy_back(drows, total);
  return s.finish_queued();
}
// what kh_chain_edits, kh_chain_cigars and kh_chain_ends ask of k, the anchors and the two texts (a position has 31 bits)
inline bool chain_text_limits_ok(uint32_t k, uint64_t m, uint64_t nq, uint64_t nr, uint32_t ref_base) {
  const uint64_t lim = uint64_t(1) << 31;
  return k >= 1 && k <= 64 && m <= (uint64_t(1) << 24) && nq < lim && nr <= lim && ref_base + nr <= lim;
}
// ... and their texts and anchors as a KedArgs, inside a layout function: the texts are staged only where there are anchors to face
// them; pred and chain are absent (null) for the ends.  n_chains and max_edits are the caller's.
inline void chain_text_args(Scratch& c, KedArgs& P, const void* qtext, uint64_t nq, const void* rtext, uint64_t nr, uint32_t ref_base, const uint32_t* qpos,
                            const uint32_t* rpos, const uint8_t* rev, const int32_t* pred, const int32_t* chain, uint64_t m, uint32_t k, kh_mem where) {
  P.qtext = c.in(static_cast<const uint8_t*>(qtext), m ? nq : 0, where); P.rtext = c.in(static_cast<const uint8_t*>(rtext), m ? nr : 0, where);
  P.qpos = c.in(qpos, m, where); P.rpos = c.in(rpos, m, where); P.rev = c.in(rev, m, where);
  if (pred) { P.pred = c.in(pred, m, where); P.chain = c.in(chain, m, where); }
  P.nq = (uint32_t)nq; P.nr = (uint32_t)nr; P.ref_base = ref_base; P.m = (uint32_t)m; P.k = k;
}

// ---- workspace arena ---------------------------------------------------------------------------
void arena_reset(kh_table* t) { t->blk = 0; t->off = 0; }
kh_status arena_take(kh_table* t, size_t bytes, void** out) {
  bytes = (bytes + 255) & ~size_t(255);
  if (bytes == 0) bytes = 256;
  while (t->blk < t->blocks.size()) {
    Block& b = t->blocks[t->blk];
    if (t->off + bytes <= b.cap) { *out = b.p + t->off; t->off += bytes; return KH_OK; }
    ++t->blk; t->off = 0;
  }
  size_t cap = std::max(bytes, size_t(64) << 20);
  void* vp = nullptr;
  if (getenv("KH_DEBUG_ARENA")) fprintf(stderr, "[kmerhash_amd] arena grows by %.3f GB (block %zu)\n", cap / 1e9, t->blocks.size());
  HIPCHK(pool_alloc(t->device, cap, &vp));
  char* p = static_cast<char*>(vp);
  Block b; b.p = p; b.cap = cap;
  t->blocks.push_back(b);
  t->blk = t->blocks.size() - 1;
  t->off = bytes;
  *out = p;
  return KH_OK;
}
// Before an operation: make the arena ONE block of at least `bytes` (an upper estimate of what the
// operation takes), so that the steady state allocates nothing; arena_take still grows on demand.
kh_status arena_prepare(kh_table* t, size_t bytes) {
  arena_reset(t);
  if (t->blocks.size() == 1 && t->blocks[0].cap >= bytes) return KH_OK;
  size_t total = 0;
  for (auto& b : t->blocks) total += b.cap;
  if (!t->blocks.empty()) {
    hipStreamSynchronize(t->stream);
    for (auto& b : t->blocks) pool_free(t->device, b.p);
    t->blocks.clear();
  }
  void* p = nullptr;
  // (3 % of headroom: a caller's batches differ by a few reads -- without it the NEXT batch, a megabyte larger, frees and allocates the whole
  //  arena again: 0.27 s for 35 GB where hipMalloc is slow)
  const size_t want = std::max(bytes + bytes / 32, total);
  if (getenv("KH_DEBUG_ARENA")) fprintf(stderr, "[kmerhash_amd] arena prepared: %.3f GB (asked %.3f, held %.3f)\n", want / 1e9, bytes / 1e9, total / 1e9);
  HIPCHK(pool_alloc(t->device, want, &p));
  Block b; b.p = static_cast<char*>(p); b.cap = want;
  t->blocks.push_back(b);
  return KH_OK;
}
#define TAKE(ptr, type, count)                                                                  \
  do {                                                                                          \
    void* p__ = nullptr;                                                                        \
    kh_status s__ = arena_take(t, sizeof(type) * size_t(count), &p__);                          \
    if (s__ != KH_OK) return s__;                                                               \
    ptr = static_cast<type*>(p__);                                                              \
  } while (0)

// ---- slots ---------------------------------------------------------------------------------------
// One buffer lifecycle for both key widths: the buffers are held width-erased (SlotBuf) and typed where a kernel takes them.
const KhSlots kNoSlots = KhSlots{nullptr, 0};
inline bool is_wide(const kh_table* t) { return t->slot_bytes == sizeof(KwSlot); }
inline KhSlots narrow(const SlotBuf& b) { return KhSlots{static_cast<KhSlot*>(b.p), b.cap}; }
inline KwSlots wide(const SlotBuf& b) { return KwSlots{static_cast<KwSlot*>(b.p), b.cap}; }
const bool g_poison = getenv("KH_DEBUG_POISON") != nullptr;      // test hook: destination buffers start as garbage
void free_slots(kh_table* t, SlotBuf& s) {
  pool_free(t->device, s.p);
  s = SlotBuf();
}
kh_status alloc_slots(kh_table* t, uint64_t cap, SlotBuf& s) {
  s = SlotBuf();
  hipError_t e = pool_alloc(t->device, std::max<uint64_t>(cap, 16) * t->slot_bytes, &s.p);
  if (e != hipSuccess) { s = SlotBuf(); return fail(t, KH_ERR_NOMEM, std::string("table allocation: ") + hipGetErrorString(e)); }
  s.cap = cap;
  return KH_OK;
}
inline dim3 slots_grid(uint64_t cap) { return dim3((uint32_t)std::min<uint64_t>((cap + 255) / 256, 256 * 16)); }
kh_status fill_empty(kh_table* t, const SlotBuf& s) {
  if (is_wide(t)) hipLaunchKernelGGL(kw_fill_empty, slots_grid(s.cap), dim3(256), 0, t->stream, wide(s));
  else if (t->kind == KHK_RH) hipLaunchKernelGGL((k_fill_empty<KHK_RH>), slots_grid(s.cap), dim3(256), 0, t->stream, narrow(s));
  else hipLaunchKernelGGL((k_fill_empty<KHK_LP>), slots_grid(s.cap), dim3(256), 0, t->stream, narrow(s));
  HIPCHK(hipGetLastError());
  return KH_OK;
}
// a destination buffer of capacity `cap`, as the typed view the caller launches with.  It is NOT cleared: a re-layout writes
// every slot of its destination, occupied or empty, exactly once (the slices of the chunk workgroups tile the circular table),
// so clearing 16 B x capacity first would only add a 2 GB memset per build of a 2^27-bucket table
template <typename Slots>
kh_status fresh_slots(kh_table* t, uint64_t cap, Slots& s) {
  SlotBuf b;
  if (t->spare.cap == cap && t->spare.p) { b = t->spare; t->spare = SlotBuf(); }
  else {
    kh_status st = alloc_slots(t, cap, b);
    if (st != KH_OK) return st;
  }
  s = Slots{static_cast<decltype(s.s)>(b.p), cap};
  if (g_poison) {
    if (is_wide(t)) hipLaunchKernelGGL(kw_poison, slots_grid(cap), dim3(256), 0, t->stream, wide(b));
    else hipLaunchKernelGGL(k_poison, slots_grid(cap), dim3(256), 0, t->stream, narrow(b));
    HIPCHK(hipGetLastError());
  }
  return KH_OK;
}
void retire_slots(kh_table* t, SlotBuf s) {   // keep one spare buffer for ping-pong rebuilds
  if (!s.p) return;
  if (t->spare.p) { hipStreamSynchronize(t->stream); free_slots(t, t->spare); }
  t->spare = s;
}
// a completed re-layout becomes the table; the buffer it replaces becomes the spare
void adopt_slots(kh_table* t, SlotBuf nw) {
  const SlotBuf old = t->cur;
  t->cur = nw;
  retire_slots(t, old);
  t->min_load = threshold(nw.cap, t->min_lf);
  t->max_load = threshold(nw.cap, t->max_lf);
}

// ---- profiling -----------------------------------------------------------------------------------
struct Launch {
  kh_table* t; const char* name; hipEvent_t a, b; bool on;
  Launch(kh_table* t_, const char* n) : t(t_), name(n), a(nullptr), b(nullptr), on(t_ && t_->prof) {
    if (on) { a = event_get(t->device); b = event_get(t->device); hipEventRecord(a, t->stream); }
  }
  ~Launch() {
    if (on) { hipEventRecord(b, t->stream); ProfRec r; r.name = name; r.a = a; r.b = b; t->recs.push_back(r); }
  }
};
void prof_collect(kh_table* t) {
  if (t->recs.empty()) return;
  hipStreamSynchronize(t->stream);
  for (auto& r : t->recs) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, r.a, r.b);
    event_put(t->device, r.a); event_put(t->device, r.b);
    bool found = false;
    for (auto& a : t->prof_acc) if (a.first == r.name) { a.second.first += ms; a.second.second += 1; found = true; break; }
    if (!found) t->prof_acc.push_back(std::make_pair(std::string(r.name), std::make_pair(double(ms), uint64_t(1))));
  }
  t->recs.clear();
}

#define KH_SWITCH_HASH(h, ...)                                                        \
  switch (h) {                                                                        \
    case KHH_IDENTITY: { constexpr int HASH = KHH_IDENTITY; __VA_ARGS__; } break;     \
    case KHH_MURMUR3_X86: { constexpr int HASH = KHH_MURMUR3_X86; __VA_ARGS__; } break; \
    case KHH_MURMUR3_X64: { constexpr int HASH = KHH_MURMUR3_X64; __VA_ARGS__; } break; \
    default: { constexpr int HASH = KHH_FARM; __VA_ARGS__; } break;                   \
  }
#define KH_SWITCH_KIND_HASH(k, h, ...)                                                \
  if ((k) == KHK_RH) { constexpr int KIND = KHK_RH; KH_SWITCH_HASH(h, __VA_ARGS__) }  \
  else { constexpr int KIND = KHK_LP; KH_SWITCH_HASH(h, __VA_ARGS__) }

inline uint32_t grid_for(uint64_t n, uint32_t block, uint32_t maxblocks = 256 * 16) {
  uint64_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > maxblocks) g = maxblocks;
  return (uint32_t)g;
}

// stage a host array on the device (workspace) or pass a device pointer through
template <typename T>
kh_status stage_in(kh_table* t, const void* p, uint64_t n, kh_mem where, const T** out) {
  if (where == KH_MEM_DEVICE || p == nullptr) { *out = static_cast<const T*>(p); return KH_OK; }
  T* d = nullptr;
  TAKE(d, T, n);
  HIPCHK(hipMemcpyAsync(d, p, sizeof(T) * n, hipMemcpyHostToDevice, t->stream));
  *out = d;
  return KH_OK;
}

// workspace a rebuild at capacity `cap` takes (home counts + per-chunk scan arrays)
inline size_t ws_rebuild(uint64_t cap) { return size_t(cap) * 2 + (cap > KH_L ? (cap >> KH_LB) : 1) * 48 + (size_t(1) << 16); }

// ---- chunk rebuild ---------------------------------------------------------------------------------
// Lays out (live elements of t->cur, minus `erased`) U (new distinct elements) at capacity new_cap in
// a fresh buffer and makes it current.  On KH_ERR_* the current table is unchanged.
struct PreCount { uint16_t* homecnt; long long* sumA; long long* sumN; };   // chunk counts already produced by k_dedup

const bool g_disable_fused_rebuild = getenv("KH_DISABLE_FUSED_BUILD") != nullptr || getenv("KH_DISABLE_FUSED_REBUILD") != nullptr;   // test hooks

// The three speculative one-launch forms share their launch sequence: k_build_fused<KIND, HASH, SRC> over all chunks, the
// reduction of the per-chunk totals, and the tail launch that places chunk 0 once the last chunk's run-over is known.
// SRC 0: bulk build into an empty table from partition records; 1: re-layout of the current table (+ new distinct lists);
// 2: current table + partition records folded together.  Returns with the stream synchronised and, in t->hpin,
// [0] elements placed, [1] max(first-occurrence position + 1), bytes 32..: the vote words, bytes 64..: the flags.
const long long g_poll_limit = getenv("KH_DEBUG_POLL_LIMIT") ? atoll(getenv("KH_DEBUG_POLL_LIMIT")) : (1ll << 23);     // test hook: look-back time-out
struct FusedRun { unsigned long long* totals; uint32_t* flags; };
const bool g_disable_lean = getenv("KH_DISABLE_LEAN_BUILD") != nullptr;      // test hook / A-B: the general one-launch build for 12-byte records too
// granules, control words (256 bytes), maxidx, the lean build's count words: zeroed by ONE fill
inline size_t fused_blk_bytes(uint32_t nch) { return (size_t)nch * 12 + 256 + (size_t)KH_FUSED_NCNT * KH_FUSED_CNT_STRIDE * 8; }
kh_status launch_fused(kh_table* t, int src, KhFusedParams& F, const KhSlots& nw, uint32_t PB_tail, const char* name, FusedRun* out) {
  const uint32_t nch = (uint32_t)(nw.cap >> KH_LB);
  char* blk; uint32_t* maxidx; uint64_t* ck0; uint32_t* cv0; uint16_t* hc0;
  const size_t sz_pub = (size_t)nch * 8, sz_ctl = sz_pub + 256, sz_all = fused_blk_bytes(nch);
  // (an optimistic bulk insert has zeroed the block with its sample set, before the partition: no fill between the second pass and the build)
  if (t->fused_blk && t->fused_blk_bytes == sz_all) blk = t->fused_blk;
  else { TAKE(blk, char, sz_all); HIPCHK(hipMemsetAsync(blk, 0, sz_all, t->stream)); }
  t->fused_blk = nullptr;
  maxidx = reinterpret_cast<uint32_t*>(blk + sz_ctl);
  TAKE(ck0, uint64_t, KH_DD_M); TAKE(cv0, uint32_t, KH_DD_M); TAKE(hc0, uint16_t, KH_L);
  F.New = nw; F.seed = t->seed;
  F.pub = reinterpret_cast<unsigned long long*>(blk);
  unsigned long long* totals = reinterpret_cast<unsigned long long*>(blk + sz_pub);   // 2 x u64 (k_fused_totals / k_fused_tail)
  F.maxidx = maxidx; F.ck0 = ck0; F.cv0 = cv0; F.homecnt0 = hc0;
  F.cnt = reinterpret_cast<unsigned long long*>(blk + sz_ctl + (size_t)nch * 4);
  F.skip = src == 0 ? t->sample_dups : nullptr;
  F.est = reinterpret_cast<unsigned long long*>(blk + sz_pub + 32);          // 2 x u64
  F.flags = reinterpret_cast<uint32_t*>(blk + sz_pub + 64);                  // KH_NFLAGS x u32
  F.poll_limit = g_poll_limit;
  F.R.New = nw; F.R.seed = t->seed; F.R.flags = F.flags;
  bool lean = false;
  { Launch L(t, name);
    // (the benchmark case -- a duplicate-free sample, one source of 12-byte records -- has its own kernel with 17 KB less LDS: 4 workgroups per CU)
    // (... as long as a chunk of mean + 5 sigma records fits its smaller staging arrays: a table filled to 0.9 would fail it in a chunk or two
    //  of 65536 and pay for the discarded launch)
    const double mean_c = (double)F.n_total / (double)nch;
    const bool lean_fits = mean_c + 5.0 * std::sqrt(mean_c) < (double)KH_LEAN_M;
    lean = src == 0 && F.nodup && F.src.rec12 == 1 && F.src.n == 1 && lean_fits && !g_disable_lean;
    if (lean) { KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_build_lean<KIND, HASH>), dim3(nch), dim3(KH_CHUNK_THREADS), 0, t->stream, F)); }
    else if (src == 0) { KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_build_fused<KIND, HASH, 0>), dim3(nch), dim3(KH_CHUNK_THREADS), 0, t->stream, F)); }
    else if (src == 1) { KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_build_fused<KIND, HASH, 1>), dim3(nch), dim3(KH_CHUNK_THREADS), 0, t->stream, F)); }
    else if (src == 3) { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_build_fused<KHK_RH, HASH, 3>), dim3(nch), dim3(KH_CHUNK_THREADS), 0, t->stream, F)); }      // (batch erase: Robin Hood only)
    else if (src == 4) { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_erase_stream<HASH>), dim3(nch), dim3(KH_CHUNK_THREADS), 0, t->stream, F)); }              // (batch erase as an ordered stream)
    else if (src == 5) { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_insert_stream<HASH>), dim3(nch), dim3(KH_CHUNK_THREADS), 0, t->stream, F)); }             // (insert into a loaded table as an ordered stream)
    else { KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_build_fused<KIND, HASH, 2>), dim3(nch), dim3(KH_CHUNK_THREADS), 0, t->stream, F)); } }
  // (the lean build has added its chunks' counts to F.cnt and carries no stream positions: the tail launch sums the count words itself)
  if (!lean) { Launch L(t, "k_fused_totals");
    hipLaunchKernelGGL(k_fused_totals, dim3(std::max<uint32_t>(1u, std::min<uint32_t>(64u, nch / 1024u))), dim3(1024), 0, t->stream, F.pub, maxidx, nch, totals); }
  { // chunk 0: placed now that the last chunk's run-over is known (one workgroup, the placement of the general path); the same launch
    // gathers what the host reads: the totals of the lean build, the sample's and the partition's words next to the control words
    Launch L(t, "k_fused_tail");
    KhRebuildParams T0;
    memset(&T0, 0, sizeof(T0));
    T0.Old = kNoSlots; T0.New = nw; T0.ck = ck0; T0.cv = cv0; T0.PB = PB_tail;
    T0.seed = t->seed; T0.homecnt = hc0; T0.flags = F.flags;
    KhTailParams E;
    E.pub = F.pub; E.nch = nch; E.cnt = lean ? F.cnt : nullptr; E.totals = totals;
    E.skip = F.skip; E.ovf = t->part_overflow; E.status = reinterpret_cast<uint32_t*>(blk + sz_pub + 16);
    KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_fused_tail<KIND, HASH>), dim3(1), dim3(KH_CHUNK_THREADS), 0, t->stream, T0, E));
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t->hpin, blk + sz_pub, 128, hipMemcpyDeviceToHost, t->stream));      // the one copy: totals, status words, vote, flags
  HIPCHK(hipStreamSynchronize(t->stream));
  { const uint32_t* status = reinterpret_cast<const uint32_t*>(t->hpin + 2);
    t->hpin[31] = status[0];      // duplicates the sample found (optimistic attempt; non-zero: every kernel of the attempt returned at once)
    t->hpin[30] = status[1]; }    // a partition outgrew its slot
  out->totals = totals; out->flags = F.flags;
  return KH_OK;
}

// what the flags of a re-layout or a de-duplication mean to the caller (KH_OK: none is raised)
const char* const kProbeOverflowText = "Robin Hood probe distance would exceed 127 (7-bit info field, hashmap_robinhood.hpp:142-144,556)";
const char* const kDedupOverflowText = "internal: de-duplication set overflow";
kh_status flags_status(kh_table* t, const uint32_t* f) {
  if (f[KH_FLAG_PROBE_OVERFLOW]) return fail(t, KH_ERR_PROBE_OVERFLOW, kProbeOverflowText);
  if (f[KH_FLAG_REGION_OVERFLOW]) return fail(t, KH_ERR_PROBE_OVERFLOW, "cluster longer than one chunk (2048 slots) without an empty slot");
  if (f[KH_FLAG_COUNT_OVERFLOW]) return fail(t, KH_ERR_PROBE_OVERFLOW, "more than 65535 keys share one home bucket");
  if (f[KH_FLAG_INTERNAL]) return fail(t, KH_ERR_HIP, kDedupOverflowText);
  return KH_OK;
}

// what the general re-layout driver needs to know of a key width: the kernels' argument struct and the two chunk launches
struct Narrow {
  typedef KhSlots Slots; typedef KhRebuildParams Params;
  static Slots view(const SlotBuf& b) { return narrow(b); }
  static void set_seed(Params& P, const kh_table* t) { P.seed = t->seed; }
  static void count(kh_table* t, uint32_t nch, const Params& P) {
    Launch L(t, "k_chunk_count");
    KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_chunk_count<KIND, HASH>), dim3(nch), dim3(KH_CHUNK_THREADS), 0, t->stream, P));
  }
  static void place(kh_table* t, uint32_t nch, const Params& P) {
    Launch L(t, "k_chunk_place");
    KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_chunk_place<KIND, HASH>), dim3(nch), dim3(KH_CHUNK_THREADS), 0, t->stream, P));
  }
};
struct Wide {
  typedef KwSlots Slots; typedef KwRebuildParams Params;
  static Slots view(const SlotBuf& b) { return wide(b); }
  static void set_seed(Params& P, const kh_table* t) { P.seed = t->seed.s; }
  static void count(kh_table* t, uint32_t nch, const Params& P) {
    Launch L(t, "kw_chunk_count");
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((kw_chunk_count<HASH>), dim3(nch), dim3(KW_DD_THREADS), 0, t->stream, P));
  }
  static void place(kh_table* t, uint32_t nch, const Params& P) {
    Launch L(t, "kw_chunk_place");
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((kw_chunk_place<HASH>), dim3(nch), dim3(KW_DD_THREADS), 0, t->stream, P));
  }
};
// The general re-layout into the fresh buffer nw: chunk count (unless `pre` has the counts) -> k_chunk_carry -> chunk place, then
// nw becomes the table.  A raised flag leaves the table as it was and makes nw the spare.
template <typename W>
kh_status relayout(kh_table* t, typename W::Slots nw, const uint64_t* ck, const uint32_t* cv, const uint64_t* noff, const uint32_t* ncnt,
                   uint32_t PB, bool drop_marked, const PreCount* pre) {
  const uint32_t nch = nw.cap > KH_L ? (uint32_t)(nw.cap >> KH_LB) : 1u;
  uint16_t* homecnt; long long *sumA, *sumN, *xcarry; KhMP* ptmp; uint32_t* flags;
  if (pre) { homecnt = pre->homecnt; sumA = pre->sumA; sumN = pre->sumN; }
  else { TAKE(homecnt, uint16_t, nw.cap); TAKE(sumA, long long, nch); TAKE(sumN, long long, nch); }
  TAKE(xcarry, long long, nch);
  TAKE(ptmp, KhMP, nch);
  TAKE(flags, uint32_t, KH_NFLAGS);
  HIPCHK(hipMemsetAsync(flags, 0, sizeof(uint32_t) * KH_NFLAGS, t->stream));
  typename W::Params P;
  memset(&P, 0, sizeof(P));
  P.Old = W::view(t->cur); P.drop_marked = drop_marked ? 1 : 0; P.New = nw; P.ck = ck; P.cv = cv; P.noff = noff; P.ncnt = ncnt; P.PB = PB;
  if (t->lsize == 0) P.Old.cap = 0;   // nothing to carry over: the chunk kernels skip the source scan
  W::set_seed(P, t); P.homecnt = homecnt; P.sumA = sumA; P.sumN = sumN; P.xcarry = xcarry; P.flags = flags;
  if (!pre) W::count(t, nch, P);
  { Launch L(t, "k_chunk_carry");
    hipLaunchKernelGGL(k_chunk_carry, dim3(1), dim3(1024), 0, t->stream, sumA, sumN, nch, (long long)nw.cap, xcarry, ptmp); }
  W::place(t, nch, P);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t->hpin, flags, sizeof(uint32_t) * KH_NFLAGS, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  const kh_status st = flags_status(t, reinterpret_cast<const uint32_t*>(t->hpin));
  if (st != KH_OK) { retire_slots(t, nw); return st; }
  adopt_slots(t, nw);
  return KH_OK;
}

kh_status rebuild(kh_table* t, uint64_t new_cap, const uint64_t* ck, const uint32_t* cv, const uint64_t* noff,
                  const uint32_t* ncnt, uint32_t PB, bool drop_marked, uint64_t total_after, const PreCount* pre = nullptr) {
  if (total_after > new_cap)
    return fail(t, KH_ERR_FULL, "table would hold more elements than buckets (no slot to insert into)");
  if (is_wide(t)) {      // the general driver is all a wide table has
    KwSlots nw;
    kh_status st = fresh_slots(t, new_cap, nw);
    return st != KH_OK ? st : relayout<Wide>(t, nw, ck, cv, noff, ncnt, PB, drop_marked, nullptr);
  }
  KhSlots nw;
  kh_status st = fresh_slots(t, new_cap, nw);
  if (st != KH_OK) return st;
  // ---- one-launch rebuild (k_build_fused with the current table as its source): Robin Hood, same or doubled capacity.
  // Speculative like the bulk build: a chunk denser than the staging area, a carry chain or a poll time-out raise a flag,
  // and the three-kernel path below redoes the work into the same buffer.
  // Also taken with an EMPTY source table (either kind): the batch was de-duplicated on the general path and only its
  // distinct keys (ck/cv lists) have to be laid out.
  const bool from_empty = t->lsize == 0;
  if (!pre && !g_disable_fused_rebuild && new_cap >= 2 * (uint64_t)KH_L && total_after <= threshold(new_cap, 0.9f) &&
      (!noff || PB >= log2u(new_cap >> KH_LB)) &&
      (from_empty ? noff != nullptr
                  : (t->cur.cap >= 2 * (uint64_t)KH_L && (new_cap == t->cur.cap || new_cap == 2 * t->cur.cap)))) {
    const size_t keep_blk = t->blk, keep_off = t->off;
    KhFusedParams F;
    memset(&F, 0, sizeof(F));
    F.PB = PB; F.mode = KH_DEDUP_FIRST;
    F.R.Old = narrow(t->cur); F.R.drop_marked = drop_marked ? 1 : 0; F.R.ck = ck; F.R.cv = cv; F.R.noff = noff; F.R.ncnt = ncnt; F.R.PB = PB;
    if (from_empty) F.R.Old.cap = 0;     // nothing to carry over: the source scan is skipped
    FusedRun run;
    // (the parked list of chunk 0 is its own: one partition per chunk)
    { kh_status fs = launch_fused(t, 1, F, nw, log2u(new_cap >> KH_LB), "k_rebuild_fused", &run); if (fs != KH_OK) return fs; }
    const uint32_t* ff = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(t->hpin) + 64);
    bool bad = false;
    for (int i = 0; i < KH_NFLAGS; ++i) bad = bad || ff[i] != 0;
    if (!bad && t->hpin[0] == total_after) {
      adopt_slots(t, nw);
      return KH_OK;
    }
    if (getenv("KH_DEBUG_FUSED"))
      fprintf(stderr, "[kmerhash_amd] fused rebuild rejected: placed %llu expected %llu flags=%u %u %u %u %u\n", (unsigned long long)t->hpin[0],
              (unsigned long long)total_after, ff[0], ff[1], ff[2], ff[3], ff[4]);
    if (ff[KH_FLAG_PROBE_OVERFLOW] && !ff[KH_FLAG_FUSE_INVALID]) {   // a genuine 7-bit overflow: the general path would find the same
      retire_slots(t, nw);
      return fail(t, KH_ERR_PROBE_OVERFLOW, kProbeOverflowText);
    }
    t->blk = keep_blk; t->off = keep_off;      // scratch of the failed attempt is reused by the general path
  }
  return relayout<Narrow>(t, nw, ck, cv, noff, ncnt, PB, drop_marked, pre);
}

// rehash(b): hashmap_robinhood.hpp:432-464 / hashmap_linearprobe.hpp:324-349
// Robin Hood rehash to c buckets (a power of two): copy() re-inserts through insert(), which doubles whenever size >= max_load (:530);
// the capacity that results is the doubling rule applied to `size` distinct inserts from c.
inline uint64_t rh_rehash_capacity(uint64_t c, uint64_t size, float max_lf) {
  if (size > 0) {
    if (0 >= threshold(c, max_lf)) c <<= 1;
    while (size > threshold(c, max_lf)) c <<= 1;
  }
  return c;
}
kh_status refuse_streaming(kh_table* t) { return fail(t, KH_ERR_INVALID, "a streamed insert is in progress (kh_insert_end first)"); }
kh_status do_rehash(kh_table* t, uint64_t b) {
  if (t->ins.active) return refuse_streaming(t);
  uint64_t n = next_pow2(b);
  if (n == t->cur.cap) return KH_OK;
  if (t->kind == KHK_RH) {
    n = rh_rehash_capacity(n, t->lsize, t->max_lf);
    if (n == t->cur.cap) return KH_OK;
  } else if (t->lsize > n) {
    return fail(t, KH_ERR_FULL, "ERROR: did not find any place to insert.  should not have happend (hashmap_linearprobe.hpp:408)");
  }
  { kh_status ps = arena_prepare(t, ws_rebuild(n)); if (ps != KH_OK) return ps; }
  return rebuild(t, n, nullptr, nullptr, nullptr, nullptr, 0, false, t->lsize);
}
kh_status do_reserve(kh_table* t, uint64_t n) {   // :421-426 / :313-318
  if (n > t->max_load) return do_rehash(t, static_cast<uint64_t>(static_cast<float>(n) / t->max_lf));
  return KH_OK;
}

// ---- radix partition of a batch by bit-reversed chunk id ------------------------------------------
struct Partitioned {
  ulonglong2* rec;                              // records grouped by partition: (key, idx<<32|val)
  uint64_t* part_off;                           // [nparts+1]
  uint32_t PB, nparts;
  ulonglong2* spare;                            // the other record buffer (free for outputs)
  uint64_t slot;                                // != 0: histogram-free layout: partition q = rec[q * slot, cursor[q])
  const unsigned long long* cursor;
  uint32_t* overflow;                           // device flag: a partition outgrew its slot (the batch must be redone with exact offsets)
  int rec12;                                    // 0: 16-byte records; 1: 12-byte (key, value) (histogram-free layout only); 2: 8-byte keys (counting insert)
};
// (slack_slot: the slot of a histogram-free partition, mean + 7 sigma -- kh_part_sizing.h)
const bool g_disable_slack = getenv("KH_DISABLE_SLACK_PARTITION") != nullptr;      // test hook: exact offsets always
// eight consecutive partition tiles per XCD (blocks b, b + 8, ... share one): the adjacent output runs of consecutive tiles meet in
// one L2 (-3 % scatter time, measured A/B); KH_DISABLE_XCD_SWIZZLE=1 turns it off
const int g_xcd_swizzle = getenv("KH_DISABLE_XCD_SWIZZLE") ? 0 : 1;
// XCD-private write fronts of the histogram-free partition (KhPartParams::sub_slot): KH_DISABLE_XCD_FRONTS=1 restores one cursor per
// level-1 bucket and the tile order of the second pass
const int g_xcd_fronts = getenv("KH_DISABLE_XCD_FRONTS") ? 0 : 1;
// (sizing: xcd_sub_slot in kh_part_sizing.h.  KH_XCD_FRONTS_MIN_TILES: the least mean fill of a sub-slot, in tiles, for which the sub-slots are used --
//  default 4; the benchmark shape has 6.4, a batch of 6e6 records into 2^12 partitions 1.4.  Read at every call: the tests reach the sub-slots at small shapes with it)
inline uint32_t xcd_fronts_min_tiles() { const char* e = getenv("KH_XCD_FRONTS_MIN_TILES"); return e ? (uint32_t)std::max(0, atoi(e)) : 4u; }
// records the two buffers of partition_batch must hold
inline uint64_t part_buffer_records(uint64_t n, uint32_t PB, bool allow_slack, double vf = 1.0) {
  if (!allow_slack || g_disable_slack || PB <= 11 || n < (uint64_t(256) << PB)) return n;
  return (slack_slot((double)n / (double)(uint64_t(1) << PB), vf) << PB) + KH_PART_TILE;        // slots + the dump area of the scatter
}

// the duplicate sample of an optimistic bulk insert (insert_core): taken by the launch that initialises the partition's cursors, and both
// passes return at once if it finds a duplicate (KhPartParams::skip).  set / dups: zeroed by the caller
struct SampleRun { unsigned long long* set; uint32_t* dups; };
// Partitions n input pairs into `fin` (n records); `tmp` (n records) is scratch for the first of two passes.  idx_base =
// stream position of the first pair (pairs fed before it in a streamed insert).  Asynchronous on the table's stream.
kh_status partition_batch(kh_table* t, const char* kbase, uint32_t kstride, const char* vbase, uint32_t vstride,
                          uint32_t vconst, uint64_t n, uint64_t idx_base, uint32_t PB, ulonglong2* tmp, ulonglong2* fin, Partitioned& out,
                          bool allow_slack = false, int rec12 = 0, const SlackShared* shared = nullptr, bool force_slack = false, double vf = 1.0,
                          const SampleRun* sample = nullptr) {
  const uint32_t nparts = 1u << PB;
  out.slot = 0; out.cursor = nullptr; out.overflow = nullptr; out.rec12 = 0;
  // (force_slack: the caller has sized tmp / fin for the fixed slots itself -- (slack_slot(n / 2^PB) << PB) + KH_PART_TILE records each --
  //  whatever n is: the erase keys of a batch erase, where the histogram sweep would cost more than the partition)
  if (shared || force_slack || part_buffer_records(n, PB, allow_slack, vf) != n) {
    // ---- histogram-free two-pass partition: hashed keys fill the 2^PB partitions evenly, so every partition
    // gets a fixed slot of mean + 7 sigma records and the passes reserve space with their cursors alone: no histogram sweep
    // over the keys (0.33 ms per 1e8), no offset scan.  Level-1 buckets are the unions of their partitions' slots.
    const uint32_t B1 = (PB + 1) / 2, B2 = PB - B1, nb1 = 1u << B1, nb2 = 1u << B2;
    // (a piece of a streamed insert: its level-1 buckets are sized for the piece, the final slots -- shared -- for the whole batch)
    const uint64_t slot = shared ? shared->slot : slack_slot((double)n / (double)nparts, vf);
    const uint64_t slot1 = shared ? slack_slot((double)n / (double)nb1) : slot * nb2;
    // (XCD-private fronts: eight sub-slots per level-1 bucket, see xcd_sub_slot; a streamed piece keeps one cursor per bucket)
    uint32_t tps_sub = 0;
    const uint64_t sub_slot = (g_xcd_fronts && !shared) ? xcd_sub_slot(n, nb1, nb2, slot1, vf, KH_PART_TILE, xcd_fronts_min_tiles(), &tps_sub) : 0;
    unsigned long long *cur1, *cur2; uint64_t* starts; uint32_t* ovf;
    TAKE(cur1, unsigned long long, sub_slot ? (size_t)nb1 * 8 : nb1);
    if (shared) { cur2 = shared->cur2; starts = shared->starts; ovf = shared->ovf; }
    else { TAKE(cur2, unsigned long long, nparts); TAKE(starts, uint64_t, (size_t)nparts + 1); TAKE(ovf, uint32_t, 1); }
    // the second pass cuts every level-1 slot into tiles by arithmetic (no tile list, see KhPartParams::slot_in) -- up to mean + 9 sigma of a
    // level-1 bucket's fill, which is well inside the slot (the union of its partitions' slots: 256 x 7 sigma of THEIR fill); a bucket
    // that holds more raises the overflow flag like a slot that runs over
    const double mean1 = (double)n / (double)nb1;
    const uint64_t fill_cap = std::min<uint64_t>(slot1, (uint64_t)(mean1 + 9.0 * std::sqrt(mean1 * vf) + 16.0));
    const uint32_t tps = sub_slot ? tps_sub : (uint32_t)((fill_cap + KH_PART_TILE - 1) / KH_PART_TILE);
    const uint32_t max_tiles = (sub_slot ? nb1 * 8u : nb1) * tps;
    if (shared) hipLaunchKernelGGL(k_init_cursors, dim3((nb1 + 255) / 256), dim3(256), 0, t->stream, cur1, (uint64_t*)nullptr, (uint64_t)nb1, slot1);
    else {
      KhCursorInit I;
      I.cur1 = cur1; I.n1 = nb1; I.slot1 = slot1; I.sub1 = sub_slot ? 8u : 1u; I.cur2 = cur2; I.starts = starts; I.n2 = nparts; I.slot2 = slot; I.ovf = ovf;
      if (sample) { Launch L(t, "k_sample_dups");
        hipLaunchKernelGGL(k_sample_dups, dim3(KH_SAMPLE_N / 256), dim3(256), 0, t->stream, kbase, kstride, n, sample->set, sample->dups, I); }
      else hipLaunchKernelGGL(k_init_cursors2, dim3((nparts + 256) / 256), dim3(256), 0, t->stream, I);
    }
    KhPartParams P;
    memset(&P, 0, sizeof(P));
    P.skip = sample ? sample->dups : nullptr;
    P.idx_base = idx_base;
    P.xcd_swizzle = g_xcd_swizzle;
    P.kbase = kbase; P.kstride = kstride; P.vbase = vbase; P.vstride = vstride; P.vconst = vconst; P.n = n;
    P.ntiles = (uint32_t)((n + KH_PART_TILE - 1) / KH_PART_TILE);
    P.seed = t->seed; P.PB = PB; P.shift = B2; P.nb = nb1; P.cursor = cur1; P.orec = tmp; P.slot = slot1; P.overflow = ovf; P.dump = slot1 * nb1;
    P.sub_slot = sub_slot;
    { Launch L(t, "k_part_scatter");
      if (rec12 == 1) { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_scatter<HASH, 1>), dim3(P.ntiles), dim3(KH_PART_THREADS), ((nb1 + 1u) & ~1u) * 8 + nb1 * 8, t->stream, P)); }
      else if (rec12 == 2) { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_scatter<HASH, 2>), dim3(P.ntiles), dim3(KH_PART_THREADS), ((nb1 + 1u) & ~1u) * 8 + nb1 * 8, t->stream, P)); }
      else { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_scatter<HASH, 0>), dim3(P.ntiles), dim3(KH_PART_THREADS), ((nb1 + 1u) & ~1u) * 8 + nb1 * 8, t->stream, P)); } }
    KhPartParams Q = P;
    Q.kbase = nullptr; Q.kstride = 0; Q.vbase = nullptr; Q.vstride = 0; Q.rec_in = tmp;
    Q.tiles = nullptr; Q.ntiles_dev = nullptr; Q.ntiles = max_tiles; Q.slot_in = sub_slot ? sub_slot : slot1; Q.cur_in = cur1; Q.tps = tps;
    Q.sub_slot = 0; Q.seg_shift = sub_slot ? 3u : 0u; Q.xcd_buckets = sub_slot ? 1 : 0;
    Q.shift = 0; Q.nb = nb2; Q.cursor = cur2; Q.orec = fin; Q.slot = slot; Q.dump = slot * nparts;
    { Launch L(t, "k_part_scatter");
      if (rec12 == 1) { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_scatter<HASH, 1>), dim3(max_tiles), dim3(KH_PART_THREADS), ((nb2 + 1u) & ~1u) * 8 + nb2 * 8, t->stream, Q)); }
      else if (rec12 == 2) { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_scatter<HASH, 2>), dim3(max_tiles), dim3(KH_PART_THREADS), ((nb2 + 1u) & ~1u) * 8 + nb2 * 8, t->stream, Q)); }
      else { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_scatter<HASH, 0>), dim3(max_tiles), dim3(KH_PART_THREADS), ((nb2 + 1u) & ~1u) * 8 + nb2 * 8, t->stream, Q)); } }
    HIPCHK(hipGetLastError());
    out.rec = fin; out.part_off = starts; out.PB = PB; out.nparts = nparts; out.spare = tmp;
    out.slot = slot; out.cursor = cur2; out.overflow = ovf; out.rec12 = rec12;
    return KH_OK;
  }
  if (rec12 == 1) return fail(t, KH_ERR_HIP, "internal: record kind not available with exact offsets");
  ulonglong2* ar = nullptr; ulonglong2* br = fin;
  const uint32_t B1 = PB <= 11 ? PB : (PB + 1) / 2, B2 = PB - B1;
  const uint32_t nb1 = 1u << B1, nb2 = 1u << B2;
  ar = B2 ? tmp : fin;                          // a single pass writes the final buffer directly
  uint32_t* counts1; uint64_t* off1; unsigned long long* cur1;
  TAKE(counts1, uint32_t, nb1); TAKE(off1, uint64_t, nb1 + 1); TAKE(cur1, unsigned long long, nb1);
  KhPartParams P;
  memset(&P, 0, sizeof(P));
  P.idx_base = idx_base;
  P.xcd_swizzle = g_xcd_swizzle;
  P.kbase = kbase; P.kstride = kstride; P.vbase = vbase; P.vstride = vstride; P.vconst = vconst; P.rec_in = nullptr; P.n = n;
  P.tiles = nullptr; P.ntiles_dev = nullptr; P.ntiles = (uint32_t)((n + KH_PART_TILE - 1) / KH_PART_TILE);
  P.seed = t->seed; P.PB = PB; P.shift = B2; P.nb = nb1; P.counts = counts1; P.cursor = cur1;
  P.orec = ar;
  KhTile* tiles = nullptr; uint32_t* ntiles_dev = nullptr; uint32_t* counts2 = nullptr; uint64_t* off2 = nullptr; unsigned long long* cur2 = nullptr;
  const uint32_t max_tiles = (uint32_t)(n / KH_PART_TILE) + nb1 + 1;
  if (B2 > 0) {
    TAKE(tiles, KhTile, max_tiles); TAKE(ntiles_dev, uint32_t, 1);
    TAKE(counts2, uint32_t, nparts); TAKE(off2, uint64_t, nparts + 1); TAKE(cur2, unsigned long long, nparts);
    HIPCHK(hipMemsetAsync(counts2, 0, sizeof(uint32_t) * nparts, t->stream));
  }
  const bool full_hist = B2 > 0 && PB <= 18;     // 2^16 16-bit bins = 128 KB of LDS per sweep; up to four sweeps (slices of the id space)
  if (full_hist) {
    // one sweep over the keys gives the histogram of the full partition id; both levels' offsets follow from one scan
    const int ncu = cu_count(t);
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ncu, (n + 4095) / 4096));
    const uint32_t slice_bits = PB > 16 ? PB - 16 : 0;
    { Launch L(t, "k_part_hist");
      const size_t smem = (size_t)((nparts >> slice_bits) / 2) * 4;
      KH_SWITCH_HASH(t->hash,
                     if (smem > 65536) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_part_hist_full<HASH>),
                                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
                     for (uint32_t sl = 0; sl < (1u << slice_bits); ++sl)
                       hipLaunchKernelGGL((k_part_hist_full<HASH>), dim3(grid), dim3(KH_FULLHIST_THREADS), smem, t->stream,
                                          kbase, kstride, n, t->seed, PB, sl, slice_bits, counts2)); }
    { Launch L(t, "k_scan");
      hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, t->stream, counts2, (uint64_t)nparts, off2); }
    hipLaunchKernelGGL(k_seg_offsets, dim3((nb1 + 256) / 256), dim3(256), 0, t->stream, off2, nb1, nb2, off1, cur1);
  } else {
    HIPCHK(hipMemsetAsync(counts1, 0, sizeof(uint32_t) * nb1, t->stream));
    const uint32_t hist_grid = std::min<uint32_t>(P.ntiles, 1024);
    { Launch L(t, "k_part_hist");
      KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_hist<HASH>), dim3(hist_grid), dim3(KH_PART_THREADS), nb1 * 4, t->stream, P)); }
    { Launch L(t, "k_scan");
      hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, t->stream, counts1, (uint64_t)nb1, off1); }
    HIPCHK(hipMemcpyAsync(cur1, off1, sizeof(uint64_t) * nb1, hipMemcpyDeviceToDevice, t->stream));
  }
  { Launch L(t, "k_part_scatter");
    if (rec12 == 2) { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_scatter<HASH, 2>), dim3(P.ntiles), dim3(KH_PART_THREADS), ((nb1 + 1u) & ~1u) * 8 + nb1 * 8, t->stream, P)); }
    else { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_scatter<HASH, 0>), dim3(P.ntiles), dim3(KH_PART_THREADS), ((nb1 + 1u) & ~1u) * 8 + nb1 * 8, t->stream, P)); } }
  out.rec12 = rec12 == 2 ? 2 : 0;
  if (B2 == 0) {
    out.rec = ar; out.part_off = off1; out.PB = PB; out.nparts = nparts;
    out.spare = tmp;
    HIPCHK(hipGetLastError());
    return KH_OK;
  }
  // second pass inside every first-pass segment
  { Launch L(t, "k_make_tiles");
    hipLaunchKernelGGL(k_make_tiles, dim3(1), dim3(1024), 0, t->stream, off1, nb1, tiles, ntiles_dev); }
  KhPartParams Q = P;
  Q.kbase = nullptr; Q.kstride = 0;
  Q.vbase = nullptr; Q.vstride = 0; Q.rec_in = ar;
  Q.tiles = tiles; Q.ntiles_dev = ntiles_dev; Q.ntiles = max_tiles;
  Q.shift = 0; Q.nb = nb2; Q.counts = counts2; Q.cursor = cur2; Q.orec = br;
  if (!full_hist) {
    { Launch L(t, "k_part_hist");
      if (rec12 == 2) { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_hist<HASH, true>), dim3(std::min<uint32_t>(max_tiles, 1024)), dim3(KH_PART_THREADS), nb2 * 4, t->stream, Q)); }
      else { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_hist<HASH>), dim3(std::min<uint32_t>(max_tiles, 1024)), dim3(KH_PART_THREADS), nb2 * 4, t->stream, Q)); } }
    { Launch L(t, "k_scan");
      hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, t->stream, counts2, (uint64_t)nparts, off2); }
  }
  HIPCHK(hipMemcpyAsync(cur2, off2, sizeof(uint64_t) * nparts, hipMemcpyDeviceToDevice, t->stream));
  { Launch L(t, "k_part_scatter");
    if (rec12 == 2) { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_scatter<HASH, 2>), dim3(max_tiles), dim3(KH_PART_THREADS), ((nb2 + 1u) & ~1u) * 8 + nb2 * 8, t->stream, Q)); }
    else { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_scatter<HASH, 0>), dim3(max_tiles), dim3(KH_PART_THREADS), ((nb2 + 1u) & ~1u) * 8 + nb2 * 8, t->stream, Q)); } }
  HIPCHK(hipGetLastError());
  out.rec = br; out.part_off = off2; out.PB = PB; out.nparts = nparts;
  out.spare = tmp;
  return KH_OK;
}

// capacity after `ncalls` insert() calls that add `dnew` new keys, the last of which first occurs at
// call index `last_first` (hashmap_robinhood.hpp:530 / hashmap_linearprobe.hpp:439: ONE doubling per
// call made while size >= max_load, duplicates included).  Precondition: at most one doubling is
// pending at the start (size < max_load(2*cap)); the caller peels single calls otherwise.
uint64_t capacity_after(const kh_table* t, uint64_t cap, uint64_t lsize, uint64_t ncalls, uint64_t dnew, uint64_t last_first) {
  if (ncalls == 0) return cap;
  uint64_t c = cap;
  if (lsize >= threshold(c, t->max_lf)) c <<= 1;                 // call 0
  const uint64_t fin = lsize + dnew;
  while (fin > threshold(c, t->max_lf)) c <<= 1;                 // thresholds passed on the way: a later new key follows
  if (dnew > 0 && fin == threshold(c, t->max_lf) && last_first + 1 < ncalls) c <<= 1;   // reached exactly, a later call follows
  return c;
}

// INS_PLUS .. INS_OR: the reducer inserts, INS_PLUS + kh_reduce_op.  Everything structural (which keys are new, capacity rule, list
// sizing, record kinds) asks is_reduce(); what only std::plus can do (a constant value of 1, the speculative one-launch forms) asks
// mode == INS_PLUS.
enum { INS_FIRST = 0, INS_UPDATE = 1, INS_PLUS = 2, INS_MIN = 3, INS_MAX = 4, INS_OR = 5 };
inline bool is_reduce(int mode) { return mode >= INS_PLUS; }
inline int reduce_op(int mode) { return is_reduce(mode) ? mode - INS_PLUS : 0; }      // KH_ROP_* == kh_reduce_op
// the speculative one-launch forms (k_build_fused, k_build_lean, the fused insert into a loaded table, k_insert_stream) fold first-wins
// or std::plus only: a min / max / or insert goes straight to the general path
inline bool one_launch_mode(int mode) { return mode == INS_FIRST || mode == INS_UPDATE || mode == INS_PLUS; }
inline const char* apply_label(int mode) { return mode == INS_PLUS ? "k_apply_plus" : "k_apply_reduce"; }
static_assert(KH_REDUCE_MIN == KH_ROP_MIN && KH_REDUCE_MAX == KH_ROP_MAX && KH_REDUCE_OR == KH_ROP_OR && KH_REDUCE_PLUS == KH_ROP_PLUS, "kh_reduce_op is the kernels' rop");
// flags of kh_insert_begin_ex / kh_wide_insert_begin_ex: the operation field (KH_INS_REDUCE(op)) counts only next to KH_INS_REDUCE_PLUS
inline bool ins_flags_ok(unsigned flags) {
  if (flags & ~(unsigned)(KH_INS_REDUCE_PLUS | KH_INS_REPEATABLE | KH_INS_REDUCE_OP_MASK)) return false;
  return (flags & KH_INS_REDUCE_PLUS) || !(flags & KH_INS_REDUCE_OP_MASK);
}
inline int ins_flags_mode(unsigned flags) {
  return (flags & KH_INS_REDUCE_PLUS) ? INS_PLUS + (int)((flags & KH_INS_REDUCE_OP_MASK) >> KH_INS_REDUCE_OP_SHIFT) : INS_FIRST;
}
// Pairs one internal pass takes.  A batch is the reference's SEQUENCE of insert() calls (one doubling decision per call), so cutting it
// into consecutive passes changes nothing observable; what it bounds is the workspace -- ~58 B per pair of a pass: a k-mer counter's
// file batch of 1.7e9 k-mers would otherwise ask for a 100 GB arena, whose hipMalloc alone costs 0.7 s (measured, scripts/kc_scale_probe.py).
// 2^30: a second pass is an insert into a LOADED table -- a re-layout of all of it (19 ms at 2^31 buckets) -- so 10^9 keys in one call stay one pass
// (scripts/scale_1e9.py: 40.9 ms with passes of 2^29, against the partition + build of a single pass).
const uint64_t g_max_pass = getenv("KH_MAX_PASS_RECORDS") ? std::max<uint64_t>(1024, std::min<uint64_t>(strtoull(getenv("KH_MAX_PASS_RECORDS"), nullptr, 10), 0xFFFFFFF0ull))
                                                          : (uint64_t(1) << 30);
bool g_disable_fused = getenv("KH_DISABLE_FUSED_BUILD") != nullptr;   // test hook: force the general path

// second half of an insert: the n pairs have been partitioned (one source per feed); de-dup, capacity decision, build
const kh_status KH_RETRY_EXACT = static_cast<kh_status>(100);      // internal: a histogram-free partition overflowed a slot
const kh_status KH_RETRY_DUPS = static_cast<kh_status>(101);       // internal: the sample an optimistic attempt was queued behind found duplicates
const bool g_sync_sample = getenv("KH_DISABLE_OPTIMISTIC_SAMPLE") != nullptr;      // test hook / A-B: the host reads every sample before it partitions
kh_status insert_finish(kh_table* t, KhSrcSet S, uint64_t n, uint32_t PB, uint64_t cap_u, int mode, uint64_t forced_cap,
                        ulonglong2* spare, uint64_t* n_new_out, uint64_t list_cap = 0);

// does the one-launch bulk build (k_build_fused, SRC 0) apply, and may it skip the LDS fold after a duplicate-free sample?
inline bool fused_build_applies(const kh_table* t, uint64_t cap_u, uint32_t PB) {
  return t->lsize == 0 && cap_u >= 2 * (uint64_t)KH_L && t->max_lf <= 0.9f && PB == log2u(cap_u >> KH_LB) && !g_disable_fused;
}
inline bool nodup_build_applies(const kh_table* t, uint64_t cap_u, uint32_t PB, int mode) {
  return fused_build_applies(t, cap_u, PB) && t->batch_nodup && (mode == INS_FIRST || mode == INS_PLUS) && !getenv("KH_DISABLE_NODUP");
}

// core of insert/update for one batch of device-resident input (n < 2^32 - 16)
kh_status insert_core(kh_table* t, const char* kbase, uint32_t kstride, const char* vbase, uint32_t vstride,
                      uint64_t n, int mode, uint64_t forced_cap, uint64_t* n_new_out) {
  *n_new_out = 0;
  if (n == 0) return KH_OK;
  const uint64_t cap_u = forced_cap ? forced_cap : capacity_after(t, t->cur.cap, t->lsize, n, n, n - 1);
  const uint32_t PB = cap_u > KH_L ? log2u(cap_u >> KH_LB) : 0u;
  if (PB > 22) return fail(t, KH_ERR_UNSUPPORTED, "batch would need more than 2^22 partitions");
  const size_t keep_blk = t->blk, keep_off = t->off;
  int first_attempt = 0;
  bool dup_heavy = false;
  double vf = 1.0;            // variance factor of the histogram-free slots (duplicates: see below)
  // ANY duplicate among the 65536 sampled keys sends the batch down the exact path: the fixed slots are sized for partition counts
  // that are Poisson in the number of RECORDS, and already a mean multiplicity of 1.5 (a k-mer counter's file batch at low coverage:
  // ~7 duplicate pairs in the sample, birthday-bound) widens them enough to overflow a slot somewhere among 2^19 partitions --
  // measured: every such batch paid a discarded 7.5 ms partition attempt; the histogram sweep of the exact path costs 2.5 ms
  // ... UNLESS the slots are sized for the duplicates: a partition then fills key by key, E[m^2] / E[m] records at a time, and that factor
  // follows from the sample -- d duplicates among S sampled keys of n say sum m (m - 1) / n = 2 n d / S^2 (the reference benchmark's x5.5 input:
  // 129 duplicates -> 7.0; a k-mer counter's batch at coverage 1.5: 7 -> 2.5).  Taken at its upper end (d + 3 sqrt(d) + 3) and only while the
  // slot stays below twice the mean; an overflow after all repeats the batch with exact offsets as before.
  auto decide = [&](uint32_t dsample) {
    if (dsample >= 1u) {
      dup_heavy = true;
      const double d_ub = (double)dsample + 3.0 * std::sqrt((double)dsample) + 3.0;
      const double f = 1.0 + 2.0 * (double)n * d_ub / ((double)KH_SAMPLE_N * (double)KH_SAMPLE_N);
      const double mean = (double)n / (double)(uint64_t(1) << PB);
      if (!getenv("KH_DISABLE_DUP_SLACK") && (double)slack_slot(mean, f) <= 2.0 * mean) vf = f;
      else first_attempt = 1;
    }
    t->batch_nodup = dsample == 0u;
  };
  // histogram-free partition only for batches a sample finds (nearly) free of duplicates.  Ahead of the one-launch bulk build the host does
  // not wait for the sample: it queues what a clean sample would make it choose (vf = 1, 12-byte records where nodup_build_applies) directly
  // behind it, every kernel of that attempt tests the sample's word and returns at once if it is not zero, and the word reaches the host with
  // the build's control words (launch_fused) -- a batch with duplicates then pays one discarded round trip and goes on exactly as below.
  // Every other path (a loaded table, one chunk, a reducer other than plus: the general path decides on the host first) reads the sample now.
  const bool slackable = part_buffer_records(n, PB, true) != n;
  bool optimistic = slackable && fused_build_applies(t, cap_u, PB) && one_launch_mode(mode) && !g_sync_sample;
  if (slackable && !optimistic) {
    unsigned long long* sset; uint32_t* dups;      // (adjacent: one fill)
    { char* b; TAKE(b, char, sizeof(unsigned long long) * KH_SAMPLE_SET + 256);
      sset = reinterpret_cast<unsigned long long*>(b); dups = reinterpret_cast<uint32_t*>(b + sizeof(unsigned long long) * KH_SAMPLE_SET);
      HIPCHK(hipMemsetAsync(b, 0, sizeof(unsigned long long) * KH_SAMPLE_SET + 256, t->stream)); }
    { Launch L(t, "k_sample_dups");
      hipLaunchKernelGGL(k_sample_dups, dim3(KH_SAMPLE_N / 256), dim3(256), 0, t->stream, kbase, kstride, n, sset, dups, KhCursorInit{}); }
    HIPCHK(hipMemcpyAsync(t->hpin + 31, dups, 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    decide((uint32_t)t->hpin[31]);
  } else if (!slackable) first_attempt = 1;
  for (int attempt = first_attempt; attempt < 2; ++attempt) {
    const bool slack = attempt == 0;          // histogram-free first; exact offsets if a partition outgrew its slot (skewed keys)
    const uint64_t m = part_buffer_records(n, PB, slack, vf);
    t->blk = keep_blk; t->off = keep_off;     // (the sample set, an attempt before this one: dead)
    SampleRun sample;
    const size_t rec0 = t->recs.size();
    if (optimistic) {
      // ONE fill for the call: the build's control block, the sample's count word and its set, adjacent
      const size_t fb = (fused_blk_bytes((uint32_t)(cap_u >> KH_LB)) + 255) & ~size_t(255), hb = fb + 256 + sizeof(unsigned long long) * KH_SAMPLE_SET;
      char* head; TAKE(head, char, hb);
      HIPCHK(hipMemsetAsync(head, 0, hb, t->stream));
      t->fused_blk = head; t->fused_blk_bytes = fused_blk_bytes((uint32_t)(cap_u >> KH_LB));
      sample.dups = reinterpret_cast<uint32_t*>(head + fb); sample.set = reinterpret_cast<unsigned long long*>(head + fb + 256);
      t->sample_dups = sample.dups;
      t->batch_nodup = true;
    }
    // no duplicate in the sample and an empty table ahead of the one-launch build: the records need no stream position
    // (12 bytes instead of 16); whatever that build cannot take (a duplicate after all, a dense chunk) repeats the batch
    const bool rec12 = slack && t->batch_nodup && nodup_build_applies(t, cap_u, PB, mode);
    // a counting insert (Reducer = std::plus, every value 1) of a batch the sample found heavy in duplicates -- the k-mer counter's
    // batches: the records are the keys alone (8 bytes: neither value nor position is needed), and the general path takes them
    // directly (the one-launch forms speculate on few duplicates: hopeless here)
    const bool rec8 = !rec12 && dup_heavy && mode == INS_PLUS && vbase == nullptr && !getenv("KH_DISABLE_REC8");
    const int kind = rec12 ? 1 : rec8 ? 2 : 0;
    ulonglong2 *tmp, *fin, *spare;
    { char *a, *b; const size_t rb = kind == 1 ? sizeof(KhRec12) : kind == 2 ? sizeof(KhRec8) : sizeof(ulonglong2);
      TAKE(a, char, m * rb); TAKE(b, char, m * rb);
      tmp = reinterpret_cast<ulonglong2*>(a); fin = reinterpret_cast<ulonglong2*>(b); spare = tmp;
      if (kind == 2) { char* c; TAKE(c, char, m * 12); spare = reinterpret_cast<ulonglong2*>(c); } }     // (lists of distinct keys + counts: 12 bytes per entry)
    Partitioned R;
    kh_status st = partition_batch(t, kbase, kstride, vbase, vstride, mode == INS_PLUS ? 1u : 0u, n, 0, PB, tmp, fin, R, slack, kind, nullptr, false, vf,
                                   optimistic ? &sample : nullptr);
    if (st == KH_OK) {
      KhSrcSet S;
      memset(&S, 0, sizeof(S));
      S.rec[0] = R.rec; S.off[0] = R.part_off; S.n = 1; S.merged_off = R.part_off; S.slot[0] = R.slot; S.cur[0] = R.cursor;
      S.rec12 = (uint32_t)R.rec12;
      t->part_overflow = R.overflow; t->batch_vf = vf;
      st = insert_finish(t, S, n, PB, cap_u, mode, forced_cap, spare, n_new_out, m);
    }
    t->part_overflow = nullptr; t->batch_nodup = false; t->batch_vf = 1.0; t->sample_dups = nullptr; t->fused_blk = nullptr;
    const bool was_optimistic = optimistic;
    optimistic = false;
    if (st == KH_RETRY_DUPS && was_optimistic) {      // the sample found duplicates: nothing was written; decide as above and start over
      decide((uint32_t)t->hpin[31]);
      // (profile: the launches that returned at once do not count as passes or builds; they keep their times under a label of their own)
      for (size_t i = rec0; i < t->recs.size(); ++i) if (strcmp(t->recs[i].name, "k_sample_dups")) t->recs[i].name = "k_attempt_skipped";
      attempt = first_attempt - 1;
      continue;
    }
    if (st != KH_RETRY_EXACT) return st;
  }
  return fail(t, KH_ERR_HIP, "internal: exact partition reported a slot overflow");
}

kh_status insert_finish(kh_table* t, KhSrcSet S, uint64_t n, uint32_t PB, uint64_t cap_u, int mode, uint64_t forced_cap,
                        ulonglong2* spare, uint64_t* n_new_out, uint64_t list_cap) {
  *n_new_out = 0;
  if (list_cap < n) list_cap = n;       // entries the per-partition output lists span (slots of a histogram-free partition: > n)
  kh_status st = KH_OK;
  const uint32_t nparts = 1u << PB;
  struct { uint32_t nparts; } R; R.nparts = nparts;
  // ---- fused bulk build: empty table, moderate load factor, at least two chunks.  Speculates that the capacity the
  // reference's rule yields equals cap_u (true when the batch holds few duplicates); otherwise falls through.
  // (not for a batch whose sample says that a key comes E[m^2]/E[m] >= 2 times: the build speculates that every pair is a new key, its first 64
  //  chunks would vote it down -- 0.11 ms of launches for the reference benchmark's own input; a batch that is mostly distinct after all is
  //  merely built by the general path)
  if (fused_build_applies(t, cap_u, PB) && one_launch_mode(mode) && S.rec12 != 2 && !(t->batch_vf >= 2.0)) {
    const uint32_t nch = (uint32_t)(cap_u >> KH_LB);
    KhSlots nw;
    st = fresh_slots(t, cap_u, nw);
    if (st != KH_OK) return st;
    KhFusedParams F;
    memset(&F, 0, sizeof(F));
    F.src = S; F.PB = PB;
    F.mode = mode == INS_PLUS ? KH_DEDUP_PLUS : KH_DEDUP_FIRST;
    F.base_size = 0;
    F.n_total = n;
    F.nodup = nodup_build_applies(t, cap_u, PB, mode) ? 1 : 0;
    // giving up early only makes sense if a smaller capacity is possible at all (an insert never shrinks the table)
    F.half_max_load = (cap_u >> 1) >= t->cur.cap ? threshold(cap_u >> 1, t->max_lf) : 0;
    FusedRun run;
    { kh_status fs = launch_fused(t, 0, F, nw, PB, "k_build_fused", &run); if (fs != KH_OK) return fs; }
    if (F.skip && (uint32_t)t->hpin[31]) { retire_slots(t, nw); return KH_RETRY_DUPS; }      // (every kernel of the attempt returned at once)
    if (t->part_overflow && (uint32_t)t->hpin[30]) { retire_slots(t, nw); return KH_RETRY_EXACT; }
    unsigned long long* totals = run.totals;
    const uint64_t fd = t->hpin[0];
    // (12-byte records: accepted only if all n keys were distinct, so the last call is the last first occurrence)
    const uint64_t flast = (mode == INS_PLUS || S.rec12) ? n - 1 : (t->hpin[1] ? t->hpin[1] - 1 : 0);
    const uint32_t* ff = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(t->hpin) + 64);
    bool bad = S.rec12 && fd != n;
    for (int i = 0; i < KH_NFLAGS; ++i) bad = bad || ff[i] != 0;
    if (!bad && capacity_after(t, t->cur.cap, t->lsize, n, fd, flast) == cap_u) {
      adopt_slots(t, nw);
      t->lsize = fd;
      *n_new_out = fd;
      if (mode == INS_UPDATE) {
        KhDedupParams A;
        memset(&A, 0, sizeof(A));
        A.src = S; A.T = narrow(t->cur); A.seed = t->seed; A.table_empty = 0; A.mode = KH_DEDUP_LAST;
        uint32_t* cn; TAKE(cn, uint32_t, R.nparts);
        A.cnt_new = cn; A.max_idx_plus1 = totals; A.flags = F.flags; A.count_cap = 0; A.PB = PB;
        Launch L(t, "k_dedup_assign");
        KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_dedup<KIND, HASH>), dim3(R.nparts), dim3(KH_CHUNK_THREADS), 0, t->stream, A));
        HIPCHK(hipGetLastError());
      }
      return KH_OK;
    }
    if (getenv("KH_DEBUG_FUSED"))
      fprintf(stderr, "[kmerhash_amd] fused build rejected: n=%llu dnew=%llu cap_u=%llu cap_rule=%llu flags=%u %u %u %u %u est=%u/%u/%u\n", (unsigned long long)n,
              (unsigned long long)fd, (unsigned long long)cap_u, (unsigned long long)capacity_after(t, t->cur.cap, t->lsize, n, fd, flast), ff[0], ff[1], ff[2], ff[3], ff[4],
              reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(t->hpin) + 32)[1], reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(t->hpin) + 32)[0],
              reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(t->hpin) + 32)[2]);
    retire_slots(t, nw);      // speculation failed (duplicates, skew): the buffer becomes the spare, general path below
    if (S.rec12 == 1) return KH_RETRY_EXACT;      // (the general path needs the stream positions: repartition with 16-byte records)
  }
  if (S.rec12 == 1) return fail(t, KH_ERR_HIP, "internal: 12-byte records outside the bulk build");
  // ---- fused insert into a NON-empty Robin Hood table: every chunk stages its current elements (home from the info byte)
  // next to the batch's records of the same chunk, folds them together (an element of the table beats every record), and
  // lays the chunk out -- no membership probes at random into HBM (k_dedup), no separate re-layout.  Speculates, like the
  // bulk build, that the capacity the reference's rule yields equals cap_u.
  // (first-wins and std::plus only, like every one-launch form: one_launch_mode; spelled out here because kh_update has its own way)
  if (t->lsize > 0 && S.rec12 != 2 && (mode == INS_FIRST || mode == INS_PLUS) && !forced_cap && !g_disable_fused_rebuild &&
      t->cur.cap >= 2 * (uint64_t)KH_L && (cap_u == t->cur.cap || cap_u == 2 * t->cur.cap) && t->max_lf <= 0.9f &&
      PB == log2u(cap_u >> KH_LB) && t->lsize + n <= threshold(cap_u, 0.92f)) {
    const size_t keep_blk = t->blk, keep_off = t->off;
    const uint32_t nch = (uint32_t)(cap_u >> KH_LB);
    KhSlots nw;
    st = fresh_slots(t, cap_u, nw);
    if (st != KH_OK) return st;
    KhFusedParams F;
    memset(&F, 0, sizeof(F));
    F.src = S; F.PB = PB;
    F.mode = mode == INS_PLUS ? KH_DEDUP_PLUS : KH_DEDUP_FIRST;
    F.n_total = n;
    F.base_size = t->lsize;
    // giving up early only makes sense if the smaller capacity is possible at all (an insert never shrinks the table)
    F.half_max_load = (cap_u >> 1) >= t->cur.cap ? threshold(cap_u >> 1, t->max_lf) : 0;
    F.R.Old = narrow(t->cur); F.R.PB = PB;
    FusedRun run;
    // (Robin Hood at equal capacity, one source of 16-byte records, a chunk's records fit two per lane: the ordered-stream kernel; else the staging form)
    const bool ordered = t->kind == KHK_RH && cap_u == t->cur.cap && S.n == 1 && S.rec12 == 0 &&
                         (S.slot[0] ? S.slot[0] <= KH_IS_MAXR : n / (uint64_t(1) << PB) <= KH_IS_MAXR / 2) && !getenv("KH_DISABLE_ORDERED_INSERT");
    { kh_status fs = launch_fused(t, ordered ? 5 : 2, F, nw, PB, "k_insert_fused", &run); if (fs != KH_OK) return fs; }
    if (t->part_overflow && (uint32_t)t->hpin[30]) { retire_slots(t, nw); return KH_RETRY_EXACT; }
    const uint64_t total = t->hpin[0];
    const uint64_t fd = total >= t->lsize ? total - t->lsize : 0;
    const uint64_t flast = mode == INS_PLUS ? n - 1 : (t->hpin[1] ? t->hpin[1] - 1 : 0);
    const uint32_t* ff = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(t->hpin) + 64);
    bool bad = total < t->lsize;
    for (int i = 0; i < KH_NFLAGS; ++i) bad = bad || ff[i] != 0;
    if (!bad && capacity_after(t, t->cur.cap, t->lsize, n, fd, flast) == cap_u) {
      adopt_slots(t, nw);
      t->lsize = total;
      *n_new_out = fd;
      return KH_OK;
    }
    if (getenv("KH_DEBUG_FUSED"))
      fprintf(stderr, "[kmerhash_amd] fused insert rejected: n=%llu size=%llu total=%llu cap_u=%llu cap_rule=%llu flags=%u %u %u %u %u\n", (unsigned long long)n,
              (unsigned long long)t->lsize, (unsigned long long)total, (unsigned long long)cap_u,
              (unsigned long long)capacity_after(t, t->cur.cap, t->lsize, n, fd, flast), ff[0], ff[1], ff[2], ff[3], ff[4]);
    retire_slots(t, nw);
    t->blk = keep_blk; t->off = keep_off;
  }
  uint32_t* cnt_new; uint64_t* noff; unsigned long long* scal; uint32_t* flags;
  TAKE(cnt_new, uint32_t, R.nparts); TAKE(noff, uint64_t, R.nparts + 1); TAKE(scal, unsigned long long, 4);
  TAKE(flags, uint32_t, KH_NFLAGS);
  HIPCHK(hipMemsetAsync(scal, 0, sizeof(unsigned long long) * 4, t->stream));
  HIPCHK(hipMemsetAsync(flags, 0, sizeof(uint32_t) * KH_NFLAGS, t->stream));
  KhDedupParams D;
  D.src = S;
  // outputs go into the scratch record buffer (16 B per input record): keys in its first half, values behind them
  D.nk = reinterpret_cast<uint64_t*>(spare); D.nv = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(spare) + list_cap * 8);
  D.cnt_new = cnt_new; D.max_idx_plus1 = scal;
  // speculate that the capacity decided below equals cap_u (true whenever the batch holds few duplicates): then the
  // de-dup kernel already produces the chunk counts and k_chunk_count is skipped
  PreCount pre; pre.homecnt = nullptr; pre.sumA = nullptr; pre.sumN = nullptr;
  const bool fuse = t->lsize == 0;
  if (fuse) {
    TAKE(pre.homecnt, uint16_t, cap_u); TAKE(pre.sumA, long long, R.nparts); TAKE(pre.sumN, long long, R.nparts);
  }
  D.count_cap = fuse ? cap_u : 0; D.PB = PB; D.homecnt = pre.homecnt; D.sumA = pre.sumA; D.sumN = pre.sumN;
  D.T = narrow(t->cur); D.seed = t->seed; D.table_empty = t->lsize == 0 ? 1 : 0; D.mode = is_reduce(mode) ? KH_DEDUP_PLUS : KH_DEDUP_FIRST; D.flags = flags;
  D.rop = reduce_op(mode);
  D.xcd_group = 0;
  // Reducer = std::plus into a non-empty table: k_dedup only LISTS the sums of the keys the table already holds; they are added
  // (k_apply_reduce) once nothing can discard this attempt any more -- a histogram-free partition that overflowed repeats the whole
  // batch, and a repeatable streamed insert promises "table unchanged" with KH_ERR_RETRY
  // (any Reducer; min / max / or are not taken back by a second pass with the sign turned but restored from the values the apply
  //  step leaves in the list: k_apply_reduce)
  const bool plus_live = is_reduce(mode) && t->lsize > 0;
  D.cnt_upd = nullptr;
  if (plus_live) TAKE(D.cnt_upd, uint32_t, R.nparts);
  // with exact partition offsets nothing can discard the attempt before the re-layout: the sums are added inside k_dedup (its
  // membership probes have the slot in hand) and the list only serves to take them back should the re-layout fail
  // ... and so they are behind a histogram-free partition once its overflow flag has been read clean: the partition is complete in stream
  // order, so the flag is final -- one small copy + wait (tens of microseconds) instead of a k_apply_reduce pass at random over the table
  // (7 ms per 4.5e8-k-mer batch of the k-mer counter, measured)
  bool overflow_clean = t->part_overflow == nullptr;
  if (plus_live && !overflow_clean && !getenv("KH_DISABLE_PLUS_IMMEDIATE")) {
    t->hpin[30] = 0;
    HIPCHK(hipMemcpyAsync(t->hpin + 30, t->part_overflow, 4, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    if ((uint32_t)t->hpin[30]) return KH_RETRY_EXACT;
    overflow_clean = true;
  }
  D.plus_immediate = (plus_live && overflow_clean && !getenv("KH_DISABLE_PLUS_IMMEDIATE")) ? 1 : 0;
  if (t->lsize > 0 && t->cur.cap > KH_L && !getenv("KH_DISABLE_XCD_GROUP")) {
    // partitions are cut for cap_u, the probes go to the (smaller) current table: 2^(PB - k) consecutive partitions share one of its chunks
    const uint32_t k_tab = log2u(t->cur.cap >> KH_LB);
    if (PB > k_tab) {
      const uint32_t G = std::min<uint32_t>(1u << (PB - k_tab), 16u);
      if (R.nparts % (8u * G) == 0) D.xcd_group = G;
    }
  }
  { Launch L(t, "k_dedup");
    if (S.rec12 == 2) { KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_dedup<KIND, HASH, true>), dim3(R.nparts), dim3(KH_CHUNK_THREADS), 0, t->stream, D)); }
    else { KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_dedup<KIND, HASH>), dim3(R.nparts), dim3(KH_CHUNK_THREADS), 0, t->stream, D)); } }
  { Launch L(t, "k_scan");
    hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, t->stream, cnt_new, (uint64_t)R.nparts, noff); }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t->hpin, noff + R.nparts, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipMemcpyAsync(t->hpin + 1, scal, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipMemcpyAsync(t->hpin + 2, flags, sizeof(uint32_t) * KH_NFLAGS, hipMemcpyDeviceToHost, t->stream));
  t->hpin[30] = 0;
  if (t->part_overflow) HIPCHK(hipMemcpyAsync(t->hpin + 30, t->part_overflow, 4, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  if (t->part_overflow && (uint32_t)t->hpin[30]) return KH_RETRY_EXACT;
  const uint64_t dnew = t->hpin[0];
  const uint64_t last_first = is_reduce(mode) ? n - 1 : (t->hpin[1] ? t->hpin[1] - 1 : 0);
  if (reinterpret_cast<const uint32_t*>(t->hpin + 2)[KH_FLAG_INTERNAL])
    return fail(t, KH_ERR_HIP, kDedupOverflowText);
  auto apply_plus = [&](int sign) {
    Launch L(t, apply_label(mode));
    hipLaunchKernelGGL(k_apply_reduce, dim3(std::min<uint32_t>(R.nparts, 4096u)), dim3(256), 0, t->stream, narrow(t->cur).s, S.merged_off, (const uint32_t*)D.cnt_upd,
                       (const uint64_t*)D.nk, D.nv, R.nparts, sign, D.rop);
  };
  if (plus_live) apply_plus(+1);
  const uint64_t new_cap = forced_cap ? forced_cap : capacity_after(t, t->cur.cap, t->lsize, n, dnew, last_first);
  if (dnew > 0 || new_cap != t->cur.cap) {
    // a chunk of the new table owns 2^(PB-k) consecutive partitions; read their lists in place when that is a
    // handful, gather them into one dense list when the capacity shrank far below the partitioning capacity
    const uint32_t k_new = new_cap > KH_L ? log2u(new_cap >> KH_LB) : 0u;
    const uint64_t* ck = nullptr; const uint32_t* cv = nullptr; const uint64_t* lo = nullptr; const uint32_t* lc = nullptr;
    if (dnew > 0) {
      if (PB - k_new <= 3) { ck = D.nk; cv = D.nv; lo = S.merged_off; lc = cnt_new; }
      else {
        uint64_t* gk; uint32_t* gv;
        TAKE(gk, uint64_t, dnew); TAKE(gv, uint32_t, dnew);
        Launch L(t, "k_gather_new");
        hipLaunchKernelGGL(k_gather_new, dim3(R.nparts), dim3(256), 0, t->stream, S.merged_off, noff, D.nk, D.nv, gk, gv);
        ck = gk; cv = gv; lo = noff; lc = nullptr;
      }
    }
    const bool pre_ok = fuse && new_cap == cap_u && !reinterpret_cast<const uint32_t*>(t->hpin + 2)[KH_FLAG_FUSE_INVALID];
    st = rebuild(t, new_cap, ck, cv, lo, lc, PB, false, t->lsize + dnew, pre_ok ? &pre : nullptr);
    if (st != KH_OK) {        // the table keeps its layout: it must keep its values too
      if (plus_live) { apply_plus(-1); hipStreamSynchronize(t->stream); }
      return st;
    }
    t->lsize += dnew;
  }
  if (mode == INS_UPDATE) {   // update(k,v): existing keys take the value of their LAST occurrence in the batch
    D.T = narrow(t->cur); D.table_empty = 0; D.mode = KH_DEDUP_LAST; D.count_cap = 0;
    Launch L(t, "k_dedup_assign");
    KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_dedup<KIND, HASH>), dim3(R.nparts), dim3(KH_CHUNK_THREADS), 0, t->stream, D));
    HIPCHK(hipGetLastError());
  }
  *n_new_out = dnew;
  return KH_OK;
}

// device-resident pairs -> table; the batch is cut only where the reference's one-doubling-per-call rule or the 32-bit
// record index demands it.  What the arena holds at entry stays (staged input); the rest is reused per sub-batch.
kh_status insert_device(kh_table* t, const char* kb, uint32_t kstride, const char* vb, uint32_t vstride, uint64_t n, int mode,
                        uint64_t* total_new_out) {
  const size_t keep_blk = t->blk, keep_off = t->off;
  uint64_t total_new = 0, done = 0;
  kh_status st = KH_OK;
  while (done < n && st == KH_OK) {
    // more than one doubling pending (only after set_max_load_factor / an LP shrink): the reference doubles
    // once per insert() call, so peel single calls until at most one is pending
    uint64_t take = n - done;
    if (t->lsize >= threshold(t->cur.cap << 1, t->max_lf)) take = 1;
    if (take > g_max_pass) take = g_max_pass;          // 32-bit record indices; bounded workspace (see g_max_pass)
    t->blk = keep_blk; t->off = keep_off;
    uint64_t nn = 0;
    if (take == 1 && t->lsize >= threshold(t->cur.cap << 1, t->max_lf)) {
      // single call: insert() runs rehash(2c) once (:530 / LP :439).  The LP rehash copies without looking at the load: exactly
      // one doubling.  The RH rehash re-inserts through insert() (:432-464), whose own doubling check fires again while the copy
      // is under way: the capacity ends where all lsize elements fit below max_load (the rule do_rehash applies)
      uint64_t c = t->cur.cap << 1;
      if (t->kind == KHK_RH) while (t->lsize > threshold(c, t->max_lf)) c <<= 1;
      st = insert_core(t, kb + done * kstride, kstride, vb ? vb + done * vstride : nullptr, vstride, 1, mode, c, &nn);
    } else {
      st = insert_core(t, kb + done * kstride, kstride, vb ? vb + done * vstride : nullptr, vstride, take, mode, 0, &nn);
    }
    total_new += nn;
    done += take;
  }
  *total_new_out = total_new;
  return st;
}

// A handful of keys applied in place by one lane (k_small_batch) instead of re-laying out the table.  *done = keys applied
// (all of them unless a Robin Hood displacement chain would pass distance 127: the caller continues on the general path).
#define KH_SMALL_N 16
const bool g_disable_small = getenv("KH_DISABLE_SMALL_BATCH") != nullptr;      // test hook
kh_status small_batch(kh_table* t, const char* kb, uint32_t kstride, const char* vb, uint32_t vstride, uint32_t vconst, uint32_t n, int op,
                      uint64_t* changed, uint32_t* done, int rop = KH_ROP_PLUS) {
  unsigned long long* out; uint32_t* flags;
  TAKE(out, unsigned long long, 2); TAKE(flags, uint32_t, KH_NFLAGS);
  HIPCHK(hipMemsetAsync(out, 0, 16, t->stream));
  HIPCHK(hipMemsetAsync(flags, 0, sizeof(uint32_t) * KH_NFLAGS, t->stream));
  { Launch L(t, "k_small_batch");
    KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_small_batch<KIND, HASH>), dim3(1), dim3(64), 0, t->stream, narrow(t->cur), kb, kstride, vb, vstride,
                                                             vconst, n, op, t->seed, out, flags, rop)); }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t->hpin, out, 16, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipMemcpyAsync(t->hpin + 2, flags, sizeof(uint32_t) * KH_NFLAGS, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  if (reinterpret_cast<const uint32_t*>(t->hpin + 2)[KH_FLAG_INTERNAL]) return fail(t, KH_ERR_FULL, "ERROR: did not find a slot to insert into (hashmap_linearprobe.hpp:503)");
  *changed = t->hpin[0];
  *done = (uint32_t)t->hpin[1];
  return KH_OK;
}

// ---- batches of middle size applied in place (Robin Hood; kh_kernels.h "Batches of middle size") --------------------------
// Taken when no call of the batch can trigger a doubling (size + n <= max_load), the batch is small against the table (at
// most ~1 key per region of 512 slots) and the load stays moderate (clusters much shorter than a region): cost O(batch)
// instead of the O(table) re-layout.
const bool g_disable_inplace = getenv("KH_DISABLE_INPLACE") != nullptr;      // test hook: force the re-layout
inline bool inplace_ok(const kh_table* t, uint64_t n) {
  return !g_disable_inplace && t->kind == KHK_RH && n > KH_SMALL_N && t->lsize > 0 && t->cur.cap >= 16 * (uint64_t)KH_IP_L &&
         n <= (t->cur.cap >> KH_IP_LB) && t->lsize + n <= threshold(t->cur.cap, 0.85f);
}
inline size_t ws_inplace(const kh_table* t, uint64_t n) { return n * 32 + (n <= 32768 ? n * 32 * 32 : 0) + (t->cur.cap >> KH_IP_LB) * (size_t)(KH_IP_CAP * 16 + 8) + (size_t(1) << 20); }
// result block of the in-place passes (device, zero at launch; copied to t->hpin in one piece)
struct IpResult { unsigned long long defer1, defer2, done, n_in; uint32_t flags[KH_NFLAGS]; };
// the three passes over the input list `src` describes (fields in_* / part_* / n of P0): regions, regions shifted by half, one lane
template <int OP>
kh_status inplace_passes(kh_table* t, const KhInplaceParams& src, uint64_t n_max, IpResult** res_out) {
  const uint32_t regions = (uint32_t)(t->cur.cap >> KH_IP_LB);
  // one zero-initialised block: result + the two counter arrays
  char* z; ulonglong2 *bins, *defer1, *defer2;
  const size_t zbytes = sizeof(IpResult) + sizeof(uint32_t) * 2 * (size_t)regions;
  TAKE(z, char, zbytes);
  TAKE(bins, ulonglong2, (size_t)regions * KH_IP_CAP);
  TAKE(defer1, ulonglong2, n_max); TAKE(defer2, ulonglong2, n_max);
  HIPCHK(hipMemsetAsync(z, 0, zbytes, t->stream));
  IpResult* res = reinterpret_cast<IpResult*>(z);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(z + sizeof(IpResult));
  KhInplaceParams P = src;
  P.T = narrow(t->cur); P.seed = t->seed; P.bins = bins; P.n_done = &res->done; P.n_in = &res->n_in; P.flags = res->flags;
  const uint32_t apply_grid = (regions + KH_IP_THREADS - 1) / KH_IP_THREADS;
  // pass 1: regions [r L, (r+1) L)
  P.ofs = 0; P.cnt = cnt; P.defer = defer1; P.n_defer = &res->defer1;
  { Launch L(t, "k_ip_bin");
    const uint32_t grid = P.part_off ? std::min<uint32_t>(P.nparts, 4096u) : grid_for(n_max, 256);
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_ip_bin<HASH>), dim3(grid), dim3(256), 0, t->stream, P)); }
  { Launch L(t, "k_ip_apply");
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_ip_apply<HASH, OP>), dim3(apply_grid), dim3(KH_IP_THREADS), 0, t->stream, P)); }
  // pass 2: what crossed a boundary, regions shifted by half a region
  P.ofs = KH_IP_L / 2; P.in_k = nullptr; P.in_v = nullptr; P.part_off = nullptr; P.in_rec = defer1; P.n = 0; P.n_dev = &res->defer1;
  P.cnt = cnt + regions; P.defer = defer2; P.n_defer = &res->defer2;
  { Launch L(t, "k_ip_bin2");
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_ip_bin<HASH>), dim3(grid_for(std::max<uint64_t>(n_max / 8, 256), 256)), dim3(256), 0, t->stream, P)); }
  { Launch L(t, "k_ip_apply2");
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_ip_apply<HASH, OP>), dim3(apply_grid), dim3(KH_IP_THREADS), 0, t->stream, P)); }
  // pass 3: the rest, one lane
  P.in_rec = defer2; P.n_dev = &res->defer2;
  { Launch L(t, "k_ip_serial");
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_ip_serial<HASH, OP>), dim3(1), dim3(64), 0, t->stream, P)); }
  HIPCHK(hipGetLastError());
  *res_out = res;
  return KH_OK;
}

kh_status insert_inplace(kh_table* t, const char* kb, uint32_t kstride, const char* vb, uint32_t vstride, uint64_t n, int mode, uint64_t* n_new_out) {
  *n_new_out = 0;
  // equal keys must meet: partition by a few hash bits into pieces of ~1024 records (one pass), fold duplicates in LDS and
  // test membership against the table (k_dedup: updates / sums of EXISTING keys happen there); what comes out are the
  // batch's distinct NEW keys, one list per partition, which the binning kernel reads where they lie
  uint32_t PB = 0;
  while (PB < 11 && (n >> PB) > 1024) ++PB;
  Partitioned R;
  kh_status st = KH_OK;
  uint64_t list_cap = n;                       // entries the per-partition output lists of k_dedup span
  if (n <= 32768) {
    // one launch: workgroup q keeps partition q in its own slot of n records (k_part_direct)
    const uint32_t nparts = 1u << PB;
    list_cap = (uint64_t)nparts * n;
    ulonglong2 *rec, *spare; unsigned long long* cur; uint64_t* starts;
    TAKE(rec, ulonglong2, list_cap); TAKE(spare, ulonglong2, list_cap); TAKE(cur, unsigned long long, nparts); TAKE(starts, uint64_t, (size_t)nparts + 1);
    { Launch L(t, "k_part_direct");
      KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_part_direct<HASH>), dim3(nparts), dim3(512), 0, t->stream, kb, kstride, vb, vstride,
                                                 mode == INS_PLUS ? 1u : 0u, n, t->seed, PB, rec, cur, starts)); }
    HIPCHK(hipGetLastError());
    R.rec = rec; R.part_off = starts; R.PB = PB; R.nparts = nparts; R.spare = spare; R.slot = n; R.cursor = cur; R.overflow = nullptr;
  } else {
    ulonglong2 *tmp, *fin;
    TAKE(tmp, ulonglong2, n); TAKE(fin, ulonglong2, n);
    st = partition_batch(t, kb, kstride, vb, vstride, mode == INS_PLUS ? 1u : 0u, n, 0, PB, tmp, fin, R);
    if (st != KH_OK) return st;
  }
  KhSrcSet S;
  memset(&S, 0, sizeof(S));
  S.rec[0] = R.rec; S.off[0] = R.part_off; S.n = 1; S.merged_off = R.part_off; S.slot[0] = R.slot; S.cur[0] = R.cursor;
  uint32_t* cnt_new;
  TAKE(cnt_new, uint32_t, R.nparts);
  KhInplaceParams src;
  memset(&src, 0, sizeof(src));
  src.in_k = reinterpret_cast<uint64_t*>(R.spare); src.in_v = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(R.spare) + list_cap * 8);
  src.part_off = R.part_off; src.part_cnt = cnt_new; src.nparts = R.nparts;
  KhDedupParams D;
  memset(&D, 0, sizeof(D));
  D.src = S;
  D.nk = const_cast<uint64_t*>(src.in_k); D.nv = const_cast<uint32_t*>(src.in_v);
  D.cnt_new = cnt_new; D.count_cap = 0; D.PB = PB;
  D.T = narrow(t->cur); D.seed = t->seed; D.table_empty = 0; D.mode = is_reduce(mode) ? KH_DEDUP_PLUS : KH_DEDUP_FIRST;
  D.rop = reduce_op(mode);
  char* zpre;                   // k_dedup's scalar and flag words
  TAKE(zpre, char, 64);
  HIPCHK(hipMemsetAsync(zpre, 0, 64, t->stream));
  D.max_idx_plus1 = reinterpret_cast<unsigned long long*>(zpre); D.flags = reinterpret_cast<uint32_t*>(zpre + 32);
  if (is_reduce(mode)) { TAKE(D.cnt_upd, uint32_t, R.nparts); D.plus_immediate = getenv("KH_DISABLE_PLUS_IMMEDIATE") ? 0 : 1; }      // (nothing discards an in-place batch)
  { Launch L(t, "k_dedup");
    KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_dedup<KIND, HASH>), dim3(R.nparts), dim3(KH_CHUNK_THREADS), 0, t->stream, D)); }
  if (is_reduce(mode)) {      // reductions of the keys the table already holds (listed by k_dedup; nothing can discard an in-place batch)
    Launch L(t, apply_label(mode));
    hipLaunchKernelGGL(k_apply_reduce, dim3(std::min<uint32_t>(R.nparts, 4096u)), dim3(256), 0, t->stream, narrow(t->cur).s, (const uint64_t*)R.part_off, (const uint32_t*)D.cnt_upd,
                       (const uint64_t*)D.nk, D.nv, R.nparts, 1, D.rop);
  }
  IpResult* res = nullptr;
  st = inplace_passes<KH_IP_INSERT>(t, src, n, &res);
  if (st != KH_OK) return st;
  if (mode == INS_UPDATE) {   // update(k,v): every key of the batch is in the table now; it takes the value of its LAST occurrence
    D.mode = KH_DEDUP_LAST;
    Launch L(t, "k_dedup_assign");
    KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_dedup<KIND, HASH>), dim3(R.nparts), dim3(KH_CHUNK_THREADS), 0, t->stream, D));
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(t->hpin, res, sizeof(IpResult), hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipMemcpyAsync(t->hpin + 32, zpre, 64, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  const IpResult* h = reinterpret_cast<const IpResult*>(t->hpin);
  const uint64_t dnew = h->n_in, placed = h->done;
  t->lsize += placed;
  *n_new_out = placed;
  if (reinterpret_cast<const uint32_t*>(t->hpin + 32 + 4)[KH_FLAG_INTERNAL]) return fail(t, KH_ERR_HIP, kDedupOverflowText);
  if (placed != dnew || h->flags[KH_FLAG_PROBE_OVERFLOW])
    return fail(t, KH_ERR_PROBE_OVERFLOW, "Robin Hood probe distance would exceed 127 (7-bit info field, hashmap_robinhood.hpp:142-144,556); "
                                          "the keys of the batch that fit were applied in place");
  return KH_OK;
}

kh_status do_insert(kh_table* t, const void* keys, uint32_t kstride, const void* vals, uint32_t vstride, uint64_t n,
                    kh_mem where, int mode, uint64_t* n_inserted, bool tail_reserve = true) {
  if (n_inserted) *n_inserted = 0;
  if (n && !keys) return fail(t, KH_ERR_INVALID, "null keys");
  if (is_reduce(mode) && mode != INS_PLUS && !vals) return fail(t, KH_ERR_INVALID, "null values: only the std::plus reducer has a default value (1)");
  if (t->ins.active) return refuse_streaming(t);
  HIPCHK(hipSetDevice(t->device));
  { const uint64_t np_ = std::min<uint64_t>(n, g_max_pass);       // (pairs of one internal pass: insert_device)
    const uint64_t cu = capacity_after(t, t->cur.cap, t->lsize, np_ ? np_ : 1, np_, np_ ? np_ - 1 : 0);
    const bool ip = inplace_ok(t, n) && t->lsize + n <= t->max_load;      // in place: no re-layout workspace, bins instead
    kh_status ps = ip ? arena_prepare(t, (where == KH_MEM_HOST ? n * 16 : 0) + n * 48 + ws_inplace(t, n))
                      // (68 B per pair: two buffers of 16-byte records in histogram-free slots of up to twice the mean fill -- a duplicate-heavy batch,
                      //  insert_core -- + the sample set; a duplicate-free batch takes 28 B per pair of it, an exact partition 58)
                      : arena_prepare(t, (where == KH_MEM_HOST ? n * 16 : 0) + np_ * 68 + ws_rebuild(cu) + cu * 2 + (cu > KH_L ? (cu >> KH_LB) : 1) * 64 + (np_ / KH_PART_TILE + 4096) * 16 + (size_t(1) << 20));
    if (ps != KH_OK) return ps; }
  const char* kb = static_cast<const char*>(keys);
  const char* vb = static_cast<const char*>(vals);
  if (where == KH_MEM_HOST && n) {
    char* d = nullptr;
    if (kstride == 16) {           // pair array: one copy, values live at +8
      TAKE(d, char, n * 16);
      HIPCHK(hipMemcpyAsync(d, keys, n * 16, hipMemcpyHostToDevice, t->stream));
      kb = d; vb = d + 8;
    } else {
      TAKE(d, char, n * 8);
      HIPCHK(hipMemcpyAsync(d, keys, n * 8, hipMemcpyHostToDevice, t->stream));
      kb = d;
      if (vals) {
        char* dv = nullptr;
        TAKE(dv, char, n * 4);
        HIPCHK(hipMemcpyAsync(dv, vals, n * 4, hipMemcpyHostToDevice, t->stream));
        vb = dv;
      }
    }
  }
  uint64_t total_new = 0;
  kh_status st = KH_OK;
  // a handful of keys into a table with room for all of them (no insert() call of the batch can trigger the doubling):
  // applied in place, one after the other, by the reference's own single-key algorithms
  if (n > 0 && n <= KH_SMALL_N && t->lsize > 0 && t->lsize + n <= t->max_load && !g_disable_small) {
    uint64_t ch = 0; uint32_t done = 0;
    st = small_batch(t, kb, kstride, vb, vstride, mode == INS_PLUS ? 1u : 0u, (uint32_t)n,
                     mode == INS_UPDATE ? KH_SMALL_UPDATE : (is_reduce(mode) ? KH_SMALL_PLUS : KH_SMALL_FIRST), &ch, &done, reduce_op(mode));
    if (st != KH_OK) return st;
    t->lsize += ch;
    total_new = ch;
    kb += (uint64_t)done * kstride;
    if (vb) vb += (uint64_t)done * vstride;
    n -= done;                      // > 0 only when a displacement chain would pass distance 127: the general path reports it
  }
  if (n > 0 && inplace_ok(t, n) && t->lsize + n <= t->max_load) {
    uint64_t more = 0;
    st = insert_inplace(t, kb, kstride, vb, vstride, n, mode, &more);
    total_new += more;
    n = 0;
  }
  if (n > 0) {
    uint64_t more = 0;
    st = insert_device(t, kb, kstride, vb, vstride, n, mode, &more);
    total_new += more;
  }
  // trailing reserve(lsize) of insert(Iter,Iter) (:672 / :546): a no-op unless size > max_load (after set_max_load_factor).
  // kh_update stands for a sequence of update(k,v) calls (:1274), which has no such tail
  if (st == KH_OK && mode != INS_UPDATE && tail_reserve) st = do_reserve(t, t->lsize);
  if (st == KH_OK) HIPCHK(hipStreamSynchronize(t->stream));
  if (n_inserted) *n_inserted = total_new;
  return st;
}

// generic compaction: flags/q/vals (device) -> out (device), keys of the table's width; returns the number of hits
kh_status compact(kh_table* t, const uint8_t* flags, const uint64_t* q, const uint32_t* vals, uint64_t n,
                  uint64_t* out_keys, uint32_t* out_vals, uint64_t* n_out) {
  *n_out = 0;
  if (n == 0) return KH_OK;
  const uint64_t ntl = (n + KH_CMP_TILE - 1) / KH_CMP_TILE;
  uint32_t* sums; uint64_t* offs;
  TAKE(sums, uint32_t, ntl); TAKE(offs, uint64_t, ntl + 1);
  { Launch L(t, "k_flag_tile_sums");
    hipLaunchKernelGGL(k_flag_tile_sums, dim3((uint32_t)ntl), dim3(256), 0, t->stream, flags, n, sums); }
  { Launch L(t, "k_scan");
    hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, t->stream, sums, ntl, offs); }
  if (is_wide(t)) {
    Launch L(t, "kw_compact");
    hipLaunchKernelGGL(kw_compact, dim3((uint32_t)ntl), dim3(256), 0, t->stream, flags, q, vals, n, (const uint64_t*)offs, out_keys, out_vals);
  } else {
    Launch L(t, "k_compact_hits");
    hipLaunchKernelGGL(k_compact_hits, dim3((uint32_t)ntl), dim3(256), 0, t->stream, flags, q, vals, n, offs, out_keys, out_vals, (uint8_t*)nullptr);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t->hpin, offs + ntl, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  *n_out = t->hpin[0];
  return KH_OK;
}
// host epilogue of a per-query find: found flags and, for the hits only, values (values of misses stay untouched in the caller's buffer)
kh_status copy_hits_selective(kh_table* t, const uint32_t* dv, const uint8_t* df, uint64_t n, uint32_t* out_vals, uint8_t* out_found) {
  std::vector<uint32_t> hv(out_vals ? n : 0); std::vector<uint8_t> hf(n);
  if (out_vals) HIPCHK(hipMemcpyAsync(hv.data(), dv, n * 4, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipMemcpyAsync(hf.data(), df, n, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  for (uint64_t i = 0; i < n; ++i) { if (out_found) out_found[i] = hf[i]; if (hf[i] && out_vals) out_vals[i] = hv[i]; }
  return KH_OK;
}
// host epilogue of a compacted find / to_vector: the first m (key, value) pairs, keys of the table's width (null: not wanted)
kh_status copy_compacted(kh_table* t, uint64_t m, const uint64_t* ck, const uint32_t* cv, uint64_t* keys_host, uint32_t* vals_host) {
  if (m && keys_host) HIPCHK(hipMemcpyAsync(keys_host, ck, m * (t->slot_bytes / 2), hipMemcpyDeviceToHost, t->stream));
  if (m && vals_host) HIPCHK(hipMemcpyAsync(vals_host, cv, m * 4, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  return KH_OK;
}

// launches k_find<KIND, HASH, OUT> over n device-resident queries; *hits_dev (device, 8 B) receives the number of hits
kh_status launch_find(kh_table* t, int out_mode, const uint64_t* q, uint64_t n, uint32_t* dvals, uint8_t* dfound, uint64_t* dkeys, uint8_t* dpairs,
                      unsigned long long** hits_dev) {
  const uint64_t ntiles = (n + KH_Q_TILE - 1) / KH_Q_TILE;
  // control block: [0] hit count, [1] ticket, then one look-back granule per tile (compacted forms)
  unsigned long long* ctl;
  const size_t nctl = 2 + ((out_mode == KH_FIND_COMPACT || out_mode == KH_FIND_PAIRS) ? ntiles : 0);
  TAKE(ctl, unsigned long long, nctl);
  HIPCHK(hipMemsetAsync(ctl, 0, nctl * 8, t->stream));
  KhFindParams F;
  memset(&F, 0, sizeof(F));
  F.T = narrow(t->cur); F.q = q; F.n = n; F.seed = t->seed;
  F.out_vals = dvals; F.out_found = dfound; F.out_keys = dkeys; F.out_pairs16 = dpairs;
  F.n_found = (out_mode == KH_FIND_COUNT && !hits_dev) ? nullptr : ctl;      // count(Iter,Iter) returns no total
  F.ticket = reinterpret_cast<uint32_t*>(ctl + 1); F.tile_state = ctl + 2;
  const int ncu = cu_count(t);
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(ntiles, (uint64_t)ncu * 8));
  const char* name = out_mode == KH_FIND_COUNT ? "k_count" : "k_find";
  { Launch L(t, name);
#define KH_FIND_LAUNCH(OUT)                                                                                                            \
    if (t->seed.xk) { KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_find<KIND, HASH, OUT, true>), dim3(grid), dim3(KH_Q_THREADS), 0, t->stream, F)); }   \
    else { KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_find<KIND, HASH, OUT, false>), dim3(grid), dim3(KH_Q_THREADS), 0, t->stream, F)); }
    switch (out_mode) {
      case KH_FIND_PERQUERY: KH_FIND_LAUNCH(KH_FIND_PERQUERY) break;
      case KH_FIND_COMPACT: KH_FIND_LAUNCH(KH_FIND_COMPACT) break;
      case KH_FIND_PAIRS: KH_FIND_LAUNCH(KH_FIND_PAIRS) break;
      default: KH_FIND_LAUNCH(KH_FIND_COUNT) break;
    }
#undef KH_FIND_LAUNCH
  }
  HIPCHK(hipGetLastError());
  if (hits_dev) *hits_dev = ctl;
  return KH_OK;
}

kh_status do_find(kh_table* t, const void* keys, uint64_t n, kh_mem where, uint32_t* out_vals, uint8_t* out_found,
                  uint64_t* out_ckeys, uint32_t* out_cvals, void* out_pairs, bool compacted, uint64_t* n_found) {
  if (n_found) *n_found = 0;
  if (t->ins.active) return refuse_streaming(t);
  if (n == 0) return KH_OK;
  if (!keys) return fail(t, KH_ERR_INVALID, "null keys");
  HIPCHK(hipSetDevice(t->device));
  { kh_status ps = arena_prepare(t, n * 40 + (n / KH_Q_TILE + 8) * 8 + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  const uint64_t* q;
  kh_status st = stage_in<uint64_t>(t, keys, n, where, &q);
  if (st != KH_OK) return st;
  const bool host = where == KH_MEM_HOST;
  unsigned long long* hits_dev = nullptr;
  uint64_t hits = 0;
  if (!compacted) {
    uint32_t* dv = out_vals; uint8_t* df = out_found;
    if (host && dv) TAKE(dv, uint32_t, n);
    if (host || !df) TAKE(df, uint8_t, n);
    st = launch_find(t, KH_FIND_PERQUERY, q, n, dv, df, nullptr, nullptr, &hits_dev);
    if (st != KH_OK) return st;
    HIPCHK(hipMemcpyAsync(t->hpin, hits_dev, 8, hipMemcpyDeviceToHost, t->stream));
    if (host) { st = copy_hits_selective(t, dv, df, n, out_vals, out_found); if (st != KH_OK) return st; }
    else if (n_found) HIPCHK(hipStreamSynchronize(t->stream));
    hits = t->hpin[0];
  } else {
    uint64_t* ck = out_ckeys; uint32_t* cv = out_cvals; uint8_t* cp = static_cast<uint8_t*>(out_pairs);
    if (host) {
      if (out_pairs) TAKE(cp, uint8_t, n * 16);
      else { TAKE(ck, uint64_t, n); TAKE(cv, uint32_t, n); }
    }
    st = launch_find(t, out_pairs ? KH_FIND_PAIRS : KH_FIND_COMPACT, q, n, out_pairs ? nullptr : cv, nullptr, out_pairs ? nullptr : ck,
                     out_pairs ? cp : nullptr, &hits_dev);
    if (st != KH_OK) return st;
    HIPCHK(hipMemcpyAsync(t->hpin, hits_dev, 8, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    hits = t->hpin[0];
    if (host && hits) {
      if (out_pairs) { HIPCHK(hipMemcpyAsync(out_pairs, cp, hits * 16, hipMemcpyDeviceToHost, t->stream)); HIPCHK(hipStreamSynchronize(t->stream)); }
      else { st = copy_compacted(t, hits, ck, cv, out_ckeys, out_cvals); if (st != KH_OK) return st; }
    }
  }
  if (n_found) *n_found = hits;
  return KH_OK;
}

// erase_no_resize over a batch; the caller applies the form-specific resize rule
kh_status erase_core(kh_table* t, const void* keys, uint64_t n, kh_mem where, uint64_t* n_erased) {
  *n_erased = 0;
  if (t->ins.active) return refuse_streaming(t);
  if (n == 0) return KH_OK;
  if (!keys) return fail(t, KH_ERR_INVALID, "null keys");
  HIPCHK(hipSetDevice(t->device));
  { kh_status ps = inplace_ok(t, n) ? arena_prepare(t, n * 8 + ws_inplace(t, n))
                                    : arena_prepare(t, n * 8 + 2 * 8 * ((slack_slot((double)n / (double)std::max<uint64_t>(1, t->cur.cap >> KH_LB)) * std::max<uint64_t>(1, t->cur.cap >> KH_LB)) + KH_PART_TILE + n) +
                                                       ws_rebuild(t->cur.cap) + (t->cur.cap > KH_L ? (t->cur.cap >> KH_LB) : 1) * 96 + (n / KH_PART_TILE + 4096) * 16 + (size_t(2) << 20));
    if (ps != KH_OK) return ps; }
  const uint64_t* q;
  kh_status st = stage_in<uint64_t>(t, keys, n, where, &q);
  if (st != KH_OK) return st;
  if (t->kind == KHK_RH && n <= KH_SMALL_N && t->lsize > 0 && !g_disable_small) {      // backward-shift deletes in place
    uint64_t ne = 0; uint32_t done = 0;
    st = small_batch(t, reinterpret_cast<const char*>(q), 8, nullptr, 0, 0, (uint32_t)n, KH_SMALL_ERASE, &ne, &done);
    if (st != KH_OK) return st;
    t->lsize -= ne;
    *n_erased = ne;
    return KH_OK;
  }
  if (inplace_ok(t, n)) {       // backward-shift deletes in place, one lane per region of the table
    KhInplaceParams src;
    memset(&src, 0, sizeof(src));
    src.in_k = q; src.n = n;
    IpResult* res = nullptr;
    st = inplace_passes<KH_IP_ERASE>(t, src, n, &res);
    if (st != KH_OK) return st;
    HIPCHK(hipMemcpyAsync(t->hpin, &res->done, 8, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    t->lsize -= t->hpin[0];
    *n_erased = t->hpin[0];
    return KH_OK;
  }
  // ---- Robin Hood batch erase as streaming passes: the erase keys are partitioned by chunk like an insert batch (8-byte
  // records), and ONE launch re-lays the table out chunk by chunk, dropping every element whose key is among its chunk's erase keys (LDS
  // fold) -- no probe at random into HBM.  Speculative like the other one-launch forms: a chunk whose elements + erase keys exceed the
  // staging area, a carry chain or a poll time-out send the batch down the mark + re-layout path below.
  const uint32_t PBe = t->cur.cap > KH_L ? log2u(t->cur.cap >> KH_LB) : 0u;
  if (t->kind == KHK_RH && !g_disable_fused_rebuild && !getenv("KH_DISABLE_STREAM_ERASE") && t->cur.cap >= 2 * (uint64_t)KH_L && PBe <= 22 &&
      t->lsize > 0 && t->lsize <= threshold(t->cur.cap, 0.9f) && n <= 0xFFFFFFF0ull) {
    const size_t keep_blk = t->blk, keep_off = t->off;
    // hashed erase keys fill the chunks evenly: histogram-free partition into fixed slots (two passes for more than 2^11 chunks); a
    // slot that overflows (keys given many times over) is caught by the flag and the mark path takes the batch
    const bool slack = PBe > 11 && !g_disable_slack;
    const uint64_t mrec = slack ? (slack_slot((double)n / (double)(uint64_t(1) << PBe)) << PBe) + KH_PART_TILE : n;
    char *a, *b;
    TAKE(a, char, mrec * sizeof(KhRec8)); TAKE(b, char, mrec * sizeof(KhRec8));
    Partitioned R;
    st = partition_batch(t, reinterpret_cast<const char*>(q), 8, nullptr, 0, 0u, n, 0, PBe, reinterpret_cast<ulonglong2*>(a), reinterpret_cast<ulonglong2*>(b), R, slack, 2, nullptr, slack);
    if (st != KH_OK) return st;
    t->part_overflow = R.overflow;
    KhSlots nw;
    st = fresh_slots(t, t->cur.cap, nw);
    if (st != KH_OK) return st;
    KhFusedParams F;
    memset(&F, 0, sizeof(F));
    F.src.rec[0] = R.rec; F.src.off[0] = R.part_off; F.src.n = 1; F.src.merged_off = R.part_off; F.src.slot[0] = R.slot; F.src.cur[0] = R.cursor; F.src.rec12 = 2;
    F.PB = PBe; F.mode = KH_DEDUP_ERASE;
    F.R.Old = narrow(t->cur); F.R.PB = PBe;
    FusedRun run;
    // (erase keys of a chunk fit one per lane -- a histogram-free partition's slot, or the mean of an exact one leaves room: the ordered-stream
    //  kernel, four workgroups per CU; else the staging form)
    const bool ordered = (R.slot != 0 ? R.slot <= KH_ES_MAXK : n / (uint64_t(1) << PBe) <= KH_ES_MAXK / 2) && !getenv("KH_DISABLE_ORDERED_ERASE");
    { kh_status fs = launch_fused(t, ordered ? 4 : 3, F, nw, PBe, "k_erase_fused", &run); t->part_overflow = nullptr; if (fs != KH_OK) return fs; }
    const uint32_t* ff = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(t->hpin) + 64);
    bool bad = R.overflow && (uint32_t)t->hpin[30];
    for (int i = 0; i < KH_NFLAGS; ++i) bad = bad || ff[i] != 0;
    const uint64_t placed = t->hpin[0];
    if (!bad && placed <= t->lsize) {
      adopt_slots(t, nw);
      *n_erased = t->lsize - placed;
      t->lsize = placed;
      return KH_OK;
    }
    if (getenv("KH_DEBUG_FUSED"))
      fprintf(stderr, "[kmerhash_amd] fused erase rejected: placed %llu size %llu flags=%u %u %u %u %u\n", (unsigned long long)placed, (unsigned long long)t->lsize, ff[0], ff[1], ff[2], ff[3], ff[4]);
    retire_slots(t, nw);
    t->blk = keep_blk; t->off = keep_off;
  }
  unsigned long long* cnt;
  TAKE(cnt, unsigned long long, 1);
  HIPCHK(hipMemsetAsync(cnt, 0, 8, t->stream));
  { Launch L(t, "k_erase_mark");
    KH_SWITCH_KIND_HASH(t->kind, t->hash, hipLaunchKernelGGL((k_erase_mark<KIND, HASH>), dim3(grid_for(n, KH_Q_THREADS * KH_Q_ITEMS, 2048)), dim3(KH_Q_THREADS), 0, t->stream, narrow(t->cur), q, n, t->seed, cnt)); }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t->hpin, cnt, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  const uint64_t ne = t->hpin[0];
  if (ne && t->kind == KHK_RH) {
    st = rebuild(t, t->cur.cap, nullptr, nullptr, nullptr, nullptr, 0, true, t->lsize - ne);
    if (st != KH_OK) {        // the table keeps its elements: take the marks back
      hipLaunchKernelGGL(k_clear_marks, dim3(grid_for(t->cur.cap, 256)), dim3(256), 0, t->stream, narrow(t->cur));
      hipStreamSynchronize(t->stream);
      return st;
    }
  }
  t->lsize -= ne;
  *n_erased = ne;
  return KH_OK;
}

bool valid(const kh_table* t) { return t != nullptr; }
// the one place a table's state is set up: the first slot buffer (slot_bytes is set), pinned scratch, thresholds; the caller has
// checked its arguments and made `device` current.  On an error nothing is left allocated.
kh_status table_init(kh_table* t, int kind, int hash, uint64_t seed, uint64_t capacity, float min_lf, float max_lf, int device) {
  t->kind = kind; t->hash = hash; t->device = device; t->seed = KhSeed{seed, 0u};
  t->min_lf = min_lf; t->max_lf = max_lf;
  const uint64_t cap = next_pow2(capacity);
  if (alloc_slots(t, cap, t->cur) != KH_OK) return KH_ERR_NOMEM;
  t->hpin = pinned_get();
  if (!t->hpin) { free_slots(t, t->cur); return KH_ERR_NOMEM; }
  if (fill_empty(t, t->cur) != KH_OK || hipStreamSynchronize(t->stream) != hipSuccess) { free_slots(t, t->cur); pinned_put(t->hpin); return KH_ERR_HIP; }
  t->min_load = threshold(cap, min_lf);
  t->max_load = threshold(cap, max_lf);
  return KH_OK;
}
void table_release(kh_table* t) {
  if (!t) return;
  hipSetDevice(t->device);
  hipStreamSynchronize(t->stream);
  for (auto& r : t->recs) { event_put(t->device, r.a); event_put(t->device, r.b); }
  free_slots(t, t->cur); free_slots(t, t->spare);
  for (auto& b : t->blocks) pool_free(t->device, b.p);
  pinned_put(t->hpin);
}

}  // namespace

// ===================================================================================================
// C ABI
// ===================================================================================================
extern "C" {

const char* kh_version(void) { return KH_VERSION_STR; }

kh_status kh_release_cached_memory(int device) {
  if (device < 0 || device >= 16) return KH_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess) return KH_ERR_HIP;
  hipDeviceSynchronize();
  pool_trim(device);
  return KH_OK;
}

kh_status kh_create(kh_table** out, kh_kind kind, uint32_t key_bytes, uint32_t val_bytes, kh_hash hash, uint64_t seed,
                    uint64_t capacity, float min_lf, float max_lf, int device) {
  if (!out) return KH_ERR_INVALID;
  *out = nullptr;
  if (key_bytes != 8 || val_bytes != 4) return KH_ERR_UNSUPPORTED;
  if ((int)kind < 0 || (int)kind > 1 || (int)hash < 0 || (int)hash > 3) return KH_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return KH_ERR_HIP;   // fail loudly: no CPU fallback exists
  if (device < 0 || device >= ndev) return KH_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess) return KH_ERR_HIP;
  kh_table* t = new kh_table();
  const kh_status st = table_init(t, (int)kind, (int)hash, seed, capacity, min_lf, max_lf, device);
  if (st != KH_OK) { delete t; return st; }
  *out = t;
  return KH_OK;
}

kh_status kh_destroy(kh_table* t) { table_release(t); delete t; return KH_OK; }

kh_status kh_set_stream(kh_table* t, void* s) {
  if (!valid(t)) return KH_ERR_INVALID;
  if (t->stream == static_cast<hipStream_t>(s)) return KH_OK;     // unchanged: nothing to order
  hipSetDevice(t->device);
  hipStreamSynchronize(t->stream);                                   // work already issued stays ordered before the new stream's
  t->stream = static_cast<hipStream_t>(s);
  return KH_OK;
}
const char* kh_last_error(const kh_table* t) { return t ? t->err.c_str() : "null table"; }

kh_status kh_size(const kh_table* t, uint64_t* out) { if (!t || !out) return KH_ERR_INVALID; *out = t->lsize; return KH_OK; }
kh_status kh_capacity(const kh_table* t, uint64_t* out) { if (!t || !out) return KH_ERR_INVALID; *out = t->cur.cap; return KH_OK; }
kh_status kh_get_load_thresholds(const kh_table* t, uint64_t* mn, uint64_t* mx) {
  if (!t) return KH_ERR_INVALID;
  if (mn) *mn = t->min_load;
  if (mx) *mx = t->max_load;
  return KH_OK;
}
kh_status kh_set_min_load_factor(kh_table* t, float f) { if (!t) return KH_ERR_INVALID; t->min_lf = f; t->min_load = threshold(t->cur.cap, f); return KH_OK; }
kh_status kh_set_max_load_factor(kh_table* t, float f) { if (!t) return KH_ERR_INVALID; t->max_lf = f; t->max_load = threshold(t->cur.cap, f); return KH_OK; }
kh_status kh_get_load_factors(const kh_table* t, float* mn, float* mx, float* cur) {
  if (!t) return KH_ERR_INVALID;
  if (mn) *mn = t->min_lf;
  if (mx) *mx = t->max_lf;
  if (cur) *cur = static_cast<float>(t->lsize) / static_cast<float>(t->cur.cap);
  return KH_OK;
}
kh_status kh_clear(kh_table* t) {
  if (!t) return KH_ERR_INVALID;
  if (t->ins.active) return refuse_streaming(t);
  HIPCHK(hipSetDevice(t->device));
  t->lsize = 0;
  { kh_status fs = fill_empty(t, t->cur); if (fs != KH_OK) return fs; }
  HIPCHK(hipStreamSynchronize(t->stream));
  return KH_OK;
}
kh_status kh_reserve(kh_table* t, uint64_t n) { if (!t) return KH_ERR_INVALID; HIPCHK(hipSetDevice(t->device)); return do_reserve(t, n); }
kh_status kh_rehash(kh_table* t, uint64_t b) { if (!t) return KH_ERR_INVALID; HIPCHK(hipSetDevice(t->device)); return do_rehash(t, b); }

kh_status kh_insert(kh_table* t, const void* keys, const void* vals, uint64_t n, kh_mem where, uint64_t* n_inserted) {
  if (!t) return KH_ERR_INVALID;
  return do_insert(t, keys, 8, vals, 4, n, where, INS_FIRST, n_inserted);
}
kh_status kh_insert_pairs(kh_table* t, const void* pairs16, uint64_t n, kh_mem where, uint64_t* n_inserted) {
  if (!t) return KH_ERR_INVALID;
  return do_insert(t, pairs16, 16, pairs16 ? static_cast<const char*>(pairs16) + 8 : nullptr, 16, n, where, INS_FIRST, n_inserted);
}
kh_status kh_insert_one(kh_table* t, uint64_t key, uint32_t val, uint64_t* n_inserted) {
  if (!t) return KH_ERR_INVALID;
  return do_insert(t, &key, 8, &val, 4, 1, KH_MEM_HOST, INS_FIRST, n_inserted, false);
}
kh_status kh_update(kh_table* t, const void* keys, const void* vals, uint64_t n, kh_mem where, uint64_t* n_inserted) {
  if (!t) return KH_ERR_INVALID;
  return do_insert(t, keys, 8, vals, 4, n, where, INS_UPDATE, n_inserted);
}
// ---- streamed insert: ONE insert(Iter,Iter) whose input arrives in pieces (the multi-GPU exchange feeds the pieces as
//      they land; every feed is radix-partitioned right away, asynchronously, so that work overlaps the next transfer)
kh_status kh_insert_begin(kh_table* t, uint64_t n_total, int reduce_plus) {
  return kh_insert_begin_ex(t, n_total, reduce_plus ? KH_INS_REDUCE_PLUS : 0u);
}
kh_status kh_insert_begin_ex(kh_table* t, uint64_t n_total, unsigned flags) {
  if (!t) return KH_ERR_INVALID;
  if (t->ins.active) return fail(t, KH_ERR_INVALID, "a streamed insert is already in progress");
  if (!ins_flags_ok(flags)) return fail(t, KH_ERR_INVALID, "unknown flag");
  HIPCHK(hipSetDevice(t->device));
  memset(&t->ins, 0, sizeof(t->ins));
  t->ins.mode = ins_flags_mode(flags);
  t->ins.repeatable = (flags & KH_INS_REPEATABLE) != 0 && !g_disable_slack;
  t->ins.n_total = n_total;
  const uint64_t cu = capacity_after(t, t->cur.cap, t->lsize, n_total ? n_total : 1, n_total, n_total ? n_total - 1 : 0);
  { kh_status ps = arena_prepare(t, n_total * ((flags & KH_INS_REPEATABLE) ? 72 : 56) + ws_rebuild(cu) + cu * 2 + (cu > KH_L ? (cu >> KH_LB) : 1) * 64 * (KH_MAX_SRC + 1) +
                                    (n_total / KH_PART_TILE + 4096 * KH_MAX_SRC) * 16 + (size_t(8) << 20));
    if (ps != KH_OK) return ps; }
  const uint32_t PB = cu > KH_L ? log2u(cu >> KH_LB) : 0u;
  // the one-shot rule evaluation needs at most one pending doubling and 32-bit stream positions; otherwise the pieces are
  // only collected and inserted by the general entry point at the end
  t->ins.fallback = n_total == 0 || n_total > 0xFFFFFFF0ull || PB > 22 || t->lsize >= threshold(t->cur.cap << 1, t->max_lf);
  t->ins.cap_u = cu; t->ins.PB = PB;
  if (n_total) {
    if (t->ins.fallback) { TAKE(t->ins.stage_k, uint64_t, n_total); TAKE(t->ins.stage_v, uint32_t, n_total); }
    else if (!t->ins.repeatable) { TAKE(t->ins.tmp, ulonglong2, n_total); TAKE(t->ins.fin, ulonglong2, n_total); }
    // (repeatable: the first feed's sample decides the layout, the buffers are taken there)
  }
  t->ins.active = true;
  return KH_OK;
}

kh_status kh_insert_feed(kh_table* t, const void* keys, const void* vals, uint64_t n, kh_mem where) {
  if (!t) return KH_ERR_INVALID;
  if (!t->ins.active) return fail(t, KH_ERR_INVALID, "kh_insert_feed without kh_insert_begin");
  if (n == 0) return KH_OK;
  if (!keys) return fail(t, KH_ERR_INVALID, "null keys");
  if (!vals && is_reduce(t->ins.mode) && t->ins.mode != INS_PLUS) return fail(t, KH_ERR_INVALID, "null values: only the std::plus reducer has a default value (1)");
  if (t->ins.fed + n > t->ins.n_total) return fail(t, KH_ERR_INVALID, "more pairs fed than announced to kh_insert_begin");
  HIPCHK(hipSetDevice(t->device));
  const uint64_t* dk; const uint32_t* dv;
  kh_status st = stage_in<uint64_t>(t, keys, n, where, &dk);
  if (st == KH_OK) st = stage_in<uint32_t>(t, vals, n, where, &dv);
  if (st != KH_OK) return st;
  if (t->ins.fallback) {
    HIPCHK(hipMemcpyAsync(t->ins.stage_k + t->ins.fed, dk, n * 8, hipMemcpyDeviceToDevice, t->stream));
    if (dv) HIPCHK(hipMemcpyAsync(t->ins.stage_v + t->ins.fed, dv, n * 4, hipMemcpyDeviceToDevice, t->stream));
    else HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(t->ins.stage_v + t->ins.fed), t->ins.mode == INS_PLUS ? 1 : 0, n, t->stream));
  } else {
    if (t->ins.S.n == KH_MAX_SRC) return fail(t, KH_ERR_UNSUPPORTED, "more than 16 feeds in one streamed insert");
    if (t->ins.S.n == 0 && n >= KH_SAMPLE_N) {
      // the first piece speaks for the batch: no duplicate among 65536 of its keys -> the one-launch build runs without its
      // LDS fold and CHECKS instead (a duplicate met after all sends the batch down the general path, nothing is lost).  One
      // host synchronisation per streamed insert, before anything else is in flight on this stream.
      unsigned long long* sset; uint32_t* dups;
      TAKE(sset, unsigned long long, KH_SAMPLE_SET); TAKE(dups, uint32_t, 1);
      HIPCHK(hipMemsetAsync(sset, 0, sizeof(unsigned long long) * KH_SAMPLE_SET, t->stream));
      HIPCHK(hipMemsetAsync(dups, 0, 4, t->stream));
      { Launch L(t, "k_sample_dups");
        hipLaunchKernelGGL(k_sample_dups, dim3(KH_SAMPLE_N / 256), dim3(256), 0, t->stream, reinterpret_cast<const char*>(dk), 8u, n, sset, dups, KhCursorInit{}); }
      HIPCHK(hipMemcpyAsync(t->hpin + 31, dups, 4, hipMemcpyDeviceToHost, t->stream));
      HIPCHK(hipStreamSynchronize(t->stream));
      t->ins.nodup = (uint32_t)t->hpin[31] == 0u;
      // a repeatable insert of (nearly) duplicate-free pieces: histogram-free partition into slots all pieces share
      t->ins.slack = t->ins.repeatable && (uint32_t)t->hpin[31] == 0u && part_buffer_records(t->ins.n_total, t->ins.PB, true) != t->ins.n_total;
    }
    if (t->ins.S.n == 0 && t->ins.repeatable) {       // buffers of the chosen layout
      const uint64_t nt = t->ins.n_total;
      if (t->ins.slack) {
        const uint32_t nparts = 1u << t->ins.PB;
        t->batch_nodup = t->ins.nodup;
        t->ins.rec12 = nodup_build_applies(t, t->ins.cap_u, t->ins.PB, t->ins.mode);
        t->batch_nodup = false;
        SlackShared& sh = t->ins.sh;
        sh.slot = slack_slot((double)nt / (double)nparts);
        char* f; TAKE(f, char, (sh.slot * nparts + KH_PART_TILE) * (t->ins.rec12 ? sizeof(KhRec12) : sizeof(ulonglong2)));
        t->ins.fin = reinterpret_cast<ulonglong2*>(f);
        TAKE(sh.cur2, unsigned long long, nparts); TAKE(sh.starts, uint64_t, (size_t)nparts + 1); TAKE(sh.ovf, uint32_t, 1);
        HIPCHK(hipMemsetAsync(sh.ovf, 0, 4, t->stream));
        hipLaunchKernelGGL(k_init_cursors, dim3((nparts + 256) / 256), dim3(256), 0, t->stream, sh.cur2, sh.starts, (uint64_t)nparts, sh.slot);
      } else { TAKE(t->ins.tmp, ulonglong2, nt); TAKE(t->ins.fin, ulonglong2, nt); }
    }
    Partitioned R;
    if (t->ins.slack) {
      // this piece's level-1 buckets (its own slots), then its records into the shared final slots
      const uint32_t B1 = (t->ins.PB + 1) / 2, nb1 = 1u << B1;
      const uint64_t slot1 = slack_slot((double)n / (double)nb1);
      char* tm; TAKE(tm, char, (slot1 * nb1 + KH_PART_TILE) * (t->ins.rec12 ? sizeof(KhRec12) : sizeof(ulonglong2)));
      st = partition_batch(t, reinterpret_cast<const char*>(dk), 8, reinterpret_cast<const char*>(dv), 4, t->ins.mode == INS_PLUS ? 1u : 0u,
                           n, t->ins.fed, t->ins.PB, reinterpret_cast<ulonglong2*>(tm), t->ins.fin, R, true, t->ins.rec12, &t->ins.sh);
      if (st != KH_OK) return st;
      t->ins.S.n = 1;      // one source whatever the number of pieces
    } else {
      st = partition_batch(t, reinterpret_cast<const char*>(dk), 8, reinterpret_cast<const char*>(dv), 4, t->ins.mode == INS_PLUS ? 1u : 0u,
                           n, t->ins.fed, t->ins.PB, t->ins.tmp, t->ins.fin + t->ins.fed, R);
      if (st != KH_OK) return st;
      t->ins.S.rec[t->ins.S.n] = R.rec; t->ins.S.off[t->ins.S.n] = R.part_off; ++t->ins.S.n;
    }
  }
  t->ins.fed += n;
  if (where == KH_MEM_HOST) HIPCHK(hipStreamSynchronize(t->stream));   // host buffers may be reused as soon as the feed returns
  return KH_OK;
}

kh_status kh_insert_end(kh_table* t, uint64_t* n_inserted) {
  if (n_inserted) *n_inserted = 0;
  if (!t) return KH_ERR_INVALID;
  if (!t->ins.active) return fail(t, KH_ERR_INVALID, "kh_insert_end without kh_insert_begin");
  t->ins.active = false;
  if (t->ins.fed != t->ins.n_total) return fail(t, KH_ERR_INVALID, "fewer pairs fed than announced to kh_insert_begin");
  HIPCHK(hipSetDevice(t->device));
  uint64_t nn = 0;
  kh_status st = KH_OK;
  const uint64_t n = t->ins.n_total;
  if (n) {
    if (t->ins.fallback) {
      st = insert_device(t, reinterpret_cast<const char*>(t->ins.stage_k), 8, reinterpret_cast<const char*>(t->ins.stage_v), 4, n, t->ins.mode, &nn);
    } else if (t->ins.slack) {
      const uint32_t nparts = 1u << t->ins.PB;
      const uint64_t list_cap = t->ins.sh.slot * nparts + KH_PART_TILE;
      KhSrcSet S;
      memset(&S, 0, sizeof(S));
      S.rec[0] = t->ins.fin; S.off[0] = t->ins.sh.starts; S.n = 1; S.merged_off = t->ins.sh.starts;
      S.slot[0] = t->ins.sh.slot; S.cur[0] = t->ins.sh.cur2; S.rec12 = t->ins.rec12 ? 1u : 0u;
      char* spare; TAKE(spare, char, list_cap * 16);
      t->part_overflow = t->ins.sh.ovf; t->batch_nodup = t->ins.nodup;
      st = insert_finish(t, S, n, t->ins.PB, t->ins.cap_u, t->ins.mode, 0, reinterpret_cast<ulonglong2*>(spare), &nn, list_cap);
      t->part_overflow = nullptr; t->batch_nodup = false;
      if (st == KH_RETRY_EXACT) {      // a slot overflowed / a duplicate met without stream positions: nothing was inserted
        if (n_inserted) *n_inserted = 0;
        HIPCHK(hipStreamSynchronize(t->stream));
        t->err = "the speculative partition of this repeatable streamed insert did not hold: feed the same pieces again (kh_insert_begin without KH_INS_REPEATABLE)";
        return KH_ERR_RETRY;
      }
    } else {
      KhSrcSet S = t->ins.S;
      if (S.n == 1) S.merged_off = S.off[0];
      else {
        uint64_t* mo;
        const uint64_t nq1 = (uint64_t(1) << t->ins.PB) + 1;
        TAKE(mo, uint64_t, nq1);
        hipLaunchKernelGGL(k_merge_offsets, dim3((uint32_t)((nq1 + 255) / 256)), dim3(256), 0, t->stream, S, nq1, mo);
        S.merged_off = mo;
      }
      t->batch_nodup = t->ins.nodup;
      st = insert_finish(t, S, n, t->ins.PB, t->ins.cap_u, t->ins.mode, 0, t->ins.tmp, &nn);
      t->batch_nodup = false;
    }
  }
  if (st == KH_OK) st = do_reserve(t, t->lsize);
  if (st == KH_OK) HIPCHK(hipStreamSynchronize(t->stream));
  if (n_inserted) *n_inserted = nn;
  return st;
}

kh_status kh_insert_abort(kh_table* t) {
  if (!t) return KH_ERR_INVALID;
  if (!t->ins.active) return KH_OK;
  // the feeds only wrote workspace (partition records); the table itself has not been touched.  Kernels queued by the feeds may
  // still read the caller's device buffers: wait for them, like kh_insert_end would have
  hipSetDevice(t->device);
  hipError_t e = hipStreamSynchronize(t->stream);
  t->ins.active = false;
  t->part_overflow = nullptr; t->batch_nodup = false;
  if (e != hipSuccess) return fail(t, KH_ERR_HIP, std::string("kh_insert_abort: ") + hipGetErrorString(e));
  return KH_OK;
}

kh_status kh_insert_reduce_plus(kh_table* t, const void* keys, const void* vals, uint64_t n, kh_mem where, uint64_t* n_inserted) {
  if (!t) return KH_ERR_INVALID;
  return do_insert(t, keys, 8, vals, 4, n, where, INS_PLUS, n_inserted);
}
kh_status kh_insert_reduce(kh_table* t, const void* keys, const void* vals, uint64_t n, kh_mem where, kh_reduce_op op, uint64_t* n_inserted) {
  if (!t) return KH_ERR_INVALID;
  if (n_inserted) *n_inserted = 0;
  if ((unsigned)op > (unsigned)KH_REDUCE_OR) return fail(t, KH_ERR_INVALID, "unknown reduce operation");
  return do_insert(t, keys, 8, vals, 4, n, where, INS_PLUS + (int)op, n_inserted);
}

kh_status kh_count(kh_table* t, const void* keys, uint64_t n, kh_mem where, uint8_t* out01) {
  if (!t) return KH_ERR_INVALID;
  if (t->ins.active) return refuse_streaming(t);
  if (n == 0) return KH_OK;
  if (!keys || !out01) return fail(t, KH_ERR_INVALID, "null argument");
  HIPCHK(hipSetDevice(t->device));
  { kh_status ps = arena_prepare(t, n * 9 + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  const uint64_t* q;
  kh_status st = stage_in<uint64_t>(t, keys, n, where, &q);
  if (st != KH_OK) return st;
  uint8_t* d = out01;
  if (where == KH_MEM_HOST) TAKE(d, uint8_t, n);
  st = launch_find(t, KH_FIND_COUNT, q, n, nullptr, d, nullptr, nullptr, nullptr);
  if (st != KH_OK) return st;
  if (where == KH_MEM_HOST) {
    HIPCHK(hipMemcpyAsync(out01, d, n, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
  }
  return KH_OK;
}

kh_status kh_find(kh_table* t, const void* keys, uint64_t n, kh_mem where, uint32_t* out_vals, uint8_t* out_found, uint64_t* n_found) {
  if (!t) return KH_ERR_INVALID;
  return do_find(t, keys, n, where, out_vals, out_found, nullptr, nullptr, nullptr, false, n_found);
}
kh_status kh_find_compact(kh_table* t, const void* keys, uint64_t n, kh_mem where, uint64_t* out_keys, uint32_t* out_vals, uint64_t* n_found) {
  if (!t) return KH_ERR_INVALID;
  if (n && (!out_keys || !out_vals)) return fail(t, KH_ERR_INVALID, "null output");
  return do_find(t, keys, n, where, nullptr, nullptr, out_keys, out_vals, nullptr, true, n_found);
}
kh_status kh_find_compact_pairs(kh_table* t, const void* keys, uint64_t n, kh_mem where, void* out_pairs16, uint64_t* n_found) {
  if (!t) return KH_ERR_INVALID;
  if (n && !out_pairs16) return fail(t, KH_ERR_INVALID, "null output");
  return do_find(t, keys, n, where, nullptr, nullptr, nullptr, nullptr, out_pairs16, true, n_found);
}

kh_status kh_erase(kh_table* t, const void* keys, uint64_t n, kh_mem where, uint64_t* n_erased) {
  if (!t) return KH_ERR_INVALID;
  uint64_t ne = 0;
  kh_status st = erase_core(t, keys, n, where, &ne);
  if (n_erased) *n_erased = ne;
  if (st != KH_OK) return st;
  if (t->lsize < t->min_load) {
    if (t->kind == KHK_RH) st = do_reserve(t, t->lsize);   // hashmap_robinhood.hpp:1437: reserve() only grows
    else st = do_rehash(t, static_cast<uint64_t>(static_cast<float>(t->lsize) / t->max_lf));   // hashmap_linearprobe.hpp:1048
  }
  return st;
}
kh_status kh_erase_one(kh_table* t, uint64_t key, uint64_t* n_erased) {
  if (!t) return KH_ERR_INVALID;
  uint64_t ne = 0;
  kh_status st = erase_core(t, &key, 1, KH_MEM_HOST, &ne);
  if (n_erased) *n_erased = ne;
  if (st == KH_OK && t->lsize < t->min_load) st = do_rehash(t, t->cur.cap >> 1);   // :1425 / :1036
  return st;
}

}  // extern "C"
namespace {
// SoA view of the current table in the workspace (any of keys / vals / info / flags may be null; a wide table: two words per key)
kh_status unpack(kh_table* t, uint64_t* k, uint32_t* v, uint8_t* info, uint8_t* flags) {
  const uint64_t cap = t->cur.cap;
  Launch L(t, "k_unpack_slots");
  if (is_wide(t)) hipLaunchKernelGGL(kw_unpack_slots, dim3(grid_for(cap, 256)), dim3(256), 0, t->stream, (const KwSlot*)wide(t->cur).s, cap, k, v, info, flags);
  else if (t->kind == KHK_RH) hipLaunchKernelGGL((k_unpack_slots<KHK_RH>), dim3(grid_for(cap, 256)), dim3(256), 0, t->stream, narrow(t->cur).s, cap, k, v, info, flags);
  else hipLaunchKernelGGL((k_unpack_slots<KHK_LP>), dim3(grid_for(cap, 256)), dim3(256), 0, t->stream, narrow(t->cur).s, cap, k, v, info, flags);
  HIPCHK(hipGetLastError());
  return KH_OK;
}
}  // namespace
extern "C" {
kh_status kh_to_vector(kh_table* t, uint64_t* keys_host, uint32_t* vals_host, uint64_t* n_out) {
  if (!t) return KH_ERR_INVALID;
  if (t->ins.active) return refuse_streaming(t);
  HIPCHK(hipSetDevice(t->device));
  const uint64_t cap = t->cur.cap, kw = t->slot_bytes / sizeof(KhSlot);      // words per key
  { kh_status ps = arena_prepare(t, cap * (10 + 16 * kw) + cap / KH_CMP_TILE * 12 + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  uint8_t* flags; uint64_t *sk, *ck; uint32_t *sv, *cv;
  TAKE(flags, uint8_t, cap); TAKE(sk, uint64_t, kw * cap); TAKE(sv, uint32_t, cap); TAKE(ck, uint64_t, kw * cap); TAKE(cv, uint32_t, cap);
  kh_status st = unpack(t, sk, sv, nullptr, flags);
  if (st != KH_OK) return st;
  uint64_t m = 0;
  st = compact(t, flags, sk, sv, cap, ck, cv, &m);
  if (st != KH_OK) return st;
  st = copy_compacted(t, m, ck, cv, keys_host, vals_host);
  if (st != KH_OK) return st;
  if (n_out) *n_out = m;
  return KH_OK;
}
kh_status kh_export_info(kh_table* t, uint8_t* out_host) {
  if (!t || !out_host) return KH_ERR_INVALID;
  if (t->ins.active) return refuse_streaming(t);
  HIPCHK(hipSetDevice(t->device));
  { kh_status ps = arena_prepare(t, t->cur.cap + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  uint8_t* info;
  TAKE(info, uint8_t, t->cur.cap);
  kh_status st = unpack(t, nullptr, nullptr, info, nullptr);
  if (st != KH_OK) return st;
  HIPCHK(hipMemcpyAsync(out_host, info, t->cur.cap, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  return KH_OK;
}
kh_status kh_export_slots(kh_table* t, uint64_t* keys_host, uint32_t* vals_host) {
  if (!t) return KH_ERR_INVALID;
  if (t->ins.active) return refuse_streaming(t);
  HIPCHK(hipSetDevice(t->device));
  { kh_status ps = arena_prepare(t, t->cur.cap * 12 + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  uint64_t* sk; uint32_t* sv;
  TAKE(sk, uint64_t, t->cur.cap); TAKE(sv, uint32_t, t->cur.cap);
  kh_status st = unpack(t, sk, sv, nullptr, nullptr);
  if (st != KH_OK) return st;
  if (keys_host) HIPCHK(hipMemcpyAsync(keys_host, sk, t->cur.cap * 8, hipMemcpyDeviceToHost, t->stream));
  if (vals_host) HIPCHK(hipMemcpyAsync(vals_host, sv, t->cur.cap * 4, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  return KH_OK;
}
kh_status kh_export_raw_slots(kh_table* t, void* out_host) {
  if (!t || !out_host) return KH_ERR_INVALID;
  if (t->ins.active) return refuse_streaming(t);
  HIPCHK(hipSetDevice(t->device));
  HIPCHK(hipMemcpyAsync(out_host, narrow(t->cur).s, t->cur.cap * sizeof(KhSlot), hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  return KH_OK;
}
kh_status kh_displacement_histogram(kh_table* t, uint64_t out[128]) {
  if (!t || !out) return KH_ERR_INVALID;
  for (int i = 0; i < 128; ++i) out[i] = 0;
  if (t->kind != KHK_RH) return KH_OK;
  if (t->ins.active) return refuse_streaming(t);
  HIPCHK(hipSetDevice(t->device));
  { kh_status ps = arena_prepare(t, size_t(1) << 20); if (ps != KH_OK) return ps; }
  unsigned long long* d;
  TAKE(d, unsigned long long, 128);
  HIPCHK(hipMemsetAsync(d, 0, 128 * 8, t->stream));
  { Launch L(t, "k_disp_hist");
    if (is_wide(t)) hipLaunchKernelGGL(kw_disp_hist, dim3(grid_for(t->cur.cap, 256, 1024)), dim3(256), 0, t->stream, (const KwSlot*)wide(t->cur).s, t->cur.cap, d);
    else hipLaunchKernelGGL(k_disp_hist, dim3(grid_for(t->cur.cap, 256, 1024)), dim3(256), 0, t->stream, narrow(t->cur).s, t->cur.cap, d); }
  HIPCHK(hipMemcpyAsync(out, d, 128 * 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  return KH_OK;
}

}  // extern "C"

// ===================================================================================================
// value-range operations: the predicate lo <= value <= hi over the stored elements (the output predicate the reference's batched maps
// take on count / find / erase, robinhood_offset_hashmap_ptr.hpp:1337-1407, fixed to a closed range on the value so that it crosses a
// C ABI).  One code path for the three tables: the kernels are instantiated per slot layout.
// ===================================================================================================
namespace {
#define KV_SWITCH_LAYOUT(t, ...)                                                       \
  if (is_wide(t)) { constexpr int LAY = KV_WIDE; __VA_ARGS__; }                        \
  else if ((t)->kind == KHK_RH) { constexpr int LAY = KV_RH; __VA_ARGS__; }            \
  else { constexpr int LAY = KV_LP; __VA_ARGS__; }

}  // namespace
extern "C" {
kh_status kh_value_histogram(kh_table* t, uint32_t nbins, uint64_t* out_host) {
  if (!t) return KH_ERR_INVALID;
  if (t->ins.active) return refuse_streaming(t);
  if (nbins < 1 || nbins > KV_MAX_BINS) return fail(t, KH_ERR_INVALID, "kh_value_histogram: nbins must be 1..16384");
  if (!out_host) return fail(t, KH_ERR_INVALID, "null output");
  HIPCHK(hipSetDevice(t->device));
  memset(out_host, 0, sizeof(uint64_t) * nbins);
  if (t->lsize == 0) { HIPCHK(hipStreamSynchronize(t->stream)); return KH_OK; }
  { kh_status ps = arena_prepare(t, size_t(nbins) * 8 + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  unsigned long long* d;
  TAKE(d, unsigned long long, nbins);
  HIPCHK(hipMemsetAsync(d, 0, size_t(nbins) * 8, t->stream));
  const uint64_t cap = t->cur.cap;
  // eight waves per SIMD while the counters leave room for four workgroups per CU; every workgroup flushes its non-zero bins once
  const uint32_t grid = grid_for(cap, KV_HIST_THREADS * KV_HIST_ITEMS, (uint32_t)cu_count(t) * 4);
  { Launch L(t, "k_value_hist");
    KV_SWITCH_LAYOUT(t, hipLaunchKernelGGL((k_value_hist<LAY>), dim3(grid), dim3(KV_HIST_THREADS), size_t(nbins) * 4, t->stream, (const void*)t->cur.p, cap, nbins, d)); }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out_host, d, size_t(nbins) * 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  return KH_OK;
}

kh_status kh_select_values(kh_table* t, uint32_t lo, uint32_t hi, kh_mem where, uint64_t* out_keys, uint32_t* out_vals, uint64_t cap_out,
                           uint64_t* n_out) {
  if (n_out) *n_out = 0;
  if (!t) return KH_ERR_INVALID;
  if (t->ins.active) return refuse_streaming(t);
  HIPCHK(hipSetDevice(t->device));
  if (lo > hi || t->lsize == 0) { HIPCHK(hipStreamSynchronize(t->stream)); return KH_OK; }
  const uint64_t cap = t->cur.cap, kw = t->slot_bytes / sizeof(KhSlot);      // words per key
  const uint64_t ntl = (cap + KV_SEL_TILE - 1) / KV_SEL_TILE;
  { kh_status ps = arena_prepare(t, ntl * 12 + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  uint32_t* sums; uint64_t* offs;
  TAKE(sums, uint32_t, ntl); TAKE(offs, uint64_t, ntl + 1);
  { Launch L(t, "k_values_tile_count");
    KV_SWITCH_LAYOUT(t, hipLaunchKernelGGL((k_values_tile_count<LAY>), dim3((uint32_t)ntl), dim3(KV_SEL_THREADS), 0, t->stream, (const void*)t->cur.p, cap, lo, hi, sums)); }
  { Launch L(t, "k_scan");
    hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, t->stream, (const uint32_t*)sums, ntl, offs); }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t->hpin, offs + ntl, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  const uint64_t m = t->hpin[0];
  if (n_out) *n_out = m;
  if (!out_keys || m == 0) return KH_OK;
  if (m > cap_out) return fail(t, KH_ERR_INVALID, "kh_select_values: more matches than cap_out (n_out holds their number)");
  const bool host = where == KH_MEM_HOST;
  uint64_t* ck = out_keys; uint32_t* cv = out_vals;
  if (host) { TAKE(ck, uint64_t, kw * m); if (out_vals) TAKE(cv, uint32_t, m); }
  { Launch L(t, "k_values_tile_emit");
    KV_SWITCH_LAYOUT(t, hipLaunchKernelGGL((k_values_tile_emit<LAY>), dim3((uint32_t)ntl), dim3(KV_SEL_THREADS), 0, t->stream, (const void*)t->cur.p, cap, lo, hi,
                                           (const uint64_t*)offs, ck, cv)); }
  HIPCHK(hipGetLastError());
  if (host) return copy_compacted(t, m, ck, cv, out_keys, out_vals);
  HIPCHK(hipStreamSynchronize(t->stream));
  return KH_OK;
}

kh_status kh_erase_values(kh_table* t, uint32_t lo, uint32_t hi, uint64_t* n_erased) {
  if (n_erased) *n_erased = 0;
  if (!t) return KH_ERR_INVALID;
  if (t->ins.active) return refuse_streaming(t);
  HIPCHK(hipSetDevice(t->device));
  uint64_t ne = 0;
  if (lo <= hi && t->lsize > 0) {
    const uint64_t cap = t->cur.cap;
    { kh_status ps = arena_prepare(t, ws_rebuild(cap) + (cap > KH_L ? (cap >> KH_LB) : 1) * 96 + (size_t(2) << 20)); if (ps != KH_OK) return ps; }
    unsigned long long* cnt;
    TAKE(cnt, unsigned long long, 1);
    HIPCHK(hipMemsetAsync(cnt, 0, 8, t->stream));
    { Launch L(t, "k_values_mark");
      KV_SWITCH_LAYOUT(t, hipLaunchKernelGGL((k_values_mark<LAY>), dim3(grid_for(cap, KV_MARK_THREADS * KV_MARK_ITEMS, (uint32_t)cu_count(t) * 8)), dim3(KV_MARK_THREADS), 0,
                                             t->stream, t->cur.p, cap, lo, hi, cnt)); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(t->hpin, cnt, 8, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    ne = t->hpin[0];
    if (ne && t->kind == KHK_RH) {      // (LP: the tombstones are the erase)
      const kh_status st = rebuild(t, cap, nullptr, nullptr, nullptr, nullptr, 0, true, t->lsize - ne);
      if (st != KH_OK) {        // the table keeps its elements: take the marks back
        if (is_wide(t)) hipLaunchKernelGGL(kw_clear_marks, dim3(grid_for(cap, 256)), dim3(256), 0, t->stream, wide(t->cur));
        else hipLaunchKernelGGL(k_clear_marks, dim3(grid_for(cap, 256)), dim3(256), 0, t->stream, narrow(t->cur));
        hipStreamSynchronize(t->stream);
        return st;
      }
    }
    t->lsize -= ne;
    if (n_erased) *n_erased = ne;
  }
  // the tail of erase(Iter,Iter), as kh_erase / kh_wide_erase apply it (also to a batch that erased nothing)
  kh_status st = KH_OK;
  if (t->lsize < t->min_load) {
    if (t->kind == KHK_RH) st = do_reserve(t, t->lsize);   // hashmap_robinhood.hpp:1437: reserve() only grows
    else st = do_rehash(t, static_cast<uint64_t>(static_cast<float>(t->lsize) / t->max_lf));   // hashmap_linearprobe.hpp:1048
  }
  if (st == KH_OK) HIPCHK(hipStreamSynchronize(t->stream));
  return st;
}
}  // extern "C"
namespace {
inline bool xform_ok(kh_key_transform xf, uint32_t k) { return xf == KH_XF_IDENTITY || (xf == KH_XF_DNA_LEX_LESS && k >= 1 && k <= 32); }
inline KhSeed make_seed(uint64_t seed, kh_key_transform xf, uint32_t k) { return KhSeed{seed, xf == KH_XF_DNA_LEX_LESS ? k : 0u}; }
// Hash::operator()(Key const*, count, out) for keys of kw 64-bit words: stage host keys in, hash, copy the hashes out
kh_status hash_batch_impl(uint32_t kw, kh_hash hash, KhSeed seed, const void* keys, uint64_t n, kh_mem where, uint64_t* out, int device, void* stream_) {
  if (n == 0) return KH_OK;
  if (!keys || !out || (int)hash < 0 || (int)hash > 3 || !wide_keys_aligned(kw, keys, where)) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  Scratch s(device, stream);
  const uint64_t* dk = nullptr; uint64_t* dout = nullptr;
  if (!s.layout([&](Scratch& c) { dk = c.in(static_cast<const uint64_t*>(keys), n * kw, where); dout = c.out(out, n, where); })) return s.finish();
  if (kw == 2) { KH_SWITCH_HASH((int)hash, hipLaunchKernelGGL((k_hash_batch<HASH, 2>), dim3(grid_for(n, 256)), dim3(256), 0, stream, dk, n, seed.s, dout)); }
  else { KH_SWITCH_HASH((int)hash, hipLaunchKernelGGL((k_hash_batch<HASH, 1>), dim3(grid_for(n, 256)), dim3(256), 0, stream, dk, n, seed, dout)); }
  if (s.launched()) s.copy_back(dout, n);
  return s.finish();
}
// stable partition of (key, value) by destination rank = hash(key) mod p for keys of kw 64-bit words (xf / k: 8-byte keys only);
// out_keys == null: count only -- the caller sizes the exchange before it permutes (pipelined multi-GPU insert)
kh_status shard_permute_impl(uint32_t kw, kh_hash hash, uint64_t seed_, kh_key_transform xf, uint32_t k, uint32_t p, const uint64_t* keys,
                             const uint32_t* vals, uint64_t n, uint64_t* out_keys, uint32_t* out_vals, uint64_t* counts_host, int device, void* stream_) {
  if (p == 0 || p > KH_SHARD_MAXR || !counts_host || (int)hash < 0 || (int)hash > 3 || !xform_ok(xf, k)) return KH_ERR_INVALID;
  const KhSeed seed = make_seed(seed_, xf, k);
  for (uint32_t r = 0; r < p; ++r) counts_host[r] = 0;
  if (n == 0) return KH_OK;
  if (!keys || (out_keys && vals && !out_vals)) return KH_ERR_INVALID;
  const uint64_t tile = kw == 2 ? KH_SHARD_TILE(2) : KH_SHARD_TILE(1);
  if (kw == 2) {
    if (!wide_keys_aligned(2, keys, KH_MEM_DEVICE) || !wide_keys_aligned(2, out_keys, KH_MEM_DEVICE)) return KH_ERR_INVALID;     // (out_keys too: one 16-byte store per key)
    if ((n + tile - 1) / tile > 0x7FFFFFFFull) return KH_ERR_UNSUPPORTED;
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  const uint32_t ntiles = (uint32_t)((n + tile - 1) / tile);
  const uint32_t pmask = (p & (p - 1)) == 0 ? p - 1 : 0;   // power of two: & (p-1); else % p.  (p == 1: mask 0 -> % 1)
  uint32_t* tc = nullptr; uint64_t* toff = nullptr;
  const uint64_t m = (uint64_t)p * ntiles;
  Scratch s(device, stream);
  if (!s.layout([&](Scratch& c) { tc = c.take<uint32_t>(m); toff = c.take<uint64_t>(m + 1); })) return s.finish();
  // (S: the seed in the form the key width's hash takes)
#define KH_SHARD_LAUNCH(KERNEL, ...)                                                                                                                            \
  if (kw == 2) { const uint64_t S = seed.s; KH_SWITCH_HASH((int)hash, hipLaunchKernelGGL((KERNEL<HASH, 2>), dim3(ntiles), dim3(KH_SHARD_THREADS), 0, stream, __VA_ARGS__)); } \
  else { const KhSeed S = seed; KH_SWITCH_HASH((int)hash, hipLaunchKernelGGL((KERNEL<HASH, 1>), dim3(ntiles), dim3(KH_SHARD_THREADS), 0, stream, __VA_ARGS__)); }
  KH_SHARD_LAUNCH(k_shard_count, keys, n, S, p, pmask, tc, ntiles);
  hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, stream, tc, m, toff);
  if (out_keys && p <= 8) { KH_SHARD_LAUNCH(k_shard_scatter8, keys, vals, n, S, p, pmask, (const uint64_t*)toff, ntiles, out_keys, out_vals); }
  else if (out_keys) { KH_SHARD_LAUNCH(k_shard_scatter, keys, vals, n, S, p, pmask, (const uint64_t*)toff, ntiles, out_keys, out_vals); }
#undef KH_SHARD_LAUNCH
  std::vector<uint64_t> ends(p + 1);
  s.launched();
  for (uint32_t r = 0; r <= p; ++r) s.read(&ends[r], toff + (uint64_t)r * ntiles);
  const kh_status st = s.finish();
  if (st != KH_OK) return st;
  for (uint32_t r = 0; r < p; ++r) counts_host[r] = ends[r + 1] - ends[r];
  return KH_OK;
}
}
extern "C" {
kh_status kh_set_key_transform(kh_table* t, kh_key_transform xf, uint32_t k) {
  if (!t) return KH_ERR_INVALID;
  if (!xform_ok(xf, k)) return fail(t, KH_ERR_INVALID, "unknown key transform / k outside 1..32");
  if (t->lsize != 0 || t->ins.active) return fail(t, KH_ERR_INVALID, "the key transform can only be set on an empty table");
  t->seed.xk = xf == KH_XF_DNA_LEX_LESS ? k : 0u;
  return KH_OK;
}
kh_status kh_get_key_transform(const kh_table* t, kh_key_transform* xf, uint32_t* k) {
  if (!t) return KH_ERR_INVALID;
  if (xf) *xf = t->seed.xk ? KH_XF_DNA_LEX_LESS : KH_XF_IDENTITY;
  if (k) *k = t->seed.xk;
  return KH_OK;
}
kh_status kh_hash_batch(kh_hash hash, uint64_t seed, const void* keys, uint64_t n, kh_mem where, uint64_t* out, int device, void* stream_) {
  return kh_hash_batch_transformed(hash, seed, KH_XF_IDENTITY, 0, keys, n, where, out, device, stream_);
}
kh_status kh_hash_batch_transformed(kh_hash hash, uint64_t seed_, kh_key_transform xf, uint32_t k, const void* keys, uint64_t n, kh_mem where,
                                    uint64_t* out, int device, void* stream_) {
  if (n && !xform_ok(xf, k)) return KH_ERR_INVALID;
  return hash_batch_impl(1, hash, make_seed(seed_, xf, k), keys, n, where, out, device, stream_);
}

kh_status kh_shard_permute(kh_hash hash, uint64_t seed, uint32_t p, const uint64_t* keys, const uint32_t* vals, uint64_t n,
                           uint64_t* out_keys, uint32_t* out_vals, uint64_t* counts_host, int device, void* stream_) {
  return kh_shard_permute_transformed(hash, seed, KH_XF_IDENTITY, 0, p, keys, vals, n, out_keys, out_vals, counts_host, device, stream_);
}
kh_status kh_shard_permute_transformed(kh_hash hash, uint64_t seed_, kh_key_transform xf, uint32_t k, uint32_t p, const uint64_t* keys,
                                       const uint32_t* vals, uint64_t n, uint64_t* out_keys, uint32_t* out_vals, uint64_t* counts_host,
                                       int device, void* stream_) {
  return shard_permute_impl(1, hash, seed_, xf, k, p, keys, vals, n, out_keys, out_vals, counts_host, device, stream_);
}

// ---- shard plan: ONE count sweep + scan over a whole batch that is going to be exchanged in pieces; the per-piece destination
//      counts fall out of the scanned offsets at the piece boundaries (tile-aligned), and every piece is then permuted by the
//      scatter kernel alone (no second count, no second scan, one host synchronisation instead of one per piece)
struct kh_shard_plan {
  int device, hash; KhSeed seed; uint32_t p, pmask, pieces, ntiles; uint64_t n;
  void* blk; const uint64_t* toff;      // the pooled block of the scan, and the scanned [rank][tile] offsets inside it
  std::vector<uint64_t> bnd;      // [p][pieces+1] scanned offsets at the piece boundaries
  std::vector<hipStream_t> used;  // the streams a scatter that reads `toff` was queued on (kh_shard_plan_destroy frees behind them)
};
// On a runtime thread, in stream order: the rule at Scratch::release (no HIP call, no wait for anyone who makes one; the block is pooled)
// One reference per stream that still has scatters queued, one for kh_shard_plan_destroy itself: who drops the last frees the block.
struct PlanRelease { int device; void* blk; std::atomic<int> refs; };
static void plan_release(void* arg) {
  PlanRelease* r = static_cast<PlanRelease*>(arg);
  if (r->refs.fetch_sub(1) != 1) return;
  pool_free(r->device, r->blk);
  delete r;
}
kh_status kh_shard_plan_create(kh_shard_plan** out, kh_hash hash, uint64_t seed_, kh_key_transform xf, uint32_t k, uint32_t p, const uint64_t* keys,
                               uint64_t n, uint32_t pieces, uint64_t* counts_host, uint64_t* bounds_host, int device, void* stream_) {
  if (!out) return KH_ERR_INVALID;
  *out = nullptr;
  if (p == 0 || p > 8 || pieces == 0 || pieces > 64 || !counts_host || !bounds_host || (int)hash < 0 || (int)hash > 3 || !xform_ok(xf, k) || (n && !keys)) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  std::unique_ptr<kh_shard_plan> P(new kh_shard_plan());
  P->device = device; P->hash = (int)hash; P->seed = make_seed(seed_, xf, k); P->p = p; P->pmask = (p & (p - 1)) == 0 ? p - 1 : 0;
  P->pieces = pieces; P->n = n; P->blk = nullptr; P->toff = nullptr;
  P->ntiles = (uint32_t)((n + KH_SHARD_TILE(1) - 1) / KH_SHARD_TILE(1));
  for (uint32_t i = 0; i <= pieces; ++i) bounds_host[i] = std::min<uint64_t>(n, ((uint64_t)P->ntiles * i / pieces) * KH_SHARD_TILE(1));
  for (uint64_t j = 0; j < (uint64_t)pieces * p; ++j) counts_host[j] = 0;
  P->bnd.assign((size_t)p * (pieces + 1), 0);
  if (n) {
    const uint64_t m = (uint64_t)p * P->ntiles;
    uint32_t* tc = nullptr; uint64_t *toff = nullptr, *bnd_dev = nullptr;
    Scratch s(device, stream);      // (an error on the way out returns the block)
    if (!s.layout([&](Scratch& c) { tc = c.take<uint32_t>(m); toff = c.take<uint64_t>(m + 1); bnd_dev = c.take<uint64_t>(P->bnd.size()); })) return s.finish();
    KH_SWITCH_HASH((int)hash, hipLaunchKernelGGL((k_shard_count<HASH, 1>), dim3(P->ntiles), dim3(KH_SHARD_THREADS), 0, stream, keys, n, P->seed, p, P->pmask, tc, P->ntiles));
    hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, stream, tc, m, toff);
    hipLaunchKernelGGL(k_shard_piece_bounds, dim3(1 + (uint32_t)P->bnd.size() / 256), dim3(256), 0, stream, (const uint64_t*)toff, P->ntiles, p, pieces, bnd_dev);
    s.launched();
    s.read(P->bnd.data(), bnd_dev, P->bnd.size());
    if (!s.sync()) return s.finish();
    P->blk = s.keep(); P->toff = toff;      // the plan's from here on
    for (uint32_t i = 0; i < pieces; ++i)
      for (uint32_t r = 0; r < p; ++r) counts_host[(size_t)i * p + r] = P->bnd[(size_t)r * (pieces + 1) + i + 1] - P->bnd[(size_t)r * (pieces + 1) + i];
  }
  *out = P.release();
  return KH_OK;
}
// one piece through the scatter kernel.  global: to its place in the layout of the WHOLE batch grouped by rank (what kh_shard_permute of
// all n pairs gives) -- the scanned [rank][tile] offsets already are positions in that layout; else to the piece's own output, rank by rank
static kh_status shard_plan_permute(kh_shard_plan* P, uint32_t piece, const uint64_t* keys, const uint32_t* vals, uint64_t* out_keys, uint32_t* out_vals,
                                    void* stream_, bool global) {
  if (!P || piece >= P->pieces || (vals && !out_vals)) return KH_ERR_INVALID;
  if (P->n == 0) return KH_OK;
  if (!keys || !out_keys) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(P->device));
  const uint32_t t0 = (uint32_t)((uint64_t)P->ntiles * piece / P->pieces), t1 = (uint32_t)((uint64_t)P->ntiles * (piece + 1) / P->pieces);
  if (t1 == t0) return KH_OK;
  const uint64_t b0 = (uint64_t)t0 * KH_SHARD_TILE(1), b1 = std::min<uint64_t>(P->n, (uint64_t)t1 * KH_SHARD_TILE(1));
  KhShardAdj adj;      // (all zero)
  uint64_t base = 0;      // where rank r's pairs of THIS piece start in the piece's output
  for (uint32_t r = 0; r < P->p && !global; ++r) {
    const uint64_t lo = P->bnd[(size_t)r * (P->pieces + 1) + piece], hi = P->bnd[(size_t)r * (P->pieces + 1) + piece + 1];
    adj.a[r] = (long long)base - (long long)lo;
    base += hi - lo;
  }
  KH_SWITCH_HASH(P->hash, hipLaunchKernelGGL((k_shard_scatter8<HASH, 1>), dim3(t1 - t0), dim3(KH_SHARD_THREADS), 0, stream, keys + b0, vals ? vals + b0 : nullptr, b1 - b0,
                                             P->seed, P->p, P->pmask, P->toff, P->ntiles, out_keys, out_vals, t0, adj));
  if (std::find(P->used.begin(), P->used.end(), stream) == P->used.end()) P->used.push_back(stream);      // (before the check: a launch may be queued)
  HIPCHK0(hipGetLastError());
  return KH_OK;
}
kh_status kh_shard_plan_permute(kh_shard_plan* P, uint32_t piece, const uint64_t* keys, const uint32_t* vals, uint64_t* out_keys, uint32_t* out_vals,
                                void* stream_) {
  return shard_plan_permute(P, piece, keys, vals, out_keys, out_vals, stream_, false);
}
kh_status kh_shard_plan_permute_global(kh_shard_plan* P, uint32_t piece, const uint64_t* keys, const uint32_t* vals, uint64_t* out_keys, uint32_t* out_vals,
                                       void* stream_) {
  return shard_plan_permute(P, piece, keys, vals, out_keys, out_vals, stream_, true);
}
kh_status kh_shard_plan_offsets(const kh_shard_plan* P, uint64_t* out) {
  if (!P || !out) return KH_ERR_INVALID;
  for (size_t i = 0; i < P->bnd.size(); ++i) out[i] = P->bnd[i];
  if (P->n == 0) for (size_t i = 0; i < P->bnd.size(); ++i) out[i] = 0;
  return KH_OK;
}
// May be called as soon as the last permute has RETURNED: the queued scatters still read the block, so it goes back to the pool behind
// them -- a host function on every stream used (Scratch::finish_queued's way); the one that runs last frees.  A stream that refuses is
// waited for on the host.  A capturing stream can neither be waited for nor given a host node (the node would hand the block back on
// every replay): it holds nothing back, the captured scatters read the block only when replayed; the other streams still do.
void kh_shard_plan_destroy(kh_shard_plan* P) {
  if (!P) return;
  if (P->blk && !P->used.empty() && hipSetDevice(P->device) == hipSuccess) {
    PlanRelease* r = new PlanRelease{P->device, P->blk, {1}};      // (the one reference is this call's)
    P->blk = nullptr;
    for (hipStream_t s : P->used) {
      hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(s, &cap) != hipSuccess) (void)hipGetLastError();
      else if (cap != hipStreamCaptureStatusNone) continue;
      r->refs.fetch_add(1);
      if (hipLaunchHostFunc(s, &plan_release, r) != hipSuccess) { (void)hipGetLastError(); hipStreamSynchronize(s); plan_release(r); }
    }
    plan_release(r);
  }
  pool_free(P->device, P->blk);
  delete P;
}

// ---- k-mer generation front end ----------------------------------------------------------------------
}  // extern "C"
namespace {
// FASTQ text -> the same bytes with everything that is not on a sequence line replaced by '\n' (line number = newlines before the byte;
// sequence lines are 1 mod 4).  sums: u32[tiles of KH_CMP_TILE], offs: u64[tiles + 1], msk: u8[n]; queued on `stream`.
void fastq_mask_text(const uint8_t* text, uint64_t n, uint32_t* sums, uint64_t* offs, uint8_t* msk, hipStream_t stream) {
  const uint64_t ntl = (n + KH_CMP_TILE - 1) / KH_CMP_TILE;
  hipLaunchKernelGGL(k_newline_tile_sums, dim3((uint32_t)ntl), dim3(256), 0, stream, text, n, sums);
  hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, stream, sums, ntl, offs);
  hipLaunchKernelGGL(k_fastq_mask, dim3((uint32_t)ntl), dim3(256), 0, stream, text, n, (const uint64_t*)offs, msk);
}
// The text front end of the k-mer, sampling, HyperLogLog and index text calls: a host text is staged, a FASTQ text is masked, and the
// tile sums / tile offsets of the passes that follow live next to it.  carve() inside the call's layout function, mask() once it ran.
struct TextFront {
  const uint8_t* text = nullptr;      // the text the window kernels read: the caller's, its staged copy, or the masked text after mask()
  uint8_t* msk = nullptr;             // u8[n] (FASTQ)
  uint32_t* sums = nullptr;           // u32[nt]
  uint64_t* offs = nullptr;           // u64[nt + 1]
  // nt: tiles of the largest pass that uses sums / offs (FASTQ: at least those of KH_CMP_TILE; 0: none)
  void carve(Scratch& c, const void* src, uint64_t n, kh_mem where, bool fastq, uint64_t nt) {
    text = c.in(static_cast<const uint8_t*>(src), n, where);
    msk = c.take<uint8_t>(fastq ? n : 0);
    sums = c.take<uint32_t>(nt);
    offs = c.take<uint64_t>(nt ? nt + 1 : 0);
  }
  void mask(uint64_t n, hipStream_t stream) {
    if (msk) { fastq_mask_text(text, n, sums, offs, msk, stream); text = msk; }
  }
};
inline uint64_t cmp_tiles(uint64_t n) { return (n + KH_CMP_TILE - 1) / KH_CMP_TILE; }      // tiles of the FASTQ line kernels
inline uint64_t km_tiles(uint64_t n) { return (n + KH_KM_TILE - 1) / KH_KM_TILE; }         // tiles of the k-mer kernels
// shared body of kh_kmers[128]_from_sequence / kh_kmers[128]_from_fastq; kw: 64-bit words per k-mer (1: k <= 32, 2: k <= 64)
// out_pos (n < 2^32): the byte offset of every window next to its k-mer (kh_kmers[128]_from_sequence_pos / _fastq_pos)
kh_status kmers_impl(uint32_t kw, const void* seq, uint64_t n, uint32_t k, int canonical, kh_mem where, bool fastq,
                     uint64_t* out_kmers, uint64_t* n_out, int device, void* stream_, uint32_t* out_pos = nullptr) {
  if (n_out) *n_out = 0;
  if (k < 1 || k > 32 * kw || !n_out) return KH_ERR_INVALID;
  if (n < k) return KH_OK;
  if (!seq || !out_kmers || !wide_keys_aligned(kw, out_kmers, where)) return KH_ERR_INVALID;      // (kw_kmers_emit*: one 16-byte store per k-mer)
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  const uint64_t nkt = km_tiles(n);
  Scratch s(device, stream);
  TextFront F;
  uint64_t* dout = nullptr; uint32_t* dpos = nullptr;      // compacted, where the caller's memory is
  if (!s.layout([&](Scratch& c) {
        F.carve(c, seq, n, where, fastq, std::max(cmp_tiles(n), nkt));
        dout = c.out(out_kmers, n * kw, where);
        dpos = c.out(out_pos, out_pos ? n : 0, where);
      })) return s.finish();
  F.mask(n, stream);
  const uint8_t* dseq = F.text; uint32_t* sums = F.sums; const uint64_t* offs = F.offs;
  // two passes over the text: valid windows per tile, scan, then the windows themselves, compacted and in order
  if (kw == 2) hipLaunchKernelGGL(k_kmers_count<2>, dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, sums);
  else hipLaunchKernelGGL(k_kmers_count<1>, dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, sums);
  hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, stream, sums, nkt, F.offs);
  if (out_pos && kw == 2 && canonical) hipLaunchKernelGGL((kw_kmers_emit_pos<true>), dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, offs, dout, dpos);
  else if (out_pos && kw == 2) hipLaunchKernelGGL((kw_kmers_emit_pos<false>), dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, offs, dout, dpos);
  else if (out_pos && canonical) hipLaunchKernelGGL((k_kmers_emit_pos<true>), dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, offs, dout, dpos);
  else if (out_pos) hipLaunchKernelGGL((k_kmers_emit_pos<false>), dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, offs, dout, dpos);
  else if (kw == 2 && canonical) hipLaunchKernelGGL((kw_kmers_emit<true>), dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, offs, dout);
  else if (kw == 2) hipLaunchKernelGGL((kw_kmers_emit<false>), dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, offs, dout);
  else if (canonical) hipLaunchKernelGGL((k_kmers_emit<true>), dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, offs, dout);
  else hipLaunchKernelGGL((k_kmers_emit<false>), dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, offs, dout);
  s.launched();
  uint64_t total = 0;
  s.read(&total, offs + nkt);
  if (s.sync()) { s.copy_back(dout, total * kw); s.copy_back(dpos, total); }
  const kh_status st = s.finish();
  if (st != KH_OK) return st;
  *n_out = total;
  return KH_OK;
}
// (w,k)-minimizers in two steps, so that a caller can size its pair buffers from the count: mz_count stages a host text, masks FASTQ,
// runs the count pass and the scan and returns the number of picks; mz_emit writes the pairs into device buffers of that many
// entries.  The work's scratch holds the front end's block (and whatever the caller carves for the pairs) until the work goes away.
// prof: the table whose profile lists the launches (an index's own), or null.
struct MzWork {
  MzWork(int device, hipStream_t stream) : scr(device, stream) {}
  Scratch scr;
  TextFront F;
  uint64_t n = 0, nkt = 0;
  uint32_t k = 0, w = 0;
  uint32_t s = 0, kw = 1;      // s != 0 (set by the caller before mz_count): closed syncmers of kw-word k-mers instead, w unused
  int canonical = 0, hash = 0;
  uint64_t seed = 0;
};
// refusals that need no device: k, w, n, the hash and null arguments (shared by kh_minimizers_* and kh_index_*_from_minimizers)
bool mz_args_ok(const void* seq, uint64_t n, uint32_t k, uint32_t w, int hash) {
  return k >= 1 && k <= 32 && w >= 1 && w <= KM_MZ_WMAX && !(n >> 32) && hash >= 0 && hash <= 3 && (seq || n == 0);
}
kh_status mz_count(kh_table* prof, MzWork& M, const void* seq, uint64_t n, uint32_t k, uint32_t w, int canonical, int hash, uint64_t seed, kh_mem where, bool fastq,
                   hipStream_t stream, uint64_t* total) {
  M.n = n; M.k = k; M.w = w; M.canonical = canonical; M.hash = hash; M.seed = seed;
  const uint64_t nkt = km_tiles(n);
  M.nkt = nkt;
  Scratch& S = M.scr;
  if (S.layout([&](Scratch& c) { M.F.carve(c, seq, n, where, fastq, std::max(cmp_tiles(n), nkt)); })) {
    M.F.mask(n, stream);
    const uint8_t* dseq = M.F.text; uint32_t* sums = M.F.sums;
    if (M.s) { Launch L(prof, "k_syncmers_count");
      if (canonical) { KH_SWITCH_HASH(hash, hipLaunchKernelGGL((k_syncmers_count<HASH, true>), dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, M.s, seed, sums)); }
      else { KH_SWITCH_HASH(hash, hipLaunchKernelGGL((k_syncmers_count<HASH, false>), dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, M.s, seed, sums)); } }
    else { Launch L(prof, "k_minimizers_count");
      if (canonical) { KH_SWITCH_HASH(hash, hipLaunchKernelGGL((k_minimizers_count<HASH, true>), dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, w, seed, sums)); }
      else { KH_SWITCH_HASH(hash, hipLaunchKernelGGL((k_minimizers_count<HASH, false>), dim3((uint32_t)nkt), dim3(KH_KM_THREADS), 0, stream, dseq, n, k, w, seed, sums)); } }
    hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, stream, sums, nkt, M.F.offs);
    S.launched();
    S.read(total, M.F.offs + nkt);
    S.sync();
  }
  if (!S.ok()) { const std::string msg = std::string("minimizer count pass: ") + hipGetErrorString(S.error()); return fail(prof, S.finish(), msg); }
  return KH_OK;
}
// queues the emit pass (dout u64[total], dpos u32[total], device memory); the caller synchronises
kh_status mz_emit(kh_table* prof, MzWork& M, hipStream_t stream, uint64_t* dout, uint32_t* dpos, uint32_t pos_base) {
  const uint8_t* dseq = M.F.text; const uint64_t* offs = M.F.offs;
  if (M.s) { Launch L(prof, "k_syncmers_emit");
#define KH_SY_EMIT(CANON, KW) KH_SWITCH_HASH(M.hash, hipLaunchKernelGGL((k_syncmers_emit<HASH, CANON, KW>), dim3((uint32_t)M.nkt), dim3(KH_KM_THREADS), 0, stream, dseq, M.n, M.k, M.s, \
                                                                  M.seed, offs, dout, dpos, pos_base))
    if (M.kw == 2) { if (M.canonical) { KH_SY_EMIT(true, 2); } else { KH_SY_EMIT(false, 2); } }
    else if (M.canonical) { KH_SY_EMIT(true, 1); }
    else { KH_SY_EMIT(false, 1); }
#undef KH_SY_EMIT
  }
  else { Launch L(prof, "k_minimizers_emit");
    if (M.canonical) { KH_SWITCH_HASH(M.hash, hipLaunchKernelGGL((k_minimizers_emit<HASH, true>), dim3((uint32_t)M.nkt), dim3(KH_KM_THREADS), 0, stream, dseq, M.n, M.k, M.w, M.seed,
                                                                 offs, dout, dpos, pos_base)); }
    else { KH_SWITCH_HASH(M.hash, hipLaunchKernelGGL((k_minimizers_emit<HASH, false>), dim3((uint32_t)M.nkt), dim3(KH_KM_THREADS), 0, stream, dseq, M.n, M.k, M.w, M.seed,
                                                     offs, dout, dpos, pos_base)); } }
  if (!M.scr.launched()) return hip_fail(prof, "minimizer emit pass", M.scr.error());
  return KH_OK;
}
// shared body of kh_minimizers_* and kh_syncmers[128]_*: the entry family has preset the work (M.s, M.kw) and judged its own arguments;
// min_n: the shortest text that holds a window.  The pairs of a host call are staged in a second block, sized by the count
kh_status sampled_impl(MzWork& M, bool args_ok, uint64_t min_n, const void* seq, uint64_t n, uint32_t k, uint32_t w, int canonical, int hash, uint64_t seed, kh_mem where,
                       bool fastq, uint64_t* out_kmers, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out, int device, hipStream_t stream) {
  if (n_out) *n_out = 0;
  if (!n_out || !args_ok || (out_kmers && !out_pos)) return KH_ERR_INVALID;
  if (!wide_keys_aligned(M.kw, out_kmers, where)) return KH_ERR_INVALID;      // (k_syncmers_emit<2>: one 16-byte store per k-mer; before the count pass)
  if (n < min_n) return KH_OK;
  HIPCHK0(hipSetDevice(device));
  uint64_t total = 0;
  kh_status st = mz_count(nullptr, M, seq, n, k, w, canonical, hash, seed, where, fastq, stream, &total);
  if (st != KH_OK) return st;
  *n_out = total;
  if (!out_kmers || total == 0) return KH_OK;
  if (total > cap_out) return KH_ERR_INVALID;       // (the total is known before anything is written)
  uint64_t* dout = nullptr; uint32_t* dpos = nullptr;
  if (!M.scr.layout([&](Scratch& c) { dout = c.out(out_kmers, total * M.kw, where); dpos = c.out(out_pos, total, where); })) return M.scr.finish();
  st = mz_emit(nullptr, M, stream, dout, dpos, 0u);
  M.scr.copy_back(dout, total * M.kw);
  M.scr.copy_back(dpos, total);
  const kh_status fs = M.scr.finish();
  return fs != KH_OK ? fs : st;
}
kh_status minimizers_impl(const void* seq, uint64_t n, uint32_t k, uint32_t w, int canonical, int hash, uint64_t seed, kh_mem where, bool fastq,
                          uint64_t* out_kmers, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out, int device, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MzWork M(device, stream);
  return sampled_impl(M, mz_args_ok(seq, n, k, w, hash), (uint64_t)w + k - 1, seq, n, k, w, canonical, hash, seed, where, fastq, out_kmers, out_pos, cap_out, n_out, device, stream);
}
// refusals of the syncmer calls that need no device: s, k for the key width, n, the hash and a null text
bool sy_args_ok(uint32_t kw, const void* seq, uint64_t n, uint32_t k, uint32_t s, int hash) {
  return s >= 1 && s <= k && s <= 32 && k <= 32 * kw && !(n >> 32) && hash >= 0 && hash <= 3 && (seq || n == 0);
}
// closed syncmers of a text: the minimizer route with the syncmer kernels; kw: 64-bit words per emitted k-mer
kh_status syncmers_impl(uint32_t kw, const void* seq, uint64_t n, uint32_t k, uint32_t s, int canonical, int hash, uint64_t seed, kh_mem where, bool fastq,
                        uint64_t* out_kmers, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out, int device, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  MzWork M(device, stream);
  M.s = s; M.kw = kw;
  return sampled_impl(M, sy_args_ok(kw, seq, n, k, s, hash), k, seq, n, k, 0u, canonical, hash, seed, where, fastq, out_kmers, out_pos, cap_out, n_out, device, stream);
}
// the keep test on a batch of packed k-mers: out_mask u8[n] in the memory the keys live in
kh_status syncmer_mask_impl(uint32_t kw, const void* keys, uint64_t n, uint32_t k, uint32_t s, int canonical, int hash, uint64_t seed, kh_mem where, uint8_t* out_mask,
                            int device, void* stream_) {
  if (!sy_args_ok(kw, keys, n, k, s, hash)) return KH_ERR_INVALID;
  if (n == 0) return KH_OK;
  if (!out_mask || !wide_keys_aligned(kw, keys, where)) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  Scratch scr(device, stream);
  const uint64_t* dk = nullptr; uint8_t* dm = nullptr;
  if (!scr.layout([&](Scratch& c) { dk = c.in(static_cast<const uint64_t*>(keys), n * kw, where); dm = c.out(out_mask, n, where); })) return scr.finish();
  const uint32_t grid = grid_for(n, 256);
#define KH_SY_MASK(CANON, KW) KH_SWITCH_HASH(hash, hipLaunchKernelGGL((k_syncmer_mask<HASH, CANON, KW>), dim3(grid), dim3(256), 0, stream, dk, n, k, s, seed, dm))
  if (kw == 2) { if (canonical) { KH_SY_MASK(true, 2); } else { KH_SY_MASK(false, 2); } }
  else if (canonical) { KH_SY_MASK(true, 1); }
  else { KH_SY_MASK(false, 1); }
#undef KH_SY_MASK
  scr.launched();
  scr.copy_back(dm, n);
  scr.sync();      // (device memory too: the mask is ready when the call returns)
  return scr.finish();
}
}  // namespace
extern "C" {
kh_status kh_syncmers_from_sequence(const void* seq, uint64_t n, uint32_t k, uint32_t s, int canonical, kh_hash order_hash, uint64_t order_seed, kh_mem where,
                                    uint64_t* out_kmers, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out, int device, void* stream_) {
  return syncmers_impl(1, seq, n, k, s, canonical, (int)order_hash, order_seed, where, false, out_kmers, out_pos, cap_out, n_out, device, stream_);
}
kh_status kh_syncmers_from_fastq(const void* text, uint64_t n, uint32_t k, uint32_t s, int canonical, kh_hash order_hash, uint64_t order_seed, kh_mem where,
                                 uint64_t* out_kmers, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out, int device, void* stream_) {
  return syncmers_impl(1, text, n, k, s, canonical, (int)order_hash, order_seed, where, true, out_kmers, out_pos, cap_out, n_out, device, stream_);
}
kh_status kh_syncmers128_from_sequence(const void* seq, uint64_t n, uint32_t k, uint32_t s, int canonical, kh_hash order_hash, uint64_t order_seed, kh_mem where,
                                       uint64_t* out_kmers, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out, int device, void* stream_) {
  return syncmers_impl(2, seq, n, k, s, canonical, (int)order_hash, order_seed, where, false, out_kmers, out_pos, cap_out, n_out, device, stream_);
}
kh_status kh_syncmers128_from_fastq(const void* text, uint64_t n, uint32_t k, uint32_t s, int canonical, kh_hash order_hash, uint64_t order_seed, kh_mem where,
                                    uint64_t* out_kmers, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out, int device, void* stream_) {
  return syncmers_impl(2, text, n, k, s, canonical, (int)order_hash, order_seed, where, true, out_kmers, out_pos, cap_out, n_out, device, stream_);
}
kh_status kh_syncmer_mask(const void* keys, uint64_t n, uint32_t k, uint32_t s, int canonical, kh_hash order_hash, uint64_t order_seed, kh_mem where, uint8_t* out_mask,
                          int device, void* stream_) {
  return syncmer_mask_impl(1, keys, n, k, s, canonical, (int)order_hash, order_seed, where, out_mask, device, stream_);
}
kh_status kh_wide_syncmer_mask(const void* keys, uint64_t n, uint32_t k, uint32_t s, int canonical, kh_hash order_hash, uint64_t order_seed, kh_mem where, uint8_t* out_mask,
                               int device, void* stream_) {
  return syncmer_mask_impl(2, keys, n, k, s, canonical, (int)order_hash, order_seed, where, out_mask, device, stream_);
}
kh_status kh_minimizers_from_sequence(const void* seq, uint64_t n, uint32_t k, uint32_t w, int canonical, kh_hash order_hash, uint64_t order_seed, kh_mem where,
                                      uint64_t* out_kmers, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out, int device, void* stream_) {
  return minimizers_impl(seq, n, k, w, canonical, (int)order_hash, order_seed, where, false, out_kmers, out_pos, cap_out, n_out, device, stream_);
}
kh_status kh_minimizers_from_fastq(const void* text, uint64_t n, uint32_t k, uint32_t w, int canonical, kh_hash order_hash, uint64_t order_seed, kh_mem where,
                                   uint64_t* out_kmers, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out, int device, void* stream_) {
  return minimizers_impl(text, n, k, w, canonical, (int)order_hash, order_seed, where, true, out_kmers, out_pos, cap_out, n_out, device, stream_);
}
kh_status kh_kmers_from_sequence(const void* seq, uint64_t n, uint32_t k, int canonical, kh_mem where,
                                 uint64_t* out_kmers, uint64_t* n_out, int device, void* stream_) {
  return kmers_impl(1, seq, n, k, canonical, where, false, out_kmers, n_out, device, stream_);
}
kh_status kh_kmers_from_fastq(const void* text, uint64_t n, uint32_t k, int canonical, kh_mem where,
                              uint64_t* out_kmers, uint64_t* n_out, int device, void* stream_) {
  return kmers_impl(1, text, n, k, canonical, where, true, out_kmers, n_out, device, stream_);
}
// the same k-mers in the same order, each with the byte offset of its window's first base in the buffer passed (positions are 32-bit:
// a text of 2^32 bytes or more is refused before anything is allocated or read)
kh_status kh_kmers_from_sequence_pos(const void* seq, uint64_t n, uint32_t k, int canonical, kh_mem where,
                                     uint64_t* out_kmers, uint32_t* out_pos, uint64_t* n_out, int device, void* stream_) {
  if (n_out) *n_out = 0;
  if (n >> 32) return KH_ERR_INVALID;
  if (n >= k && !out_pos) return KH_ERR_INVALID;
  return kmers_impl(1, seq, n, k, canonical, where, false, out_kmers, n_out, device, stream_, out_pos);
}
kh_status kh_kmers_from_fastq_pos(const void* text, uint64_t n, uint32_t k, int canonical, kh_mem where,
                                  uint64_t* out_kmers, uint32_t* out_pos, uint64_t* n_out, int device, void* stream_) {
  if (n_out) *n_out = 0;
  if (n >> 32) return KH_ERR_INVALID;
  if (n >= k && !out_pos) return KH_ERR_INVALID;
  return kmers_impl(1, text, n, k, canonical, where, true, out_kmers, n_out, device, stream_, out_pos);
}

// ---- HyperLogLog (hyperloglog64.hpp) --------------------------------------------------------------
}  // extern "C"
struct kh_hll {
  int device, hash; uint64_t seed; uint32_t precision, ignored; uint32_t* regs; hipStream_t stream;
  // workspace of the text passes (window counter, FASTQ line sums / offsets, masked text): owned by the estimator so that a call on device
  // memory can return without synchronising; reused by the next call in stream order (ws_stream: the stream its last user was queued on)
  char* ws; size_t ws_cap; hipStream_t ws_stream; int ncu;
};
extern "C" {
kh_status kh_hll_create(kh_hll** out, uint32_t precision, uint32_t ignore_msb, kh_hash hash, uint64_t seed, int device) {
  if (!out) return KH_ERR_INVALID;
  *out = nullptr;
  if (precision < 4 || precision > 18 || precision + ignore_msb >= 64 || (int)hash < 0 || (int)hash > 3) return KH_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return KH_ERR_HIP;
  HIPCHK0(hipSetDevice(device));
  kh_hll* h = new kh_hll();
  h->device = device; h->hash = (int)hash; h->seed = seed; h->precision = precision; h->ignored = ignore_msb; h->stream = nullptr; h->regs = nullptr;
  if (pool_alloc(device, sizeof(uint32_t) << precision, reinterpret_cast<void**>(&h->regs)) != hipSuccess) { delete h; return KH_ERR_NOMEM; }
  if (hipMemset(h->regs, 0, sizeof(uint32_t) << precision) != hipSuccess) { pool_free(device, h->regs); delete h; return KH_ERR_HIP; }
  *out = h;
  return KH_OK;
}
kh_status kh_hll_destroy(kh_hll* h) {
  if (!h) return KH_OK;
  hipSetDevice(h->device);
  hipStreamSynchronize(h->stream);
  if (h->ws) { hipStreamSynchronize(h->ws_stream); pool_free(h->device, h->ws); }
  pool_free(h->device, h->regs);
  delete h;
  return KH_OK;
}
kh_status kh_hll_set_stream(kh_hll* h, void* s) {
  if (!h) return KH_ERR_INVALID;
  if (h->stream == static_cast<hipStream_t>(s)) return KH_OK;     // unchanged: nothing to order
  hipSetDevice(h->device);
  hipStreamSynchronize(h->stream);                                   // work already issued stays ordered before the new stream's
  h->stream = static_cast<hipStream_t>(s);
  return KH_OK;
}
// kw: 64-bit words per key (2: 16-byte keys, from_keys only)
static kh_status hll_update(kh_hll* h, const void* in, uint64_t n, kh_mem where, bool from_keys, uint32_t kw = 1) {
  if (!h) return KH_ERR_INVALID;
  if (n == 0) return KH_OK;
  if (!in) return KH_ERR_INVALID;
  if (from_keys && !wide_keys_aligned(kw, in, where)) return KH_ERR_INVALID;
  HIPCHK0(hipSetDevice(h->device));
  Scratch s(h->device, h->stream);
  const uint64_t* d = nullptr;
  if (!s.layout([&](Scratch& c) { d = c.in(static_cast<const uint64_t*>(in), n * kw, where); })) return s.finish();
  const int use_lds = h->precision <= 13 ? 1 : 0;
  const size_t smem = use_lds ? (sizeof(uint32_t) << h->precision) : 0;
  const uint32_t grid = grid_for(n, 256, 1024);
  const KhHllRegs R{h->regs, h->precision, h->ignored, use_lds};
  if (kw == 2) { KH_SWITCH_HASH(h->hash, hipLaunchKernelGGL((k_hll_update<HASH, KH_HLL_WIDE_KEYS>), dim3(grid), dim3(256), smem, h->stream, d, n, h->seed, R)); }
  else if (from_keys) { KH_SWITCH_HASH(h->hash, hipLaunchKernelGGL((k_hll_update<HASH, KH_HLL_KEYS>), dim3(grid), dim3(256), smem, h->stream, d, n, KhSeed{h->seed, 0u}, R)); }
  else hipLaunchKernelGGL((k_hll_update<KHH_IDENTITY, KH_HLL_HASHVALS>), dim3(grid), dim3(256), smem, h->stream, d, n, KhSeed{h->seed, 0u}, R);
  s.launched();
  return s.finish();
}
kh_status kh_hll_update(kh_hll* h, const void* keys, uint64_t n, kh_mem where) { return hll_update(h, keys, n, where, true); }
kh_status kh_hll_update_via_hashval(kh_hll* h, const void* hashes, uint64_t n, kh_mem where) { return hll_update(h, hashes, n, where, false); }
kh_status kh_hll_update_wide(kh_hll* h, const void* keys, uint64_t n, kh_mem where) { return hll_update(h, keys, n, where, true, 2); }

// the fused text pass: text [-> k_fastq_mask] -> k_hll_from_text.  Grid: min(tiles of KH_KM_TILE positions, KH_HLL_TEXT_WGS_PER_CU x CUs).
static kh_status hll_from_text(kh_hll* h, const void* text, uint64_t n, uint32_t k, int canonical, kh_mem where, bool fastq, uint64_t* n_kmers) {
  if (n_kmers) *n_kmers = 0;
  if (!h || k < 1 || k > 64) return KH_ERR_INVALID;
  if (n < k) return KH_OK;      // (n == 0 included) no window: the registers stay as they are
  if (!text) return KH_ERR_INVALID;
  HIPCHK0(hipSetDevice(h->device));
  if (!h->ncu) h->ncu = cu_count(h->device);
  // the estimator's own workspace, carved like a call's block: the window counter, then the text front end (line sums / offsets: FASTQ only)
  Scratch s(h->device, h->stream);
  unsigned long long* counter = nullptr;
  TextFront F;
  auto lay = [&](Scratch& c) { counter = c.take<unsigned long long>(1); F.carve(c, text, n, where, fastq, fastq ? cmp_tiles(n) : 0); };
  const size_t need = s.measure(lay);
  if (h->ws && h->ws_stream != h->stream) HIPCHK0(hipStreamSynchronize(h->ws_stream));      // its last user ran on another stream
  if (h->ws_cap < need) {
    if (h->ws) { HIPCHK0(hipStreamSynchronize(h->ws_stream)); pool_free(h->device, h->ws); h->ws = nullptr; h->ws_cap = 0; }
    HIPCHK0(pool_alloc(h->device, need, reinterpret_cast<void**>(&h->ws)));
    h->ws_cap = need;
  }
  h->ws_stream = h->stream;
  s.carve(h->ws, lay);
  if (!s.ok()) return s.finish();
  F.mask(n, h->stream);
  const uint8_t* dseq = F.text;
  if (n_kmers) s.zero(counter, 8); else counter = nullptr;
  const int use_lds = h->precision <= 13 ? 1 : 0;
  const size_t smem = use_lds ? (sizeof(uint32_t) << h->precision) : 0;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(km_tiles(n), (uint64_t)KH_HLL_TEXT_WGS_PER_CU * (uint64_t)h->ncu);
  const KhHllRegs R{h->regs, h->precision, h->ignored, use_lds};
#define KH_HLL_TEXT_LAUNCH(KW, CANON) \
  KH_SWITCH_HASH(h->hash, hipLaunchKernelGGL((k_hll_from_text<HASH, KW, CANON>), dim3(grid), dim3(KH_KM_THREADS), smem, h->stream, dseq, n, k, h->seed, R, counter))
  if (k > 32) { if (canonical) { KH_HLL_TEXT_LAUNCH(2, true); } else { KH_HLL_TEXT_LAUNCH(2, false); } }
  else { if (canonical) { KH_HLL_TEXT_LAUNCH(1, true); } else { KH_HLL_TEXT_LAUNCH(1, false); } }
#undef KH_HLL_TEXT_LAUNCH
  s.launched();
  unsigned long long total = 0;
  if (n_kmers) s.read(&total, counter);
  const kh_status st = s.finish();      // (waits for the count or for a host text; a call on device memory without a count only queues)
  if (st == KH_OK && n_kmers) *n_kmers = total;
  return st;
}
kh_status kh_hll_update_from_sequence(kh_hll* h, const void* seq, uint64_t n, uint32_t k, int canonical, kh_mem where, uint64_t* n_kmers) {
  return hll_from_text(h, seq, n, k, canonical, where, false, n_kmers);
}
kh_status kh_hll_update_from_fastq(kh_hll* h, const void* text, uint64_t n, uint32_t k, int canonical, kh_mem where, uint64_t* n_kmers) {
  return hll_from_text(h, text, n, k, canonical, where, true, n_kmers);
}
kh_status kh_hll_merge(kh_hll* h, const kh_hll* other) {
  if (!h || !other || h->precision != other->precision || h->device != other->device) return KH_ERR_INVALID;
  HIPCHK0(hipSetDevice(h->device));
  const uint32_t m = 1u << h->precision;
  if (other->stream != h->stream) HIPCHK0(hipStreamSynchronize(other->stream));      // other's pending updates land before its registers are read
  hipLaunchKernelGGL(k_hll_merge, dim3((m + 255) / 256), dim3(256), 0, h->stream, h->regs, other->regs, m);
  HIPCHK0(hipGetLastError());
  return KH_OK;
}
kh_status kh_hll_clear(kh_hll* h) {
  if (!h) return KH_ERR_INVALID;
  HIPCHK0(hipSetDevice(h->device));
  HIPCHK0(hipMemsetAsync(h->regs, 0, sizeof(uint32_t) << h->precision, h->stream));
  return KH_OK;
}
kh_status kh_hll_registers(kh_hll* h, uint8_t* out_host) {
  if (!h || !out_host) return KH_ERR_INVALID;
  HIPCHK0(hipSetDevice(h->device));
  const uint32_t m = 1u << h->precision;
  std::vector<uint32_t> r(m);
  HIPCHK0(hipMemcpyAsync(r.data(), h->regs, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, h->stream));
  HIPCHK0(hipStreamSynchronize(h->stream));
  for (uint32_t i = 0; i < m; ++i) out_host[i] = (uint8_t)r[i];
  return KH_OK;
}
// internal_estimate (hyperloglog64.hpp:201-236): same operation order in double, so equal registers give an equal double
kh_status kh_hll_estimate(kh_hll* h, double* out) {
  if (!h || !out) return KH_ERR_INVALID;
  const uint32_t m = 1u << h->precision;
  std::vector<uint8_t> regs(m);
  kh_status st = kh_hll_registers(h, regs.data());
  if (st != KH_OK) return st;
  return kh_hll_estimate_registers(regs.data(), h->precision, out);
}
kh_status kh_hll_estimate_registers(const uint8_t* regs, uint32_t precision, double* out) {
  if (!regs || !out || precision < 4 || precision > 18) return KH_ERR_INVALID;
  const uint32_t m = 1u << precision;
  struct { uint32_t precision; } hh = {precision}; auto* h = &hh;
  double amm;
  switch (h->precision) {
    case 4: amm = 0.673; break;
    case 5: amm = 0.697; break;
    case 6: amm = 0.709; break;
    default: amm = 0.7213 / (1.0 + (1.079 / static_cast<double>(m))); break;
  }
  amm *= static_cast<double>(0x1ULL << (h->precision << 1U));
  double sum = 0.0;
  uint32_t zeros = 0;
  for (uint32_t i = 0; i < m; ++i) { sum += 1.0 / static_cast<double>(1ULL << regs[i]); if (regs[i] == 0) ++zeros; }
  double est = amm / sum;
  if (est <= static_cast<double>(5ULL * (m >> 1ULL))) {
    if (zeros > 0) est = static_cast<double>(m) * std::log(static_cast<double>(m) / static_cast<double>(zeros));
  }
  *out = est;
  return KH_OK;
}

kh_status kh_profile_enable(kh_table* t, int on) { if (!t) return KH_ERR_INVALID; prof_collect(t); t->prof = on != 0; return KH_OK; }
kh_status kh_profile_reset(kh_table* t) { if (!t) return KH_ERR_INVALID; prof_collect(t); t->prof_acc.clear(); return KH_OK; }
kh_status kh_profile_query(kh_table* t, const char* prefix, double* total_ms, uint64_t* launches) {
  if (!t || !prefix) return KH_ERR_INVALID;
  prof_collect(t);
  double ms = 0; uint64_t n = 0;
  const size_t pl = strlen(prefix);
  for (auto& a : t->prof_acc) if (a.first.compare(0, pl, prefix) == 0) { ms += a.second.first; n += a.second.second; }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = n;
  return KH_OK;
}
kh_status kh_profile_dump(kh_table* t, char* buf, uint64_t cap) {
  if (!t || !buf || cap == 0) return KH_ERR_INVALID;
  prof_collect(t);
  std::string s;
  char line[256];
  for (auto& a : t->prof_acc) {
    snprintf(line, sizeof(line), "%s %llu %.6f\n", a.first.c_str(), (unsigned long long)a.second.second, a.second.first);
    s += line;
  }
  snprintf(buf, cap, "%s", s.c_str());
  return KH_OK;
}

}  // extern "C"

#ifdef KH_TRACE
extern "C" int kh_debug_trace(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(kh_trace), sizeof(unsigned long long) * 512 * 12); }
#endif

// ===================================================================================================
// Wide keys: the 16-byte-key Robin Hood table (kh_wtable) and the 128-bit k-mer front end (kernels: kh_kernels_wide.h).
// A kh_wtable IS a kh_table with 32-byte slots: buffer lifecycle, capacity rules, the general re-layout driver, the host epilogues
// and every state accessor are the 64-bit table's own code.  What is wide-only is below: the insert pass (partition -> kw_dedup ->
// capacity decision -> rebuild), the probing find and the mark-and-re-lay-out erase.  The old buffer stays current until the new
// one is complete, so a failing batch leaves the table unchanged.
// ===================================================================================================
namespace {
// workspace of one insert pass of n keys at partitioning capacity cap_u
inline size_t kw_ws_insert(uint64_t n, uint64_t cap_u) {
  const uint64_t np = cap_u > KH_L ? (cap_u >> KH_LB) : 1;
  return n * (sizeof(KwRec) + 16 + 4 + 8 + 4 + 16 + 4) + np * 48 + ws_rebuild(cap_u) + (size_t(4) << 20);
}

// the per-partition counts of one source added to cnt (queued; the counting half of the partition)
kh_status kw_count_source(kh_wtable* t, const uint64_t* keys, uint64_t n, uint32_t PB, uint32_t* cnt) {
  if (n == 0) return KH_OK;
  Launch L(t, "kw_part_count");
  KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((kw_part_count<HASH>), dim3(grid_for(n, KW_PART_THREADS, 4096)), dim3(KW_PART_THREADS), 0, t->stream, keys, n,
                                             t->seed.s, PB, cnt));
  return KH_OK;
}
// one insert() pass over device-resident keys (u64[2n]) / values (u32[n] or null); n < 2^32.  The n keys are the concatenation of
// nsrc sources (the pieces of a streamed insert; one for a plain insert).  precnt: the per-partition counts of all sources are
// already queued on the stream into that array (every kh_wide_insert_feed counted its piece when it arrived).
struct KwSrc { const uint64_t* k; const uint32_t* v; uint64_t n; };
kh_status kw_insert_core(kh_wtable* t, const KwSrc* src, uint32_t nsrc, uint64_t n, int mode, uint64_t forced_cap, uint64_t* n_new_out,
                         uint32_t* precnt = nullptr) {
  *n_new_out = 0;
  if (n == 0) return KH_OK;
  const uint64_t cap_u = forced_cap ? forced_cap : capacity_after(t, t->cur.cap, t->lsize, n, n, n - 1);
  const uint32_t PB = cap_u > KH_L ? log2u(cap_u >> KH_LB) : 0u;
  if (PB > 22) return fail(t, KH_ERR_UNSUPPORTED, "batch would need more than 2^22 partitions");
  const uint32_t nparts = 1u << PB;
  const bool plus = is_reduce(mode), plus_live = plus && t->lsize > 0;      // (plus: any Reducer)
  uint32_t *cnt, *cnt_new, *cnt_upd = nullptr, *flags, *nv, *uv = nullptr; uint64_t *off, *noff, *nk, *us = nullptr;
  unsigned long long *cursor, *scal; KwRec* rec;
  if (precnt) cnt = precnt; else TAKE(cnt, uint32_t, nparts);
  TAKE(off, uint64_t, nparts + 1); TAKE(cursor, unsigned long long, nparts); TAKE(rec, KwRec, n);
  TAKE(cnt_new, uint32_t, nparts); TAKE(noff, uint64_t, nparts + 1); TAKE(nk, uint64_t, 2 * n); TAKE(nv, uint32_t, n);
  TAKE(flags, uint32_t, KH_NFLAGS); TAKE(scal, unsigned long long, 2);
  if (plus_live) { TAKE(cnt_upd, uint32_t, nparts); TAKE(us, uint64_t, n); TAKE(uv, uint32_t, n); }
  HIPCHK(hipMemsetAsync(flags, 0, sizeof(uint32_t) * KH_NFLAGS, t->stream));
  HIPCHK(hipMemsetAsync(scal, 0, 16, t->stream));
  if (!precnt) {
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * nparts, t->stream));
    for (uint32_t s = 0; s < nsrc; ++s) { kh_status cs = kw_count_source(t, src[s].k, src[s].n, PB, cnt); if (cs != KH_OK) return cs; }
  }
  { Launch L(t, "k_scan");
    hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, t->stream, cnt, (uint64_t)nparts, off); }
  HIPCHK(hipMemcpyAsync(cursor, off, sizeof(uint64_t) * nparts, hipMemcpyDeviceToDevice, t->stream));
  { uint64_t pos0 = 0;
    for (uint32_t s = 0; s < nsrc; ++s) {        // the records of source s carry the stream positions pos0 ..
      if (src[s].n == 0) continue;
      Launch L(t, "kw_part_scatter");
      KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((kw_part_scatter<HASH>), dim3(grid_for(src[s].n, KW_PART_THREADS, 4096)), dim3(KW_PART_THREADS), 0, t->stream,
                                                 src[s].k, src[s].v, mode == INS_PLUS ? 1u : 0u, src[s].n, t->seed.s, PB, cursor, rec, (uint32_t)pos0));
      pos0 += src[s].n;
    } }
  KwDedupParams D;
  memset(&D, 0, sizeof(D));
  D.rec = rec; D.off = off; D.T = wide(t->cur); D.seed = t->seed.s; D.table_empty = t->lsize == 0 ? 1 : 0;
  D.mode = plus ? KH_DEDUP_PLUS : KH_DEDUP_FIRST; D.rop = reduce_op(mode);
  D.nk = nk; D.nv = nv; D.cnt_new = cnt_new; D.us = us; D.uv = uv; D.cnt_upd = cnt_upd; D.max_idx_plus1 = scal; D.flags = flags;
  { Launch L(t, "kw_dedup");
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((kw_dedup<HASH>), dim3(nparts), dim3(KW_DD_THREADS), 0, t->stream, D)); }
  { Launch L(t, "k_scan");
    hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, t->stream, cnt_new, (uint64_t)nparts, noff); }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t->hpin, noff + nparts, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipMemcpyAsync(t->hpin + 1, scal, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipMemcpyAsync(t->hpin + 2, flags, sizeof(uint32_t) * KH_NFLAGS, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  if (reinterpret_cast<const uint32_t*>(t->hpin + 2)[KH_FLAG_INTERNAL]) return fail(t, KH_ERR_HIP, kDedupOverflowText);
  const uint64_t dnew = t->hpin[0];
  const uint64_t last_first = plus ? n - 1 : (t->hpin[1] ? t->hpin[1] - 1 : 0);
  auto apply_plus = [&](int sign) {
    Launch L(t, mode == INS_PLUS ? "kw_apply_plus" : "kw_apply_reduce");
    hipLaunchKernelGGL(kw_apply_reduce, dim3(std::min<uint32_t>(nparts, 4096u)), dim3(256), 0, t->stream, wide(t->cur).s, (const uint64_t*)off,
                       (const uint32_t*)cnt_upd, (const uint64_t*)us, uv, nparts, sign, reduce_op(mode));
  };
  if (plus_live) apply_plus(+1);
  const uint64_t new_cap = forced_cap ? forced_cap : capacity_after(t, t->cur.cap, t->lsize, n, dnew, last_first);
  if (dnew > 0 || new_cap != t->cur.cap) {
    // a chunk of the new table owns 2^(PB-k) consecutive partitions: their lists are read in place when that is a handful, gathered
    // into one dense list when the capacity ended far below the partitioning capacity (duplicates)
    const uint32_t k_new = new_cap > KH_L ? log2u(new_cap >> KH_LB) : 0u;
    const uint64_t* ck = nullptr; const uint32_t* cv = nullptr; const uint64_t* lo = nullptr; const uint32_t* lc = nullptr;
    if (dnew > 0) {
      if (PB - k_new <= 3) { ck = nk; cv = nv; lo = off; lc = cnt_new; }
      else {
        uint64_t* gk; uint32_t* gv;
        TAKE(gk, uint64_t, 2 * dnew); TAKE(gv, uint32_t, dnew);
        Launch L(t, "kw_gather_new");
        hipLaunchKernelGGL(kw_gather_new, dim3(nparts), dim3(256), 0, t->stream, (const uint64_t*)off, (const uint64_t*)noff, (const uint64_t*)nk,
                           (const uint32_t*)nv, gk, gv);
        ck = gk; cv = gv; lo = noff; lc = nullptr;
      }
    }
    kh_status st = rebuild(t, new_cap, ck, cv, lo, lc, PB, false, t->lsize + dnew);
    if (st != KH_OK) {        // the table keeps its layout: it must keep its values too
      if (plus_live) { apply_plus(-1); hipStreamSynchronize(t->stream); }
      return st;
    }
    t->lsize += dnew;
  }
  *n_new_out = dnew;
  return KH_OK;
}

// insert(Iter,Iter) / the reducer insert over device-resident input: passes cut only where the one-doubling-per-call rule or the
// 32-bit stream positions demand it (insert_device), then the trailing reserve(size())
kh_status kw_insert_device(kh_wtable* t, const uint64_t* kb, const uint32_t* vb, uint64_t n, int mode, uint64_t* n_inserted) {
  const size_t keep_blk = t->blk, keep_off = t->off;
  uint64_t total_new = 0, done = 0;
  kh_status st = KH_OK;
  while (done < n && st == KH_OK) {
    uint64_t take = n - done, forced = 0;
    if (t->lsize >= threshold(t->cur.cap << 1, t->max_lf)) {       // more than one doubling pending: peel one call (insert_device)
      take = 1;
      forced = t->cur.cap << 1;
      while (t->lsize > threshold(forced, t->max_lf)) forced <<= 1;
    }
    if (take > g_max_pass) take = g_max_pass;
    t->blk = keep_blk; t->off = keep_off;
    uint64_t nn = 0;
    const KwSrc one = {kb + 2 * done, vb ? vb + done : nullptr, take};
    st = kw_insert_core(t, &one, 1, take, mode, forced, &nn);
    total_new += nn;
    done += take;
  }
  if (st == KH_OK) st = do_reserve(t, t->lsize);
  if (st == KH_OK) HIPCHK(hipStreamSynchronize(t->stream));
  if (n_inserted) *n_inserted = total_new;
  return st;
}
kh_status kw_do_insert(kh_wtable* t, const void* keys, const void* vals, uint64_t n, kh_mem where, int mode, uint64_t* n_inserted) {
  if (n_inserted) *n_inserted = 0;
  if (t->ins.active) return refuse_streaming(t);
  if (n && !keys) return fail(t, KH_ERR_INVALID, "null keys");
  if (n && !wide_keys_aligned(2, keys, where)) return fail(t, KH_ERR_INVALID, kWideKeysMisaligned);
  if (is_reduce(mode) && mode != INS_PLUS && !vals) return fail(t, KH_ERR_INVALID, "null values: only the std::plus reducer has a default value (1)");
  HIPCHK(hipSetDevice(t->device));
  const uint64_t np_ = std::min<uint64_t>(n, g_max_pass);
  { const uint64_t cu = capacity_after(t, t->cur.cap, t->lsize, np_ ? np_ : 1, np_, np_ ? np_ - 1 : 0);
    kh_status ps = arena_prepare(t, (where == KH_MEM_HOST ? n * 20 : 0) + kw_ws_insert(np_, cu));
    if (ps != KH_OK) return ps; }
  const uint64_t* kb = static_cast<const uint64_t*>(keys);
  const uint32_t* vb = static_cast<const uint32_t*>(vals);
  if (where == KH_MEM_HOST && n) {
    uint64_t* dk; TAKE(dk, uint64_t, 2 * n);
    HIPCHK(hipMemcpyAsync(dk, keys, n * 16, hipMemcpyHostToDevice, t->stream));
    kb = dk;
    if (vals) { uint32_t* dv; TAKE(dv, uint32_t, n); HIPCHK(hipMemcpyAsync(dv, vals, n * 4, hipMemcpyHostToDevice, t->stream)); vb = dv; }
  }
  return kw_insert_device(t, kb, vb, n, mode, n_inserted);
}

// find / count / find(Iter,Iter).  Outputs live where the queries live.
kh_status kw_do_find(kh_wtable* t, const void* keys, uint64_t n, kh_mem where, uint32_t* out_vals, uint8_t* out_found, uint64_t* out_ckeys,
                     uint32_t* out_cvals, bool compacted, bool count_only, uint64_t* n_found) {
  if (n_found) *n_found = 0;
  if (t->ins.active) return refuse_streaming(t);
  if (n == 0) return KH_OK;
  if (!keys) return fail(t, KH_ERR_INVALID, "null keys");
  if (!wide_keys_aligned(2, keys, where)) return fail(t, KH_ERR_INVALID, kWideKeysMisaligned);
  HIPCHK(hipSetDevice(t->device));
  { kh_status ps = arena_prepare(t, n * 48 + (n / KH_CMP_TILE + 8) * 16 + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  const uint64_t* q = static_cast<const uint64_t*>(keys);
  const bool host = where == KH_MEM_HOST;
  if (host) { uint64_t* d; TAKE(d, uint64_t, 2 * n); HIPCHK(hipMemcpyAsync(d, keys, n * 16, hipMemcpyHostToDevice, t->stream)); q = d; }
  unsigned long long* hits_dev; TAKE(hits_dev, unsigned long long, 1);
  HIPCHK(hipMemsetAsync(hits_dev, 0, 8, t->stream));
  uint32_t* dv = out_vals; uint8_t* df = out_found;
  if (compacted || (host && dv) || !dv) TAKE(dv, uint32_t, n);
  if (compacted || host || !df) TAKE(df, uint8_t, n);
  const int ncu = cu_count(t);
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + KW_Q_THREADS * KW_Q_ITEMS - 1) / (KW_Q_THREADS * KW_Q_ITEMS), (uint64_t)ncu * 8));
  { Launch L(t, count_only ? "kw_count" : "kw_find");
    if (count_only) { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((kw_find<HASH, KW_FIND_COUNT>), dim3(grid), dim3(KW_Q_THREADS), 0, t->stream, wide(t->cur), q, n, t->seed.s, dv, df, (unsigned long long*)nullptr)); }
    else { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((kw_find<HASH, KW_FIND_VALS>), dim3(grid), dim3(KW_Q_THREADS), 0, t->stream, wide(t->cur), q, n, t->seed.s, dv, df, hits_dev)); } }
  HIPCHK(hipGetLastError());
  if (count_only) {
    if (host) { HIPCHK(hipMemcpyAsync(out_found, df, n, hipMemcpyDeviceToHost, t->stream)); HIPCHK(hipStreamSynchronize(t->stream)); }
    return KH_OK;
  }
  uint64_t hits = 0;
  if (!compacted) {
    HIPCHK(hipMemcpyAsync(t->hpin, hits_dev, 8, hipMemcpyDeviceToHost, t->stream));
    if (host) { kh_status st = copy_hits_selective(t, dv, df, n, out_vals, out_found); if (st != KH_OK) return st; }
    else HIPCHK(hipStreamSynchronize(t->stream));
    hits = t->hpin[0];
  } else {
    uint64_t* ck = out_ckeys; uint32_t* cv = out_cvals;
    if (host) { TAKE(ck, uint64_t, 2 * n); TAKE(cv, uint32_t, n); }
    kh_status st = compact(t, df, q, dv, n, ck, cv, &hits);
    if (st == KH_OK && host && hits) st = copy_compacted(t, hits, ck, cv, out_ckeys, out_cvals);
    if (st != KH_OK) return st;
  }
  if (n_found) *n_found = hits;
  return KH_OK;
}

// erase(Iter,Iter): mark the hits, re-lay out without them (RH: never shrinks, hashmap_robinhood.hpp:1430-1440)
kh_status kw_do_erase(kh_wtable* t, const void* keys, uint64_t n, kh_mem where, uint64_t* n_erased) {
  *n_erased = 0;
  if (t->ins.active) return refuse_streaming(t);
  if (n == 0) return KH_OK;
  if (!keys) return fail(t, KH_ERR_INVALID, "null keys");
  if (!wide_keys_aligned(2, keys, where)) return fail(t, KH_ERR_INVALID, kWideKeysMisaligned);
  HIPCHK(hipSetDevice(t->device));
  { kh_status ps = arena_prepare(t, n * 16 + ws_rebuild(t->cur.cap) + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  const uint64_t* q = static_cast<const uint64_t*>(keys);
  if (where == KH_MEM_HOST) { uint64_t* d; TAKE(d, uint64_t, 2 * n); HIPCHK(hipMemcpyAsync(d, keys, n * 16, hipMemcpyHostToDevice, t->stream)); q = d; }
  unsigned long long* cnt;
  TAKE(cnt, unsigned long long, 1);
  HIPCHK(hipMemsetAsync(cnt, 0, 8, t->stream));
  { Launch L(t, "kw_erase_mark");
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((kw_erase_mark<HASH>), dim3(grid_for(n, 256, 2048)), dim3(256), 0, t->stream, wide(t->cur), q, n, t->seed.s, cnt)); }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t->hpin, cnt, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  const uint64_t ne = t->hpin[0];
  if (ne) {
    kh_status st = rebuild(t, t->cur.cap, nullptr, nullptr, nullptr, nullptr, 0, true, t->lsize - ne);
    if (st != KH_OK) {        // the table keeps its elements: take the marks back
      hipLaunchKernelGGL(kw_clear_marks, dim3(grid_for(t->cur.cap, 256)), dim3(256), 0, t->stream, wide(t->cur));
      hipStreamSynchronize(t->stream);
      return st;
    }
  }
  t->lsize -= ne;
  *n_erased = ne;
  return KH_OK;
}
}  // namespace

extern "C" {
kh_status kh_wide_create(kh_wtable** out, kh_kind kind, kh_hash hash, uint64_t seed, uint64_t capacity, float min_lf, float max_lf, int device) {
  if (!out) return KH_ERR_INVALID;
  *out = nullptr;
  if ((int)kind == KH_KIND_LINEARPROBE) return KH_ERR_UNSUPPORTED;
  if ((int)kind != KH_KIND_ROBINHOOD || (int)hash < 0 || (int)hash > 3) return KH_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return KH_ERR_HIP;
  if (device < 0 || device >= ndev) return KH_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess) return KH_ERR_HIP;
  kh_wtable* t = new kh_wtable();
  t->slot_bytes = sizeof(KwSlot);
  const kh_status st = table_init(t, KHK_RH, (int)hash, seed, capacity, min_lf, max_lf, device);
  if (st != KH_OK) { delete t; return st; }
  *out = t;
  return KH_OK;
}
kh_status kh_wide_destroy(kh_wtable* t) { table_release(t); delete t; return KH_OK; }
// state access: the 64-bit table's entry points, which read the width from the table
kh_status kh_wide_set_stream(kh_wtable* t, void* s) { return kh_set_stream(t, s); }
const char* kh_wide_last_error(const kh_wtable* t) { return kh_last_error(t); }
kh_status kh_wide_size(const kh_wtable* t, uint64_t* out) { return kh_size(t, out); }
kh_status kh_wide_capacity(const kh_wtable* t, uint64_t* out) { return kh_capacity(t, out); }
kh_status kh_wide_get_load_factors(const kh_wtable* t, float* mn, float* mx, float* cur) { return kh_get_load_factors(t, mn, mx, cur); }
kh_status kh_wide_set_min_load_factor(kh_wtable* t, float f) { return kh_set_min_load_factor(t, f); }
kh_status kh_wide_set_max_load_factor(kh_wtable* t, float f) { return kh_set_max_load_factor(t, f); }
kh_status kh_wide_clear(kh_wtable* t) { return kh_clear(t); }
kh_status kh_wide_reserve(kh_wtable* t, uint64_t n) { return kh_reserve(t, n); }
kh_status kh_wide_rehash(kh_wtable* t, uint64_t b) { return kh_rehash(t, b); }
kh_status kh_wide_to_vector(kh_wtable* t, uint64_t* keys_host, uint32_t* vals_host, uint64_t* n_out) { return kh_to_vector(t, keys_host, vals_host, n_out); }
kh_status kh_wide_export_info(kh_wtable* t, uint8_t* out_host) { return kh_export_info(t, out_host); }
kh_status kh_wide_displacement_histogram(kh_wtable* t, uint64_t out[128]) { return kh_displacement_histogram(t, out); }
kh_status kh_wide_value_histogram(kh_wtable* t, uint32_t nbins, uint64_t* out_host) { return kh_value_histogram(t, nbins, out_host); }
kh_status kh_wide_select_values(kh_wtable* t, uint32_t lo, uint32_t hi, kh_mem where, uint64_t* out_keys, uint32_t* out_vals, uint64_t cap_out, uint64_t* n_out) {
  return kh_select_values(t, lo, hi, where, out_keys, out_vals, cap_out, n_out);
}
kh_status kh_wide_erase_values(kh_wtable* t, uint32_t lo, uint32_t hi, uint64_t* n_erased) { return kh_erase_values(t, lo, hi, n_erased); }
kh_status kh_wide_insert(kh_wtable* t, const void* keys, const void* vals, uint64_t n, kh_mem where, uint64_t* n_inserted) {
  if (!t) return KH_ERR_INVALID;
  if (n && !vals) return fail(t, KH_ERR_INVALID, "null values");
  return kw_do_insert(t, keys, vals, n, where, INS_FIRST, n_inserted);
}
kh_status kh_wide_insert_reduce_plus(kh_wtable* t, const void* keys, const void* vals, uint64_t n, kh_mem where, uint64_t* n_inserted) {
  if (!t) return KH_ERR_INVALID;
  return kw_do_insert(t, keys, vals, n, where, INS_PLUS, n_inserted);
}
kh_status kh_wide_insert_reduce(kh_wtable* t, const void* keys, const void* vals, uint64_t n, kh_mem where, kh_reduce_op op, uint64_t* n_inserted) {
  if (!t) return KH_ERR_INVALID;
  if (n_inserted) *n_inserted = 0;
  if ((unsigned)op > (unsigned)KH_REDUCE_OR) return fail(t, KH_ERR_INVALID, "unknown reduce operation");
  return kw_do_insert(t, keys, vals, n, where, INS_PLUS + (int)op, n_inserted);
}
kh_status kh_wide_count(kh_wtable* t, const void* keys, uint64_t n, kh_mem where, uint8_t* out01) {
  if (!t) return KH_ERR_INVALID;
  if (n && !out01) return fail(t, KH_ERR_INVALID, "null argument");
  return kw_do_find(t, keys, n, where, nullptr, out01, nullptr, nullptr, false, true, nullptr);
}
kh_status kh_wide_find(kh_wtable* t, const void* keys, uint64_t n, kh_mem where, uint32_t* out_vals, uint8_t* out_found, uint64_t* n_found) {
  if (!t) return KH_ERR_INVALID;
  return kw_do_find(t, keys, n, where, out_vals, out_found, nullptr, nullptr, false, false, n_found);
}
kh_status kh_wide_find_compact(kh_wtable* t, const void* keys, uint64_t n, kh_mem where, uint64_t* out_keys, uint32_t* out_vals, uint64_t* n_found) {
  if (!t) return KH_ERR_INVALID;
  if (n && (!out_keys || !out_vals)) return fail(t, KH_ERR_INVALID, "null output");
  return kw_do_find(t, keys, n, where, nullptr, nullptr, out_keys, out_vals, true, false, n_found);
}
kh_status kh_wide_erase(kh_wtable* t, const void* keys, uint64_t n, kh_mem where, uint64_t* n_erased) {
  if (!t) return KH_ERR_INVALID;
  uint64_t ne = 0;
  kh_status st = kw_do_erase(t, keys, n, where, &ne);
  if (n_erased) *n_erased = ne;
  if (st == KH_OK && t->lsize < t->min_load) st = do_reserve(t, t->lsize);     // hashmap_robinhood.hpp:1437: reserve() only grows
  return st;
}
// ---- streamed insert of a wide table: the contract of kh_insert_begin / feed / end.  A feed queues the COUNTING half of the partition
//      on its piece (kw_part_count into counters all pieces share) and remembers the piece; kh_wide_insert_end scans the counters
//      and scatters every piece with its base added to the stream positions -- from there on it is kw_insert_core.  The partition is
//      exact (count, scan, scatter), so KH_INS_REPEATABLE buys nothing here and KH_ERR_RETRY is never returned.  Batches without a
//      one-pass form (n_total == 0, more than g_max_pass keys, more than one doubling pending, more than 2^22 partitions) are
//      collected in workspace and inserted by the general entry point at the end.
kh_status kh_wide_insert_begin_ex(kh_wtable* t, uint64_t n_total, unsigned flags) {
  if (!t) return KH_ERR_INVALID;
  if (t->ins.active) return fail(t, KH_ERR_INVALID, "a streamed insert is already in progress");
  if (!ins_flags_ok(flags)) return fail(t, KH_ERR_INVALID, "unknown flag");
  HIPCHK(hipSetDevice(t->device));
  memset(&t->ins, 0, sizeof(t->ins));
  t->ins.mode = ins_flags_mode(flags);
  t->ins.n_total = n_total;
  const uint64_t np_ = std::min<uint64_t>(n_total, g_max_pass);
  const uint64_t cu = capacity_after(t, t->cur.cap, t->lsize, np_ ? np_ : 1, np_, np_ ? np_ - 1 : 0);
  const uint32_t PB = cu > KH_L ? log2u(cu >> KH_LB) : 0u;
  t->ins.fallback = n_total == 0 || n_total > g_max_pass || PB > 22 || t->lsize >= threshold(t->cur.cap << 1, t->max_lf);
  t->ins.cap_u = cu; t->ins.PB = PB;
  // (n_total * 20: the collected batch of the fall-back, or host pieces copied in; device pieces of the one-pass form take nothing)
  { kh_status ps = arena_prepare(t, n_total * 20 + kw_ws_insert(np_, cu) + KH_MAX_SRC * 512); if (ps != KH_OK) return ps; }
  if (n_total) {
    if (t->ins.fallback) { TAKE(t->ins.stage_k, uint64_t, 2 * n_total); TAKE(t->ins.stage_v, uint32_t, n_total); }
    else {
      const uint32_t nparts = 1u << PB;
      TAKE(t->ins.wcnt, uint32_t, nparts);
      HIPCHK(hipMemsetAsync(t->ins.wcnt, 0, sizeof(uint32_t) * nparts, t->stream));
    }
  }
  t->ins.active = true;
  return KH_OK;
}
kh_status kh_wide_insert_feed(kh_wtable* t, const void* keys, const void* vals, uint64_t n, kh_mem where) {
  if (!t) return KH_ERR_INVALID;
  if (!t->ins.active) return fail(t, KH_ERR_INVALID, "kh_wide_insert_feed without kh_wide_insert_begin_ex");
  if (n == 0) return KH_OK;
  if (!keys) return fail(t, KH_ERR_INVALID, "null keys");
  if (!wide_keys_aligned(2, keys, where)) return fail(t, KH_ERR_INVALID, kWideKeysMisaligned);      // (the streamed insert stays open, nothing was fed)
  if (!vals && t->ins.mode != INS_PLUS) return fail(t, KH_ERR_INVALID, "null values");
  if (t->ins.fed + n > t->ins.n_total) return fail(t, KH_ERR_INVALID, "more pairs fed than announced to kh_wide_insert_begin_ex");
  if (t->ins.wsrc == KH_MAX_SRC) return fail(t, KH_ERR_UNSUPPORTED, "more than 16 feeds in one streamed insert");     // (either form: the limit does not depend on table state)
  HIPCHK(hipSetDevice(t->device));
  const hipMemcpyKind kind = where == KH_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  if (t->ins.fallback) {
    HIPCHK(hipMemcpyAsync(t->ins.stage_k + 2 * t->ins.fed, keys, n * 16, kind, t->stream));
    if (vals) HIPCHK(hipMemcpyAsync(t->ins.stage_v + t->ins.fed, vals, n * 4, kind, t->stream));
    else HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(t->ins.stage_v + t->ins.fed), 1, n, t->stream));
    ++t->ins.wsrc;
  } else {
    const uint64_t* dk = static_cast<const uint64_t*>(keys);
    const uint32_t* dv = static_cast<const uint32_t*>(vals);
    if (where == KH_MEM_HOST) {
      uint64_t* ck; TAKE(ck, uint64_t, 2 * n);
      HIPCHK(hipMemcpyAsync(ck, keys, n * 16, hipMemcpyHostToDevice, t->stream));
      dk = ck;
      if (vals) { uint32_t* cv; TAKE(cv, uint32_t, n); HIPCHK(hipMemcpyAsync(cv, vals, n * 4, hipMemcpyHostToDevice, t->stream)); dv = cv; }
    }
    kh_status st = kw_count_source(t, dk, n, t->ins.PB, t->ins.wcnt);
    if (st != KH_OK) return st;
    HIPCHK(hipGetLastError());
    const uint32_t s = t->ins.wsrc++;
    t->ins.wk[s] = dk; t->ins.wv[s] = dv; t->ins.wn[s] = n;
  }
  t->ins.fed += n;
  if (where == KH_MEM_HOST) HIPCHK(hipStreamSynchronize(t->stream));   // host buffers may be reused as soon as the feed returns
  return KH_OK;
}
kh_status kh_wide_insert_end(kh_wtable* t, uint64_t* n_inserted) {
  if (n_inserted) *n_inserted = 0;
  if (!t) return KH_ERR_INVALID;
  if (!t->ins.active) return fail(t, KH_ERR_INVALID, "kh_wide_insert_end without kh_wide_insert_begin_ex");
  t->ins.active = false;
  HIPCHK(hipSetDevice(t->device));
  if (t->ins.fed != t->ins.n_total) {
    hipStreamSynchronize(t->stream);      // (queued counts may still read the caller's pieces)
    return fail(t, KH_ERR_INVALID, "fewer pairs fed than announced to kh_wide_insert_begin_ex");
  }
  const uint64_t n = t->ins.n_total;
  if (t->ins.fallback) return kw_insert_device(t, t->ins.stage_k, t->ins.stage_v, n, t->ins.mode, n_inserted);
  KwSrc src[KH_MAX_SRC];
  for (uint32_t s = 0; s < t->ins.wsrc; ++s) { src[s].k = t->ins.wk[s]; src[s].v = t->ins.wv[s]; src[s].n = t->ins.wn[s]; }
  uint64_t nn = 0;
  kh_status st = kw_insert_core(t, src, t->ins.wsrc, n, t->ins.mode, 0, &nn, t->ins.wcnt);
  if (st == KH_OK) st = do_reserve(t, t->lsize);
  if (st == KH_OK) HIPCHK(hipStreamSynchronize(t->stream));
  else hipStreamSynchronize(t->stream);
  if (n_inserted) *n_inserted = nn;
  return st;
}
kh_status kh_wide_insert_abort(kh_wtable* t) { return kh_insert_abort(t); }

// stable partition of 16-byte keys by destination rank (kh_shard_permute for wide keys)
kh_status kh_wide_shard_permute(kh_hash hash, uint64_t seed, uint32_t p, const uint64_t* keys, const uint32_t* vals, uint64_t n,
                                uint64_t* out_keys, uint32_t* out_vals, uint64_t* counts_host, int device, void* stream_) {
  return shard_permute_impl(2, hash, seed, KH_XF_IDENTITY, 0, p, keys, vals, n, out_keys, out_vals, counts_host, device, stream_);
}
kh_status kh_wide_hash_batch(kh_hash hash, uint64_t seed, const void* keys, uint64_t n, kh_mem where, uint64_t* out, int device, void* stream) {
  return hash_batch_impl(2, hash, KhSeed{seed, 0u}, keys, n, where, out, device, stream);
}
kh_status kh_kmers128_from_sequence(const void* seq, uint64_t n, uint32_t k, int canonical, kh_mem where, uint64_t* out_kmers, uint64_t* n_out,
                                    int device, void* stream) {
  return kmers_impl(2, seq, n, k, canonical, where, false, out_kmers, n_out, device, stream);
}
kh_status kh_kmers128_from_fastq(const void* text, uint64_t n, uint32_t k, int canonical, kh_mem where, uint64_t* out_kmers, uint64_t* n_out,
                                 int device, void* stream) {
  return kmers_impl(2, text, n, k, canonical, where, true, out_kmers, n_out, device, stream);
}
// 16-byte k-mers with the byte offset of their window (kh_kmers_from_sequence_pos / _fastq_pos for k = 1..64)
kh_status kh_kmers128_from_sequence_pos(const void* seq, uint64_t n, uint32_t k, int canonical, kh_mem where,
                                        uint64_t* out_kmers, uint32_t* out_pos, uint64_t* n_out, int device, void* stream) {
  if (n_out) *n_out = 0;
  if (n >> 32) return KH_ERR_INVALID;
  if (n >= k && !out_pos) return KH_ERR_INVALID;
  return kmers_impl(2, seq, n, k, canonical, where, false, out_kmers, n_out, device, stream, out_pos);
}
kh_status kh_kmers128_from_fastq_pos(const void* text, uint64_t n, uint32_t k, int canonical, kh_mem where,
                                     uint64_t* out_kmers, uint32_t* out_pos, uint64_t* n_out, int device, void* stream) {
  if (n_out) *n_out = 0;
  if (n >> 32) return KH_ERR_INVALID;
  if (n >= k && !out_pos) return KH_ERR_INVALID;
  return kmers_impl(2, text, n, k, canonical, where, true, out_kmers, n_out, device, stream, out_pos);
}
}  // extern "C"

// ===================================================================================================
// k-mer position index (kh_index): all occurrences per k-mer.  The reference's driver offers PositionIndex<MapType> over a multimap next
// to CountIndex (BenchmarkKmerIndex.cpp:342-449); the multimap itself is kmerind's and not part of the reference tree, so the contract is
// this library's (include/kmerhash_amd.h).  A static index: one Robin Hood kh_table owned by the index, whose value per key is the key's
// rank among the live slots in slot order, and a CSR (offsets u32[size + 1], positions u32[total]) in device memory.
// ===================================================================================================
struct kh_index {
  kh_table* t = nullptr;
  uint32_t kw = 1;                    // 64-bit words per key: 1 (kh_index_*), 2 (kh_wide_index_*: the table is a kh_wtable)
  int hash = 0, device = 0;
  uint64_t seed = 0;
  float min_lf = 0.f, max_lf = 0.f;
  hipStream_t stream = nullptr;
  uint32_t* offsets = nullptr;        // u32[size + 1]
  uint32_t* positions = nullptr;      // u32[total]
  uint64_t total = 0;
  bool built = false, prof = false;
  bool stranded = false;              // kh_index_set_stranded: the text forms store ((pos_base + p) << 1) | rc(p); survives clear and a failed build
  std::string err;
};
struct kh_windex : kh_index {};      // a distinct handle type for the C header; the host state is kh_index's, the kernels that touch a slot differ
namespace {
// the index's table: fresh, capacity 128, of the index's key width
kh_status index_table_create(kh_index* x) {
  if (x->kw == 2) {
    kh_wtable* w = nullptr;
    const kh_status st = kh_wide_create(&w, KH_KIND_ROBINHOOD, (kh_hash)x->hash, x->seed, 128, x->min_lf, x->max_lf, x->device);
    x->t = w;
    return st;
  }
  return kh_create(&x->t, KH_KIND_ROBINHOOD, 8, 4, (kh_hash)x->hash, x->seed, 128, x->min_lf, x->max_lf, x->device);
}
kh_status xfail(kh_index* x, kh_status s, const std::string& msg) { if (x) x->err = msg; return s; }
// back to the state of kh_index_create: no arrays and a FRESH table (a cleared table would keep its capacity, and the layout of the next
// build is promised to be that of a fresh table)
kh_status index_reset(kh_index* x) {
  hipSetDevice(x->device);
  if (x->t) hipStreamSynchronize(x->t->stream);
  pool_free(x->device, x->offsets); pool_free(x->device, x->positions);
  x->offsets = nullptr; x->positions = nullptr; x->total = 0; x->built = false;
  if (x->t) { kh_destroy(x->t); x->t = nullptr; }
  const kh_status st = index_table_create(x);
  if (st != KH_OK) return xfail(x, st, "kh_index: the table could not be created");
  x->t->stream = x->stream; x->t->prof = x->prof;
  return KH_OK;
}
// a failed build leaves the index empty; the text of the failure survives the reset
kh_status index_abandon(kh_index* x, kh_status s) {
  const std::string msg = x->t ? x->t->err : std::string("kh_index: no table");
  index_reset(x);
  return xfail(x, s, msg);
}
inline uint32_t index_probe_grid(const kh_table* t, uint64_t n) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + KI_Q_TILE - 1) / KI_Q_TILE, (uint64_t)cu_count(t) * 8));
}
static_assert(KW_INDEX_Q_TILE == KI_Q_TILE, "one probe grid for both key widths");
// the kernels that read value and info only, on the slot layout of the index's key width (the index's table is always Robin Hood)
#define KI_SWITCH_LAYOUT(x, ...)                                                       \
  if ((x)->kw == 2) { constexpr int LAY = KV_WIDE; __VA_ARGS__; }                      \
  else { constexpr int LAY = KV_RH; __VA_ARGS__; }
// (begin, count) per query: the lookup kernel of the index's key width
void index_launch_lookup(kh_index* x, const uint64_t* q, uint64_t n, uint32_t* begin, uint32_t* cnt) {
  kh_table* t = x->t;
  Launch L(t, x->kw == 2 ? "kw_index_lookup" : "k_index_lookup");
  if (x->kw == 2) {
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((kw_index_lookup<HASH>), dim3(index_probe_grid(t, n)), dim3(KW_Q_THREADS), 0, t->stream, wide(t->cur), q, n, t->seed.s,
                                               (const uint32_t*)x->offsets, (uint64_t)t->lsize, begin, cnt));
  } else {
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_index_lookup<HASH>), dim3(index_probe_grid(t, n)), dim3(KH_Q_THREADS), 0, t->stream, narrow(t->cur), q, n, t->seed,
                                               (const uint32_t*)x->offsets, begin, cnt));
  }
}
// exclusive scan of n (> 0) device counts into n + 1 offsets of type OUT; ssums: ull[tiles + 1] of workspace
// (ssums[tiles] is left holding the total)
template <typename OUT>
void scan_counts(hipStream_t stream, const uint32_t* counts, uint64_t n, unsigned long long* ssums, OUT* out) {
  const uint64_t nst = (n + KI_SCAN_TILE - 1) / KI_SCAN_TILE;
  hipLaunchKernelGGL(k_index_tile_sums, dim3((uint32_t)nst), dim3(KI_SCAN_THREADS), 0, stream, counts, n, ssums);
  hipLaunchKernelGGL(k_index_scan_sums, dim3(1), dim3(KI_SUMS_THREADS), 0, stream, ssums, nst);
  hipLaunchKernelGGL((k_index_scan_apply<OUT>), dim3((uint32_t)nst), dim3(KI_SCAN_THREADS), 0, stream, counts, n, (const unsigned long long*)ssums, out);
}
template <typename OUT>
kh_status index_scan(kh_table* t, const uint32_t* counts, uint64_t n, unsigned long long* ssums, OUT* out) {
  Launch L(t, "k_index_scan");
  scan_counts(t->stream, counts, n, ssums, out);
  HIPCHK(hipGetLastError());
  return KH_OK;
}
// the build proper: n (> 0) pairs in device memory, the index empty.  On an error the caller abandons the index.
kh_status index_build_device(kh_index* x, const uint64_t* dk, const uint32_t* dp, uint64_t n) {
  kh_table* t = x->t;
  // 1. the counting insert, unchanged: key set, size, capacity and slot order are those of kh_insert_reduce_plus into a fresh table
  uint64_t nins = 0;
  kh_status st = x->kw == 2 ? kh_wide_insert_reduce_plus(static_cast<kh_wtable*>(t), dk, nullptr, n, KH_MEM_DEVICE, &nins)
                             : kh_insert_reduce_plus(t, dk, nullptr, n, KH_MEM_DEVICE, &nins);
  if (st != KH_OK) return st;
  const uint64_t size = t->lsize, cap = t->cur.cap;
  if (size == 0 || size > n) return fail(t, KH_ERR_HIP, "kh_index: internal: counting insert left an impossible size");
  void* vp = nullptr;
  HIPCHK(pool_alloc(t->device, (size + 1) * 4, &vp)); x->offsets = static_cast<uint32_t*>(vp);
  HIPCHK(pool_alloc(t->device, n * 4, &vp)); x->positions = static_cast<uint32_t*>(vp);
  const uint64_t ntl = (cap + KV_SEL_TILE - 1) / KV_SEL_TILE, nst = (size + KI_SCAN_TILE - 1) / KI_SCAN_TILE, nsort = (n + KI_SORT_TILE - 1) / KI_SORT_TILE;
  { kh_status ps = arena_prepare(t, ntl * 12 + size * 8 + nst * 8 + nsort * 4 + n * 4 + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  uint32_t *sums, *counts, *cursor, *xlist, *xcount, *scratch; uint64_t* toffs; unsigned long long* ssums;
  TAKE(sums, uint32_t, ntl); TAKE(toffs, uint64_t, ntl + 1); TAKE(counts, uint32_t, size); TAKE(cursor, uint32_t, size);
  TAKE(ssums, unsigned long long, nst + 1); TAKE(xlist, uint32_t, nsort); TAKE(xcount, uint32_t, 1); TAKE(scratch, uint32_t, n);
  // 2. the keys that share a home bucket in key order (the insert leaves their order to chance); rank of every live slot in slot order; counts[rank] = occurrences; the slot's value becomes the rank; offsets = scan(counts)
  if (x->kw == 2) {
    Launch L(t, "kw_index_rank");
    hipLaunchKernelGGL(kw_index_canon_runs, dim3(grid_for(cap, 256, (uint32_t)cu_count(t) * 8)), dim3(256), 0, t->stream, wide(t->cur).s, cap);
    hipLaunchKernelGGL((k_values_tile_count<KV_WIDE>), dim3((uint32_t)ntl), dim3(KV_SEL_THREADS), 0, t->stream, (const void*)t->cur.p, cap, 0u, 0xFFFFFFFFu, sums);
    hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, t->stream, (const uint32_t*)sums, ntl, toffs);
    hipLaunchKernelGGL(kw_index_rank, dim3((uint32_t)ntl), dim3(KV_SEL_THREADS), 0, t->stream, wide(t->cur).s, cap, (const uint64_t*)toffs, counts);
  } else {
    Launch L(t, "k_index_rank");
    hipLaunchKernelGGL(k_index_canon_runs, dim3(grid_for(cap, 256, (uint32_t)cu_count(t) * 8)), dim3(256), 0, t->stream, narrow(t->cur).s, cap);
    hipLaunchKernelGGL((k_values_tile_count<KV_RH>), dim3((uint32_t)ntl), dim3(KV_SEL_THREADS), 0, t->stream, (const void*)t->cur.p, cap, 0u, 0xFFFFFFFFu, sums);
    hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, t->stream, (const uint32_t*)sums, ntl, toffs);
    hipLaunchKernelGGL(k_index_rank, dim3((uint32_t)ntl), dim3(KV_SEL_THREADS), 0, t->stream, narrow(t->cur).s, cap, (const uint64_t*)toffs, counts); }
  HIPCHK(hipGetLastError());
  st = index_scan<uint32_t>(t, counts, size, ssums, x->offsets);
  if (st != KH_OK) return st;
  // 3. scatter through per-key cursors
  HIPCHK(hipMemcpyAsync(cursor, x->offsets, size * 4, hipMemcpyDeviceToDevice, t->stream));
  HIPCHK(hipMemsetAsync(xcount, 0, 4, t->stream));
  if (x->kw == 2) {
    Launch L(t, "kw_index_scatter");
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((kw_index_scatter<HASH>), dim3(index_probe_grid(t, n)), dim3(KW_Q_THREADS), 0, t->stream, wide(t->cur), dk, dp, n, t->seed.s,
                                               cursor, x->positions, n, size));
  } else {
    Launch L(t, "k_index_scatter");
    KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_index_scatter<HASH>), dim3(index_probe_grid(t, n)), dim3(KH_Q_THREADS), 0, t->stream, narrow(t->cur), dk, dp, n, t->seed,
                                               cursor, x->positions, n)); }
  HIPCHK(hipGetLastError());
  // 4. ascending order inside every segment: fixed tiles in LDS, then the segments that cross a tile boundary
  { Launch L(t, "k_index_tile_sort");
    hipLaunchKernelGGL(k_index_tile_sort, dim3((uint32_t)nsort), dim3(KI_SORT_THREADS), 0, t->stream, x->positions, n, (const uint32_t*)x->offsets, size, xlist, xcount); }
  { Launch L(t, "k_index_seg_radix");
    hipLaunchKernelGGL(k_index_seg_radix, dim3((uint32_t)std::min<uint64_t>(nsort, (uint64_t)cu_count(t) * 4)), dim3(KI_RADIX_THREADS), 0, t->stream, x->positions, scratch,
                       (const uint32_t*)x->offsets, (const uint32_t*)xlist, (const uint32_t*)xcount); }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(t->stream));
  x->total = n; x->built = true;
  return KH_OK;
}
// ---- mutation: the CSR carried across a change of the key set (kernels: the last section of kh_kernels_index.h) ----
// The table has been changed by its own insert or erase; every live slot holds old rank + bias (bias 1: stamped before an insert, 0 is a
// key the batch brought; bias 0: after an erase, which keeps the survivors' values).  New ranks, new offsets, the old segments moved to
// the front of the new ones, then -- append only -- the nb pairs (dk, dp) scattered behind them and every segment sorted again.  The new
// arrays come back through noff / npos; the caller swaps them in or frees them.
kh_status index_carry_arrays(kh_index* x, uint32_t bias, uint64_t old_size, const uint64_t* dk, const uint32_t* dp, uint64_t nb, uint32_t** noff, uint32_t** npos,
                             uint64_t* ntotal) {
  kh_table* t = x->t;
  const uint64_t size = t->lsize, cap = t->cur.cap, old_total = x->total, bound = old_total + nb;
  const uint64_t ntl = (cap + KV_SEL_TILE - 1) / KV_SEL_TILE, nst = (size + KI_SCAN_TILE - 1) / KI_SCAN_TILE, nsort = (bound + KI_SORT_TILE - 1) / KI_SORT_TILE;
  { kh_status ps = arena_prepare(t, ntl * 12 + size * 12 + nst * 8 + (nb ? nsort * 4 + bound * 4 : 0) + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  uint32_t *sums, *counts, *oldrank, *cursor = nullptr, *xlist = nullptr, *xcount = nullptr, *scratch = nullptr; uint64_t* toffs; unsigned long long* ssums;
  TAKE(sums, uint32_t, ntl); TAKE(toffs, uint64_t, ntl + 1); TAKE(counts, uint32_t, size); TAKE(oldrank, uint32_t, size); TAKE(ssums, unsigned long long, nst + 1);
  if (nb) { TAKE(cursor, uint32_t, size); TAKE(xlist, uint32_t, nsort); TAKE(xcount, uint32_t, 1); TAKE(scratch, uint32_t, bound); }
  void* vp = nullptr;
  HIPCHK(pool_alloc(t->device, (size + 1) * 4, &vp)); *noff = static_cast<uint32_t*>(vp);
  // keys of one home bucket in key order again (an insert or a re-layout leaves their order to chance), new rank into every live slot,
  // counts[new rank] = the length of the key's old segment
  { Launch L(t, "k_index_rank_carry");
    if (x->kw == 2) hipLaunchKernelGGL(kw_index_canon_runs, dim3(grid_for(cap, 256, (uint32_t)cu_count(t) * 8)), dim3(256), 0, t->stream, wide(t->cur).s, cap);
    else hipLaunchKernelGGL(k_index_canon_runs, dim3(grid_for(cap, 256, (uint32_t)cu_count(t) * 8)), dim3(256), 0, t->stream, narrow(t->cur).s, cap);
    KI_SWITCH_LAYOUT(x, hipLaunchKernelGGL((k_values_tile_count<LAY>), dim3((uint32_t)ntl), dim3(KV_SEL_THREADS), 0, t->stream, (const void*)t->cur.p, cap, 0u, 0xFFFFFFFFu, sums));
    hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, t->stream, (const uint32_t*)sums, ntl, toffs);
    KI_SWITCH_LAYOUT(x, hipLaunchKernelGGL((k_index_rank_carry<LAY>), dim3((uint32_t)ntl), dim3(KV_SEL_THREADS), 0, t->stream, t->cur.p, cap, (const uint64_t*)toffs,
                                           (const uint32_t*)x->offsets, old_size, bias, size, counts, oldrank)); }
  HIPCHK(hipGetLastError());
  if (nb) {      // the batch on top: the random touches of the scatter, once more
    Launch L(t, x->kw == 2 ? "kw_index_count_pairs" : "k_index_count_pairs");
    if (x->kw == 2) { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((kw_index_count_pairs<HASH>), dim3(index_probe_grid(t, nb)), dim3(KW_Q_THREADS), 0, t->stream, wide(t->cur), dk, nb,
                                                                 t->seed.s, counts, size)); }
    else { KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_index_count_pairs<HASH>), dim3(index_probe_grid(t, nb)), dim3(KH_Q_THREADS), 0, t->stream, narrow(t->cur), dk, nb, t->seed,
                                                      counts, size)); }
  }
  HIPCHK(hipGetLastError());
  kh_status st = index_scan<uint32_t>(t, counts, size, ssums, *noff);
  if (st != KH_OK) return st;
  HIPCHK(hipMemcpyAsync(t->hpin, *noff + size, 4, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  const uint64_t total = *reinterpret_cast<const uint32_t*>(t->hpin);
  if (total == 0 || total > bound || (nb && total != bound)) return fail(t, KH_ERR_HIP, "kh_index: internal: the carried counts do not add up");
  HIPCHK(pool_alloc(t->device, total * 4, &vp)); *npos = static_cast<uint32_t*>(vp);
  { Launch L(t, "k_index_move");
    hipLaunchKernelGGL(k_index_move, dim3(grid_for(total, 256, (uint32_t)cu_count(t) * 8)), dim3(256), 0, t->stream, (const uint32_t*)x->positions, (const uint32_t*)x->offsets,
                       old_size, old_total, (const uint32_t*)*noff, (const uint32_t*)oldrank, size, total, *npos, cursor); }
  HIPCHK(hipGetLastError());
  if (nb) {
    HIPCHK(hipMemsetAsync(xcount, 0, 4, t->stream));
    if (x->kw == 2) {
      Launch L(t, "kw_index_scatter");
      KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((kw_index_scatter<HASH>), dim3(index_probe_grid(t, nb)), dim3(KW_Q_THREADS), 0, t->stream, wide(t->cur), dk, dp, nb, t->seed.s,
                                                 cursor, *npos, total, size));
    } else {
      Launch L(t, "k_index_scatter");
      KH_SWITCH_HASH(t->hash, hipLaunchKernelGGL((k_index_scatter<HASH>), dim3(index_probe_grid(t, nb)), dim3(KH_Q_THREADS), 0, t->stream, narrow(t->cur), dk, dp, nb, t->seed,
                                                 cursor, *npos, total)); }
    HIPCHK(hipGetLastError());
    // ascending order again: the whole array (sorting only the segments that grew is an open end)
    { Launch L(t, "k_index_tile_sort");
      hipLaunchKernelGGL(k_index_tile_sort, dim3((uint32_t)nsort), dim3(KI_SORT_THREADS), 0, t->stream, *npos, total, (const uint32_t*)*noff, size, xlist, xcount); }
    { Launch L(t, "k_index_seg_radix");
      hipLaunchKernelGGL(k_index_seg_radix, dim3((uint32_t)std::min<uint64_t>(nsort, (uint64_t)cu_count(t) * 4)), dim3(KI_RADIX_THREADS), 0, t->stream, *npos, scratch,
                         (const uint32_t*)*noff, (const uint32_t*)xlist, (const uint32_t*)xcount); }
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(t->stream));
  *ntotal = total;
  return KH_OK;
}
kh_status index_carry(kh_index* x, uint32_t bias, uint64_t old_size, const uint64_t* dk, const uint32_t* dp, uint64_t nb) {
  kh_table* t = x->t;
  uint32_t *noff = nullptr, *npos = nullptr; uint64_t total = 0;
  kh_status st = KH_OK;
  if (t->lsize) st = index_carry_arrays(x, bias, old_size, dk, dp, nb, &noff, &npos, &total);      // (nothing left: an empty index on the table as the erase left it)
  hipStreamSynchronize(t->stream);
  if (st != KH_OK) { pool_free(x->device, noff); pool_free(x->device, npos); return st; }
  pool_free(x->device, x->offsets); pool_free(x->device, x->positions);
  x->offsets = noff; x->positions = npos; x->total = total; x->built = total != 0;
  return KH_OK;
}
// n (> 0) pairs in device memory onto an index in any state.  On an error the caller abandons the index.
kh_status index_append_device(kh_index* x, const uint64_t* dk, const uint32_t* dp, uint64_t n) {
  if (!x->built) return index_build_device(x, dk, dp, n);      // the build itself: the same kernels, the same bytes
  kh_table* t = x->t;
  const uint64_t old_size = t->lsize;
  { Launch L(t, "k_index_stamp");
    KI_SWITCH_LAYOUT(x, hipLaunchKernelGGL((k_index_stamp<LAY>), dim3(grid_for(t->cur.cap, KV_MARK_THREADS * KV_MARK_ITEMS, (uint32_t)cu_count(t) * 8)), dim3(KV_MARK_THREADS), 0,
                                           t->stream, t->cur.p, t->cur.cap)); }
  HIPCHK(hipGetLastError());
  // the table's own reducer insert with zero values: key set, size, capacity and layout of kh_insert_reduce_plus; stamp | 0 = stamp
  void* zeros = nullptr;      // (not in the table's workspace: the insert resets it)
  HIPCHK(pool_alloc(x->device, n * 4, &zeros));
  kh_status st = KH_ERR_HIP;
  if (hipMemsetAsync(zeros, 0, n * 4, t->stream) != hipSuccess) fail(t, KH_ERR_HIP, "kh_index_append: clearing the values failed");
  else {
    uint64_t nins = 0;
    st = x->kw == 2 ? kh_wide_insert_reduce(static_cast<kh_wtable*>(t), dk, zeros, n, KH_MEM_DEVICE, KH_REDUCE_OR, &nins)
                    : kh_insert_reduce(t, dk, zeros, n, KH_MEM_DEVICE, KH_REDUCE_OR, &nins);
  }
  hipStreamSynchronize(t->stream);
  pool_free(x->device, zeros);
  if (st != KH_OK) return st;
  if (t->lsize < old_size || t->lsize > old_size + n) return fail(t, KH_ERR_HIP, "kh_index: internal: the insert left an impossible size");
  return index_carry(x, 1u, old_size, dk, dp, n);
}
// (key, position) pairs of a build or an append: host pairs are staged once
kh_status index_pairs(kh_index* x, const void* keys, const void* pos, uint64_t n, kh_mem where, bool append) {
  if (!x) return KH_ERR_INVALID;
  if (n >> 32) return xfail(x, KH_ERR_INVALID, "kh_index_build: positions and offsets are 32-bit, n must be below 2^32");
  if (!append && x->built) return xfail(x, KH_ERR_INVALID, "kh_index_build: the index is built already (kh_index_clear first)");
  if (append && (x->total + n) >> 32) return xfail(x, KH_ERR_INVALID, "kh_index_append: offsets are 32-bit, the index must stay below 2^32 positions");
  if (n == 0) return KH_OK;
  if (!keys || !pos) return xfail(x, KH_ERR_INVALID, "null argument");
  if (!wide_keys_aligned(x->kw, keys, where)) return xfail(x, KH_ERR_INVALID, kWideKeysMisaligned);
  kh_table* t = x->t;
  HIPCHK(hipSetDevice(x->device));
  Scratch s(x->device, t->stream);      // (host pairs: not in the table's workspace, the counting insert resets it)
  const uint64_t* dk = nullptr; const uint32_t* dp = nullptr;
  s.layout([&](Scratch& c) { dk = c.in(static_cast<const uint64_t*>(keys), n * x->kw, where); dp = c.in(static_cast<const uint32_t*>(pos), n, where); });
  if (!s.ok()) { const hipError_t e = s.error(); s.finish(); return hip_fail(t, "kh_index_build: staging the pairs", e); }      // (the index is untouched)
  const kh_status st = append ? index_append_device(x, dk, dp, n) : index_build_device(x, dk, dp, n);
  s.sync();
  s.finish();
  return st == KH_OK ? KH_OK : index_abandon(x, st);
}
// what a stranded index refuses before it is touched: the strand is that of the canonical choice, and a stamped position has 31 bits
kh_status index_stranded_args(kh_index* x, uint64_t n, int canonical, uint32_t pos_base) {
  if (!canonical) return xfail(x, KH_ERR_INVALID, "kh_index: a stranded index holds canonical k-mers (the strand bit says which strand the canonical form came from)");
  if (n >> 31) return xfail(x, KH_ERR_INVALID, "kh_index: stamped positions are 31-bit, a text of 2^31 bytes or more is refused on a stranded index");
  if ((uint64_t)pos_base + n > (uint64_t(1) << 31)) return xfail(x, KH_ERR_INVALID, "kh_index: pos_base + n passes 2^31 on a stranded index");
  return KH_OK;
}
// the stamp of a stranded index: m window positions (pos_base 0, as the front end emitted them) over the device text they came from
// become ((pos_base + p) << 1) | rc(p) in place; it takes the place of k_index_add_base and of the emit pass's base
kh_status index_stamp(kh_index* x, const void* dtext, uint64_t n, uint32_t k, uint32_t* dp, uint64_t m, uint32_t pos_base) {
  kh_table* t = x->t;
  Launch L(t, "k_pos_strand");
  hipLaunchKernelGGL((k_pos_strand<false>), dim3(grid_for(m, 256, (uint32_t)cu_count(t) * 8)), dim3(256), 0, t->stream, static_cast<const uint8_t*>(dtext), n, k,
                     (const uint32_t*)dp, m, pos_base, dp, (unsigned long long*)nullptr);
  if (hipGetLastError() != hipSuccess) return fail(t, KH_ERR_HIP, "kh_index: k_pos_strand failed");
  return KH_OK;
}
// build or append straight from text: the position-keeping k-mer front end on device buffers; an append adds pos_base to every window
// position (several texts in one coordinate space)
kh_status index_text(kh_index* x, const void* text, uint64_t n, uint32_t k, int canonical, kh_mem where, bool fastq, bool append, uint32_t pos_base) {
  if (!x) return KH_ERR_INVALID;
  if (n >> 32) return xfail(x, KH_ERR_INVALID, "kh_index: positions are 32-bit, a text of 2^32 bytes or more is refused");
  if (!append && x->built) return xfail(x, KH_ERR_INVALID, "kh_index: the index is built already (kh_index_clear first)");
  if (append && (uint64_t)pos_base + n > (uint64_t(1) << 32)) return xfail(x, KH_ERR_INVALID, "kh_index_append: pos_base + n passes 2^32, a window position would wrap");
  if (k < 1 || k > 32 * x->kw) return xfail(x, KH_ERR_INVALID, x->kw == 2 ? "kh_wide_index: k must be 1..64" : "kh_index: k must be 1..32");
  if (x->stranded) { const kh_status ss = index_stranded_args(x, n, canonical, append ? pos_base : 0u); if (ss != KH_OK) return ss; }
  if (n < k) return KH_OK;
  if (!text) return xfail(x, KH_ERR_INVALID, "null text");
  kh_table* t = x->t;
  HIPCHK(hipSetDevice(x->device));
  // host text is staged once; k-mers and positions never leave the device
  Scratch s(x->device, t->stream);
  TextFront F;      // (staging only: the k-mer front end masks and scans in a block of its own)
  uint64_t* dk = nullptr; uint32_t* dp = nullptr;
  s.layout([&](Scratch& c) { F.carve(c, text, n, where, false, 0); dk = c.take<uint64_t>(n * x->kw); dp = c.take<uint32_t>(n); });
  if (!s.ok()) { const hipError_t e = s.error(); s.finish(); return hip_fail(t, "kh_index: scratch for the k-mers", e); }
  const void* dtext = F.text;
  uint64_t m = 0;
  kh_status st = kmers_impl(x->kw, dtext, n, k, canonical, KH_MEM_DEVICE, fastq, dk, &m, x->device, t->stream, dp);
  bool touched = !append;      // (a build starts from an empty index: abandoning it changes nothing)
  if (st != KH_OK) fail(t, st, "kh_index: k-mer generation failed");
  else if (append && (x->total + m) >> 32) st = fail(t, KH_ERR_INVALID, "kh_index_append: offsets are 32-bit, the index must stay below 2^32 positions");
  else if (m) {
    touched = true;
    if (x->stranded) st = index_stamp(x, dtext, n, k, dp, m, append ? pos_base : 0u);
    else if (append && pos_base) {
      hipLaunchKernelGGL(k_index_add_base, dim3(grid_for(m, 256, (uint32_t)cu_count(t) * 8)), dim3(256), 0, t->stream, dp, m, pos_base);
      if (hipGetLastError() != hipSuccess) st = fail(t, KH_ERR_HIP, "kh_index_append: k_index_add_base failed");
    }
    if (st == KH_OK) st = append ? index_append_device(x, dk, dp, m) : index_build_device(x, dk, dp, m);
  }
  s.sync();
  s.finish();
  if (st == KH_OK) return KH_OK;
  return touched ? index_abandon(x, st) : xfail(x, st, t->err);
}
// index_text over the (w,k)-minimizers of the text instead of all its windows: count pass, pair buffers of exactly that many entries
// (12 B per emitted pair, not per base), emit pass with pos_base added as it writes, then the build / append of the pairs.
// syncmers: the same route over the closed syncmers of either key width, `w` carrying s (index_syncmers below)
kh_status index_minimizers(kh_index* x, const void* text, uint64_t n, uint32_t k, uint32_t w, int canonical, int hash, uint64_t seed, kh_mem where, bool fastq,
                           bool append, uint32_t pos_base, bool syncmers = false) {
  if (!x) return KH_ERR_INVALID;
  if (!syncmers && x->kw != 1) return xfail(x, KH_ERR_INVALID, "kh_index: minimizers are defined for 64-bit k-mers only");
  if (n >> 32) return xfail(x, KH_ERR_INVALID, "kh_index: positions are 32-bit, a text of 2^32 bytes or more is refused");
  if (!append && x->built) return xfail(x, KH_ERR_INVALID, "kh_index: the index is built already (kh_index_clear first)");
  if (append && (uint64_t)pos_base + n > (uint64_t(1) << 32)) return xfail(x, KH_ERR_INVALID, "kh_index_append: pos_base + n passes 2^32, a window position would wrap");
  if (k < 1 || k > 32 * x->kw) return xfail(x, KH_ERR_INVALID, x->kw == 2 ? "kh_wide_index: k must be 1..64" : "kh_index: k must be 1..32");
  if (syncmers && (w < 1 || w > k || w > 32)) return xfail(x, KH_ERR_INVALID, "kh_index: s must be 1..min(k, 32)");
  if (!syncmers && (w < 1 || w > KM_MZ_WMAX)) return xfail(x, KH_ERR_INVALID, "kh_index: w must be 1..256");
  if (hash < 0 || hash > 3) return xfail(x, KH_ERR_INVALID, "kh_index: unknown order hash");
  if (x->stranded) { const kh_status ss = index_stranded_args(x, n, canonical, append ? pos_base : 0u); if (ss != KH_OK) return ss; }
  if (n < (syncmers ? (uint64_t)k : (uint64_t)w + k - 1)) return KH_OK;
  if (!text) return xfail(x, KH_ERR_INVALID, "null text");
  kh_table* t = x->t;
  HIPCHK(hipSetDevice(x->device));
  MzWork M(x->device, t->stream);
  if (syncmers) { M.s = w; M.kw = x->kw; }
  uint64_t m = 0;
  kh_status st = mz_count(t, M, text, n, k, w, canonical, hash, seed, where, fastq, t->stream, &m);
  if (st != KH_OK) return xfail(x, st, t->err);
  if (append && (x->total + m) >> 32) return xfail(x, KH_ERR_INVALID, "kh_index_append: offsets are 32-bit, the index must stay below 2^32 positions");
  if (m == 0) return KH_OK;
  uint64_t* dk = nullptr; uint32_t* dp = nullptr;
  if (!M.scr.layout([&](Scratch& c) { dk = c.take<uint64_t>(m * x->kw); dp = c.take<uint32_t>(m); })) return xfail(x, M.scr.finish(), "kh_index: no memory for the sampled pairs");
  st = mz_emit(t, M, t->stream, dk, dp, append && !x->stranded ? pos_base : 0u);
  if (st == KH_OK && x->stranded) st = index_stamp(x, M.F.text, n, k, dp, m, append ? pos_base : 0u);      // (FASTQ: the masked text; sequence lines are kept in it)
  bool touched = !append;      // (a build starts from an empty index: abandoning it changes nothing)
  if (st == KH_OK) {
    touched = true;
    st = append ? index_append_device(x, dk, dp, m) : index_build_device(x, dk, dp, m);
  }
  M.scr.sync();
  M.scr.finish();
  if (st == KH_OK) return KH_OK;
  return touched ? index_abandon(x, st) : xfail(x, st, t->err);
}
// every occurrence of the given keys out of the index (keys: device or host, as the table's erase takes them)
kh_status index_erase_keys(kh_index* x, const void* keys, uint64_t n, kh_mem where, uint64_t* n_keys_erased, uint64_t* n_pos_erased) {
  kh_table* t = x->t;
  const uint64_t old_size = t->lsize, old_total = x->total;
  uint64_t ne = 0;
  // the table's own erase: size, capacity and info bytes of the counting twin after the same call; the survivors keep their value, the old rank
  kh_status st = x->kw == 2 ? kh_wide_erase(static_cast<kh_wtable*>(t), keys, n, where, &ne) : kh_erase(t, keys, n, where, &ne);
  // (also after a batch of misses: a re-layout may have changed the order inside a home bucket)
  if (st == KH_OK) st = index_carry(x, 0u, old_size, nullptr, nullptr, 0);
  if (st != KH_OK) return index_abandon(x, st);
  if (n_keys_erased) *n_keys_erased = ne;
  if (n_pos_erased) *n_pos_erased = old_total - x->total;
  return KH_OK;
}
}  // namespace
extern "C" {
kh_status kh_index_create(kh_index** out, kh_hash hash, uint64_t seed, float min_lf, float max_lf, int device) {
  if (!out) return KH_ERR_INVALID;
  *out = nullptr;
  if ((int)hash < 0 || (int)hash > 3) return KH_ERR_INVALID;
  kh_index* x = new kh_index();
  x->hash = (int)hash; x->seed = seed; x->min_lf = min_lf; x->max_lf = max_lf; x->device = device;
  const kh_status st = index_table_create(x);      // (no GPU: KH_ERR_HIP)
  if (st != KH_OK) { delete x; return st; }
  *out = x;
  return KH_OK;
}
kh_status kh_index_destroy(kh_index* x) {
  if (!x) return KH_OK;
  hipSetDevice(x->device);
  if (x->t) { hipStreamSynchronize(x->t->stream); kh_destroy(x->t); }
  pool_free(x->device, x->offsets); pool_free(x->device, x->positions);
  delete x;
  return KH_OK;
}
kh_status kh_index_set_stream(kh_index* x, void* s) {
  if (!x) return KH_ERR_INVALID;
  x->stream = static_cast<hipStream_t>(s);
  return kh_set_stream(x->t, s);
}
const char* kh_index_last_error(const kh_index* x) { return x ? x->err.c_str() : "null index"; }
kh_status kh_index_clear(kh_index* x) { if (!x) return KH_ERR_INVALID; return index_reset(x); }
kh_status kh_index_size(const kh_index* x, uint64_t* out) { if (!x || !out) return KH_ERR_INVALID; *out = x->t->lsize; return KH_OK; }
kh_status kh_index_total(const kh_index* x, uint64_t* out) { if (!x || !out) return KH_ERR_INVALID; *out = x->total; return KH_OK; }
kh_status kh_index_capacity(const kh_index* x, uint64_t* out) { if (!x || !out) return KH_ERR_INVALID; *out = x->t->cur.cap; return KH_OK; }
kh_status kh_index_profile_enable(kh_index* x, int on) { if (!x) return KH_ERR_INVALID; x->prof = on != 0; if (on) kh_profile_reset(x->t); return kh_profile_enable(x->t, on); }
kh_status kh_index_profile_dump(kh_index* x, char* buf, uint64_t cap) { if (!x) return KH_ERR_INVALID; return kh_profile_dump(x->t, buf, cap); }
kh_status kh_index_set_stranded(kh_index* x, int on) {
  if (!x) return KH_ERR_INVALID;
  if (x->t->lsize != 0 || x->total != 0) return xfail(x, KH_ERR_INVALID, "kh_index_set_stranded: only on an empty index (kh_index_clear first)");
  x->stranded = on != 0;
  return KH_OK;
}

kh_status kh_index_build(kh_index* x, const void* keys, const void* pos, uint64_t n, kh_mem where) { return index_pairs(x, keys, pos, n, where, false); }
kh_status kh_index_build_from_sequence(kh_index* x, const void* seq, uint64_t n, uint32_t k, int canonical, kh_mem where) {
  return index_text(x, seq, n, k, canonical, where, false, false, 0u);
}
kh_status kh_index_build_from_fastq(kh_index* x, const void* text, uint64_t n, uint32_t k, int canonical, kh_mem where) {
  return index_text(x, text, n, k, canonical, where, true, false, 0u);
}
kh_status kh_index_append(kh_index* x, const void* keys, const void* pos, uint64_t n, kh_mem where) { return index_pairs(x, keys, pos, n, where, true); }
kh_status kh_index_append_from_sequence(kh_index* x, const void* seq, uint64_t n, uint32_t k, int canonical, kh_mem where, uint32_t pos_base) {
  return index_text(x, seq, n, k, canonical, where, false, true, pos_base);
}
kh_status kh_index_append_from_fastq(kh_index* x, const void* text, uint64_t n, uint32_t k, int canonical, kh_mem where, uint32_t pos_base) {
  return index_text(x, text, n, k, canonical, where, true, true, pos_base);
}
kh_status kh_index_build_from_minimizers(kh_index* x, const void* text, uint64_t n, uint32_t k, uint32_t w, int canonical, kh_hash order_hash, uint64_t order_seed,
                                         kh_mem where, int fastq) {
  return index_minimizers(x, text, n, k, w, canonical, (int)order_hash, order_seed, where, fastq != 0, false, 0u);
}
kh_status kh_index_append_from_minimizers(kh_index* x, const void* text, uint64_t n, uint32_t k, uint32_t w, int canonical, kh_hash order_hash, uint64_t order_seed,
                                          kh_mem where, int fastq, uint32_t pos_base) {
  return index_minimizers(x, text, n, k, w, canonical, (int)order_hash, order_seed, where, fastq != 0, true, pos_base);
}
kh_status kh_index_build_from_syncmers(kh_index* x, const void* text, uint64_t n, uint32_t k, uint32_t s, int canonical, kh_hash order_hash, uint64_t order_seed,
                                       kh_mem where, int fastq) {
  return index_minimizers(x, text, n, k, s, canonical, (int)order_hash, order_seed, where, fastq != 0, false, 0u, true);
}
kh_status kh_index_append_from_syncmers(kh_index* x, const void* text, uint64_t n, uint32_t k, uint32_t s, int canonical, kh_hash order_hash, uint64_t order_seed,
                                        kh_mem where, int fastq, uint32_t pos_base) {
  return index_minimizers(x, text, n, k, s, canonical, (int)order_hash, order_seed, where, fastq != 0, true, pos_base, true);
}
kh_status kh_index_erase(kh_index* x, const void* keys, uint64_t n, kh_mem where, uint64_t* n_keys_erased, uint64_t* n_pos_erased) {
  if (n_keys_erased) *n_keys_erased = 0;
  if (n_pos_erased) *n_pos_erased = 0;
  if (!x) return KH_ERR_INVALID;
  if (n && !keys) return xfail(x, KH_ERR_INVALID, "null argument");
  if (n && !wide_keys_aligned(x->kw, keys, where)) return xfail(x, KH_ERR_INVALID, kWideKeysMisaligned);      // (before the table's own erase: its refusal would abandon the index)
  kh_table* t = x->t;
  HIPCHK(hipSetDevice(x->device));
  if (n == 0 || !x->built) { HIPCHK(hipStreamSynchronize(t->stream)); return KH_OK; }
  return index_erase_keys(x, keys, n, where, n_keys_erased, n_pos_erased);
}
kh_status kh_index_erase_counts(kh_index* x, uint32_t lo, uint32_t hi, uint64_t* n_keys_erased, uint64_t* n_pos_erased) {
  if (n_keys_erased) *n_keys_erased = 0;
  if (n_pos_erased) *n_pos_erased = 0;
  if (!x) return KH_ERR_INVALID;
  kh_table* t = x->t;
  HIPCHK(hipSetDevice(x->device));
  if (lo > hi || !x->built) { HIPCHK(hipStreamSynchronize(t->stream)); return KH_OK; }      // (an empty range erases nothing, as in kh_erase_values)
  // the keys whose segment length lies in the range, selected in slot order: count, scan, emit
  const uint64_t cap = t->cur.cap, size = t->lsize, ntl = (cap + KV_SEL_TILE - 1) / KV_SEL_TILE;
  { kh_status ps = arena_prepare(t, ntl * 12 + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  uint32_t* sums; uint64_t* offs;
  TAKE(sums, uint32_t, ntl); TAKE(offs, uint64_t, ntl + 1);
  { Launch L(t, "k_index_len_count");
    KI_SWITCH_LAYOUT(x, hipLaunchKernelGGL((k_index_len_count<LAY>), dim3((uint32_t)ntl), dim3(KV_SEL_THREADS), 0, t->stream, (const void*)t->cur.p, cap, (const uint32_t*)x->offsets,
                                           size, lo, hi, sums));
    hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, t->stream, (const uint32_t*)sums, ntl, offs); }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t->hpin, offs + ntl, 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  const uint64_t m = t->hpin[0];
  if (m == 0) return KH_OK;
  if (m > size) return xfail(x, KH_ERR_HIP, "kh_index_erase_counts: internal: more keys selected than stored");
  void* list = nullptr;      // (not in the table's workspace: the erase resets it)
  HIPCHK(pool_alloc(x->device, m * 8 * x->kw, &list));
  { Launch L(t, "k_index_len_emit");
    KI_SWITCH_LAYOUT(x, hipLaunchKernelGGL((k_index_len_emit<LAY>), dim3((uint32_t)ntl), dim3(KV_SEL_THREADS), 0, t->stream, (const void*)t->cur.p, cap, (const uint32_t*)x->offsets,
                                           size, lo, hi, (const uint64_t*)offs, static_cast<uint64_t*>(list), m)); }
  kh_status st = hipGetLastError() == hipSuccess ? KH_OK : xfail(x, KH_ERR_HIP, "kh_index_erase_counts: k_index_len_emit failed");
  if (st == KH_OK) st = index_erase_keys(x, list, m, KH_MEM_DEVICE, n_keys_erased, n_pos_erased);
  hipStreamSynchronize(x->t->stream);
  pool_free(x->device, list);
  return st;
}
kh_status kh_index_export(kh_index* x, uint64_t* keys_host, uint32_t* offsets_host, uint32_t* positions_host) {
  if (!x) return KH_ERR_INVALID;
  kh_table* t = x->t;
  HIPCHK(hipSetDevice(x->device));
  const uint64_t size = t->lsize;
  if (!x->built || size == 0) { if (offsets_host) offsets_host[0] = 0; return KH_OK; }
  if (keys_host) {                    // the keys in slot order: the full value range selected in one pass over the slots
    uint64_t m = 0;
    const kh_status st = kh_select_values(t, 0u, 0xFFFFFFFFu, KH_MEM_HOST, keys_host, nullptr, size, &m);
    if (st != KH_OK) { x->err = t->err; return st; }
  }
  if (offsets_host) HIPCHK(hipMemcpyAsync(offsets_host, x->offsets, (size + 1) * 4, hipMemcpyDeviceToHost, t->stream));
  if (positions_host) HIPCHK(hipMemcpyAsync(positions_host, x->positions, x->total * 4, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  return KH_OK;
}

kh_status kh_index_count(kh_index* x, const void* keys, uint64_t n, kh_mem where, uint32_t* out_counts) {
  if (!x) return KH_ERR_INVALID;
  if (n == 0) return KH_OK;
  if (!keys || !out_counts) return xfail(x, KH_ERR_INVALID, "null argument");
  if (!wide_keys_aligned(x->kw, keys, where)) return xfail(x, KH_ERR_INVALID, kWideKeysMisaligned);
  kh_table* t = x->t;
  HIPCHK(hipSetDevice(x->device));
  { kh_status ps = arena_prepare(t, n * (8 * x->kw + 4) + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  const uint64_t* q;
  kh_status st = stage_in<uint64_t>(t, keys, n * x->kw, where, &q);
  if (st != KH_OK) return st;
  uint32_t* dc = out_counts;
  if (where == KH_MEM_HOST) TAKE(dc, uint32_t, n);
  index_launch_lookup(x, q, n, nullptr, dc);
  HIPCHK(hipGetLastError());
  if (where == KH_MEM_HOST) HIPCHK(hipMemcpyAsync(out_counts, dc, n * 4, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  return KH_OK;
}
kh_status kh_index_find(kh_index* x, const void* keys, uint64_t n, kh_mem where, uint64_t* out_offsets, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out) {
  if (n_out) *n_out = 0;
  if (!x) return KH_ERR_INVALID;
  if (!out_offsets || (n && !keys)) return xfail(x, KH_ERR_INVALID, "null argument");
  if (n && !wide_keys_aligned(x->kw, keys, where)) return xfail(x, KH_ERR_INVALID, kWideKeysMisaligned);
  kh_table* t = x->t;
  HIPCHK(hipSetDevice(x->device));
  const bool host = where == KH_MEM_HOST;
  if (n == 0) {
    if (host) out_offsets[0] = 0; else HIPCHK(hipMemsetAsync(out_offsets, 0, 8, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    return KH_OK;
  }
  const uint64_t nst = (n + KI_SCAN_TILE - 1) / KI_SCAN_TILE;
  { kh_status ps = arena_prepare(t, n * (16 + 8 * x->kw) + nst * 8 + (size_t(1) << 20)); if (ps != KH_OK) return ps; }
  const uint64_t* q;
  kh_status st = stage_in<uint64_t>(t, keys, n * x->kw, where, &q);
  if (st != KH_OK) return st;
  uint32_t *begin, *cnt; unsigned long long* ssums; uint64_t* doff = out_offsets;
  TAKE(begin, uint32_t, n); TAKE(cnt, uint32_t, n); TAKE(ssums, unsigned long long, nst + 1);
  if (host) TAKE(doff, uint64_t, n + 1);
  index_launch_lookup(x, q, n, begin, cnt);
  HIPCHK(hipGetLastError());
  st = index_scan<uint64_t>(t, cnt, n, ssums, doff);
  if (st != KH_OK) return st;
  HIPCHK(hipMemcpyAsync(t->hpin, doff + n, 8, hipMemcpyDeviceToHost, t->stream));
  if (host) HIPCHK(hipMemcpyAsync(out_offsets, doff, (n + 1) * 8, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  const uint64_t total = t->hpin[0];
  if (n_out) *n_out = total;
  if (!out_pos || total == 0) return KH_OK;
  if (total > cap_out) return xfail(x, KH_ERR_INVALID, "kh_index_find: more positions than cap_out (n_out holds their number)");
  uint32_t* dout = out_pos;
  if (host) TAKE(dout, uint32_t, total);
  { Launch L(t, "k_index_gather");
    hipLaunchKernelGGL(k_index_gather, dim3(grid_for(total, 256, (uint32_t)cu_count(t) * 8)), dim3(256), 0, t->stream, (const uint32_t*)x->positions, (const uint32_t*)begin,
                       (const uint64_t*)doff, n, total, dout); }
  HIPCHK(hipGetLastError());
  if (host) HIPCHK(hipMemcpyAsync(out_pos, dout, total * 4, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  return KH_OK;
}

// ---- the index over 16-byte keys: the same host code (kh_index::kw == 2) on a wide table and the kw_index_* kernels
kh_status kh_wide_index_create(kh_windex** out, kh_hash hash, uint64_t seed, float min_lf, float max_lf, int device) {
  if (!out) return KH_ERR_INVALID;
  *out = nullptr;
  if ((int)hash < 0 || (int)hash > 3) return KH_ERR_INVALID;
  kh_windex* x = new kh_windex();
  x->kw = 2;
  x->hash = (int)hash; x->seed = seed; x->min_lf = min_lf; x->max_lf = max_lf; x->device = device;
  const kh_status st = index_table_create(x);      // (no GPU: KH_ERR_HIP)
  if (st != KH_OK) { delete x; return st; }
  *out = x;
  return KH_OK;
}
kh_status kh_wide_index_destroy(kh_windex* x) { return kh_index_destroy(x); }
kh_status kh_wide_index_set_stream(kh_windex* x, void* s) { return kh_index_set_stream(x, s); }
const char* kh_wide_index_last_error(const kh_windex* x) { return kh_index_last_error(x); }
kh_status kh_wide_index_clear(kh_windex* x) { return kh_index_clear(x); }
kh_status kh_wide_index_size(const kh_windex* x, uint64_t* out) { return kh_index_size(x, out); }
kh_status kh_wide_index_total(const kh_windex* x, uint64_t* out) { return kh_index_total(x, out); }
kh_status kh_wide_index_capacity(const kh_windex* x, uint64_t* out) { return kh_index_capacity(x, out); }
kh_status kh_wide_index_profile_enable(kh_windex* x, int on) { return kh_index_profile_enable(x, on); }
kh_status kh_wide_index_profile_dump(kh_windex* x, char* buf, uint64_t cap) { return kh_index_profile_dump(x, buf, cap); }
kh_status kh_wide_index_set_stranded(kh_windex* x, int on) { return kh_index_set_stranded(x, on); }
kh_status kh_wide_index_build(kh_windex* x, const void* keys, const void* pos, uint64_t n, kh_mem where) { return kh_index_build(x, keys, pos, n, where); }
kh_status kh_wide_index_build_from_sequence(kh_windex* x, const void* seq, uint64_t n, uint32_t k, int canonical, kh_mem where) {
  return index_text(x, seq, n, k, canonical, where, false, false, 0u);
}
kh_status kh_wide_index_build_from_fastq(kh_windex* x, const void* text, uint64_t n, uint32_t k, int canonical, kh_mem where) {
  return index_text(x, text, n, k, canonical, where, true, false, 0u);
}
kh_status kh_wide_index_append(kh_windex* x, const void* keys, const void* pos, uint64_t n, kh_mem where) { return kh_index_append(x, keys, pos, n, where); }
kh_status kh_wide_index_append_from_sequence(kh_windex* x, const void* seq, uint64_t n, uint32_t k, int canonical, kh_mem where, uint32_t pos_base) {
  return index_text(x, seq, n, k, canonical, where, false, true, pos_base);
}
kh_status kh_wide_index_append_from_fastq(kh_windex* x, const void* text, uint64_t n, uint32_t k, int canonical, kh_mem where, uint32_t pos_base) {
  return index_text(x, text, n, k, canonical, where, true, true, pos_base);
}
kh_status kh_wide_index_build_from_syncmers(kh_windex* x, const void* text, uint64_t n, uint32_t k, uint32_t s, int canonical, kh_hash order_hash, uint64_t order_seed,
                                            kh_mem where, int fastq) {
  return kh_index_build_from_syncmers(x, text, n, k, s, canonical, order_hash, order_seed, where, fastq);
}
kh_status kh_wide_index_append_from_syncmers(kh_windex* x, const void* text, uint64_t n, uint32_t k, uint32_t s, int canonical, kh_hash order_hash, uint64_t order_seed,
                                             kh_mem where, int fastq, uint32_t pos_base) {
  return kh_index_append_from_syncmers(x, text, n, k, s, canonical, order_hash, order_seed, where, fastq, pos_base);
}
kh_status kh_wide_index_erase(kh_windex* x, const void* keys, uint64_t n, kh_mem where, uint64_t* n_keys_erased, uint64_t* n_pos_erased) {
  return kh_index_erase(x, keys, n, where, n_keys_erased, n_pos_erased);
}
kh_status kh_wide_index_erase_counts(kh_windex* x, uint32_t lo, uint32_t hi, uint64_t* n_keys_erased, uint64_t* n_pos_erased) {
  return kh_index_erase_counts(x, lo, hi, n_keys_erased, n_pos_erased);
}
kh_status kh_wide_index_export(kh_windex* x, uint64_t* keys_host, uint32_t* offsets_host, uint32_t* positions_host) {
  return kh_index_export(x, keys_host, offsets_host, positions_host);
}
// the info bytes of the index's table (kh_wide_export_info of it): what pins the layout to the counting twin's
kh_status kh_wide_index_export_info(kh_windex* x, uint8_t* out_host) {
  if (!x) return KH_ERR_INVALID;
  const kh_status st = kh_export_info(x->t, out_host);
  if (st != KH_OK) x->err = x->t->err;
  return st;
}
kh_status kh_wide_index_count(kh_windex* x, const void* keys, uint64_t n, kh_mem where, uint32_t* out_counts) { return kh_index_count(x, keys, n, where, out_counts); }
kh_status kh_wide_index_find(kh_windex* x, const void* keys, uint64_t n, kh_mem where, uint64_t* out_offsets, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out) {
  return kh_index_find(x, keys, n, where, out_offsets, out_pos, cap_out, n_out);
}

// ---- a permuted CSR back into query order (kernels: kh_kernels_csr.h).  No handle: device buffers, the caller's stream.
kh_status kh_csr_unpermute(const uint32_t* counts_perm, const uint32_t* pos_perm, const uint32_t* origin, uint64_t n, uint32_t* out_counts,
                           uint64_t* out_offsets, uint32_t* out_pos, uint64_t cap_out, uint64_t* n_out, int device, void* stream_) {
  if (n >> 32) return KH_ERR_INVALID;
  if (n_out) *n_out = 0;
  if (n && (!counts_perm || !origin)) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (n == 0) {
    if (!out_offsets) return KH_OK;
    HIPCHK0(hipSetDevice(device));
    HIPCHK0(hipMemsetAsync(out_offsets, 0, 8, stream));
    HIPCHK0(hipStreamSynchronize(stream));
    return KH_OK;
  }
  HIPCHK0(hipSetDevice(device));
  const uint64_t nst = (n + KI_SCAN_TILE - 1) / KI_SCAN_TILE;
  Scratch s(device, stream);
  unsigned long long* ssums = nullptr; uint64_t* doff = nullptr; uint32_t *begin_perm = nullptr, *begin_q = nullptr, *cq = nullptr;
  if (!s.layout([&](Scratch& c) {
        ssums = c.take<unsigned long long>(nst + 1);
        doff = out_offsets ? out_offsets : c.take<uint64_t>(n + 1);      // (the caller's, where it gave one)
        begin_perm = c.take<uint32_t>(n + 1);
        begin_q = c.take<uint32_t>(n);
        cq = out_counts ? out_counts : c.take<uint32_t>(n);
      })) return s.finish();
  const uint32_t ncu = (uint32_t)cu_count(device);
  uint64_t total = 0;
  kh_status st = KH_OK;
  // 1. where every permuted slot's segment begins; the total is known (and checked) before any output is written
  scan_counts(stream, counts_perm, n, ssums, begin_perm);
  s.launched();
  s.read(&total, (const uint64_t*)(ssums + nst));
  if (s.sync() && (total >> 32)) st = KH_ERR_INVALID;
  if (s.ok() && st == KH_OK) {
    if (n_out) *n_out = total;
    // 2. counts and begins to their query; 3. the query-order offsets
    hipLaunchKernelGGL(k_csr_scatter, dim3(grid_for(n, KC_THREADS, ncu * 8)), dim3(KC_THREADS), 0, stream, counts_perm, (const uint32_t*)begin_perm, origin, n, cq, begin_q);
    const bool move = out_pos && total && total <= cap_out;
    if (out_offsets || move) scan_counts(stream, (const uint32_t*)cq, n, ssums, doff);
    if (out_pos && total > cap_out) st = KH_ERR_INVALID;
    else if (move && !pos_perm) st = KH_ERR_INVALID;
    // 4. the segments, one output element per lane
    else if (move)
      hipLaunchKernelGGL(k_index_gather, dim3(grid_for(total, 256, ncu * 8)), dim3(256), 0, stream, pos_perm, (const uint32_t*)begin_q, (const uint64_t*)doff, n, total, out_pos);
    s.launched();
  }
  const kh_status fs = s.finish();
  return fs != KH_OK ? fs : st;
}

// ---- strand of window positions (kernel: k_pos_strand in kh_kernels_index.h).  No handle.  Device memory: nothing is allocated and the
//      call only queues its kernel unless n_invalid is asked for; host memory: text and positions are staged in one pooled block.
kh_status kh_stamp_strand(const void* text, uint64_t n, uint32_t k, const uint32_t* pos, uint64_t m, uint32_t pos_base, kh_mem where, uint32_t* out,
                          uint64_t* n_invalid, int device, void* stream_) {
  if (n_invalid) *n_invalid = 0;
  if (k < 1 || k > 64 || (n >> 31) || (uint64_t)pos_base + n > (uint64_t(1) << 31)) return KH_ERR_INVALID;
  if (m == 0) return KH_OK;
  if (!pos || !out || (!text && n)) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  Scratch s(device, stream);
  const uint8_t* dtext = nullptr; const uint32_t* dpos = nullptr; uint32_t* dout = nullptr; unsigned long long* dcnt = nullptr;
  if (!s.layout([&](Scratch& c) {
        dtext = c.in(static_cast<const uint8_t*>(text), n, where);
        dpos = c.in(pos, m, where);
        dout = c.out(out, m, where);
        dcnt = c.take<unsigned long long>(n_invalid ? 1 : 0);
      })) return s.finish();
  if (dcnt) s.zero(dcnt, 8);
  hipLaunchKernelGGL((k_pos_strand<true>), dim3(grid_for(m, 256, (uint32_t)cu_count(device) * 8)), dim3(256), 0, stream, dtext, n, k, dpos, m, pos_base, dout, dcnt);
  s.launched();
  unsigned long long bad = 0;
  if (dcnt) s.read(&bad, dcnt);
  s.copy_back(dout, m);
  const kh_status st = s.finish();      // (staged arrays or a counter: waits; else the kernel is only queued)
  if (st == KH_OK && n_invalid) *n_invalid = bad;
  return st;
}
// ---- a CSR of hits over stamped positions into flat anchors (kernel: k_anchors_expand).  No handle; device memory: queued only.
kh_status kh_anchors_from_csr(const uint32_t* qpos, const uint64_t* offsets, uint64_t n, const uint32_t* pos, uint64_t total, kh_mem where,
                              uint32_t* out_qpos, uint32_t* out_rpos, uint8_t* out_rev, int device, void* stream_) {
  if (total >> 32) return KH_ERR_INVALID;
  if (n == 0 || total == 0) return KH_OK;
  if (!qpos || !offsets || !pos || !out_qpos || !out_rpos || !out_rev) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  Scratch s(device, stream);
  const uint64_t* doff = nullptr; const uint32_t *dq = nullptr, *dp = nullptr;
  uint32_t *oq = nullptr, *orp = nullptr; uint8_t* orv = nullptr;
  if (!s.layout([&](Scratch& c) {
        doff = c.in(offsets, n + 1, where); dq = c.in(qpos, n, where); dp = c.in(pos, total, where);
        oq = c.out(out_qpos, total, where); orp = c.out(out_rpos, total, where); orv = c.out(out_rev, total, where);
      })) return s.finish();
  hipLaunchKernelGGL(k_anchors_expand, dim3(grid_for(total, 256, (uint32_t)cu_count(device) * 8)), dim3(256), 0, stream, dq, doff, n, dp, total, oq, orp, orv);
  s.launched();
  s.copy_back(oq, total); s.copy_back(orp, total); s.copy_back(orv, total);
  return s.finish();
}
// ---- collinear chains per segment from flat anchors (kernels: kh_kernels_chain.h).  No handle; one pooled block holds the scratch (and
//      the staged arrays of a host call); every kernel is queued on the caller's stream and the one host wait is the one for *n_chains.
kh_status kh_chain_anchors(const uint32_t* qpos, const uint32_t* rpos, const uint8_t* rev, uint64_t m, const uint64_t* seg_offsets, uint64_t n_seg, uint32_t k,
                           uint32_t lookback, uint32_t max_gap, uint32_t band, int32_t min_score, uint32_t min_count, kh_mem where, int32_t* out_score,
                           int32_t* out_pred, int32_t* out_chain, uint32_t* c_first, uint32_t* c_last, uint32_t* c_count, int32_t* c_score, uint64_t cap_chains,
                           uint64_t* n_chains, int device, void* stream_) {
  const int n_tab = (c_first != nullptr) + (c_last != nullptr) + (c_count != nullptr) + (c_score != nullptr);
  if (k < 1 || k > 64 || lookback < 1 || lookback > 64 || max_gap < 1 || (max_gap >> 31) || (band >> 31)) return KH_ERR_INVALID;
  if (m > (uint64_t(1) << 24) || (where != KH_MEM_HOST && where != KH_MEM_DEVICE) || (n_tab != 0 && n_tab != 4)) return KH_ERR_INVALID;
  if (seg_offsets && (n_seg > m + (uint64_t(1) << 24) || (n_seg == 0 && m))) return KH_ERR_INVALID;
  if (m && (!qpos || !rpos || !rev || !out_score || !out_pred || !out_chain)) return KH_ERR_INVALID;
  if (m == 0) { if (n_chains) *n_chains = 0; return KH_OK; }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  const bool table = n_tab == 4;
  const uint64_t nst = (m + KI_SCAN_TILE - 1) / KI_SCAN_TILE, tab = table ? std::min<uint64_t>(cap_chains, m) : 0;
  Scratch s(device, stream);
  int32_t* bc = nullptr; uint32_t *cnt = nullptr, *last = nullptr, *bad = nullptr, *num = nullptr; unsigned long long* ssums = nullptr;
  const uint32_t *dq = nullptr, *dr = nullptr; const uint8_t* dv = nullptr; const uint64_t* dseg = nullptr;
  int32_t *df = nullptr, *dp = nullptr, *dc = nullptr, *t_score = nullptr;
  uint32_t *t_first = nullptr, *t_last = nullptr, *t_count = nullptr;
  if (!s.layout([&](Scratch& c) {
        bc = c.take<int32_t>(m);                                                                   // best child, then the kept-chain flags
        // taken in a row: one memset clears the three (bad: one word, taken as a whole 256 bytes so that the memset ends on the boundary)
        cnt = c.take<uint32_t>(m); last = c.take<uint32_t>(m); bad = c.take<uint32_t>(64);
        num = c.take<uint32_t>(m + 1);                                                             // chain numbers
        ssums = c.take<unsigned long long>(nst + 1);
        dq = c.in(qpos, m, where); dr = c.in(rpos, m, where); dv = c.in(rev, m, where);
        dseg = c.in(seg_offsets, seg_offsets ? n_seg + 1 : 0, where);
        df = c.out(out_score, m, where); dp = c.out(out_pred, m, where); dc = c.out(out_chain, m, where);
        t_first = c.out(c_first, tab, where); t_last = c.out(c_last, tab, where); t_count = c.out(c_count, tab, where); t_score = c.out(c_score, tab, where);
      })) return s.finish();
  s.zero(cnt, reinterpret_cast<char*>(bad + 64) - reinterpret_cast<char*>(cnt));
  const uint32_t ncu = (uint32_t)cu_count(device);
  const uint32_t m32 = (uint32_t)m, ns32 = (uint32_t)n_seg;
  const uint32_t gseg = grid_for(dseg ? n_seg : 1, KCH_WAVES, ncu * 8), gflat = grid_for(m, 256, ncu * 8);
  const KchParams P{k, lookback, max_gap, band};
  hipLaunchKernelGGL(k_chain_dp, dim3(gseg), dim3(KCH_THREADS), 0, stream, dq, dr, dv, m32, dseg, ns32, P, df, dp, bad);
  hipLaunchKernelGGL(k_chain_link, dim3(gseg), dim3(KCH_THREADS), 0, stream, (const int32_t*)df, (const int32_t*)dp, m32, dseg, ns32, bc, dc, cnt, last);
  uint32_t* flag = reinterpret_cast<uint32_t*>(bc);          // (the best children are done with)
  hipLaunchKernelGGL((k_chain_emit<0>), dim3(gflat), dim3(256), 0, stream, (const int32_t*)df, (const int32_t*)dp, dc, m32, (const uint32_t*)cnt, (const uint32_t*)last,
                     min_score, min_count, flag, (const uint32_t*)num, (const unsigned long long*)(ssums + nst), (const uint32_t*)bad, t_first, t_last, t_count, t_score, tab);
  scan_counts(stream, (const uint32_t*)flag, m, ssums, num);
  hipLaunchKernelGGL((k_chain_emit<1>), dim3(gflat), dim3(256), 0, stream, (const int32_t*)df, (const int32_t*)dp, dc, m32, (const uint32_t*)cnt, (const uint32_t*)last,
                     min_score, min_count, flag, (const uint32_t*)num, (const unsigned long long*)(ssums + nst), (const uint32_t*)bad, t_first, t_last, t_count, t_score, tab);
  s.launched();
  unsigned long long total = 0;
  uint32_t hbad = 0;
  s.read(&total, (const unsigned long long*)(ssums + nst));
  s.read(&hbad, (const uint32_t*)bad);
  s.sync();      // the one host wait of a device call: *n_chains
  kh_status st = KH_OK;
  if (hbad) { st = KH_ERR_INVALID; total = 0; }
  else if (table && total > cap_chains) st = KH_ERR_INVALID;
  if (!hbad) {
    s.copy_back(df, m); s.copy_back(dp, m); s.copy_back(dc, m);
    if (st == KH_OK) { s.copy_back(t_first, total); s.copy_back(t_last, total); s.copy_back(t_count, total); s.copy_back(t_score, total); }
  }
  const kh_status fs = s.finish();
  if (fs != KH_OK) return fs;
  if (n_chains) *n_chains = total;
  return st;
}
// ---- edit distance per chain link (kernels: kh_kernels_edits.h).  No handle; one pooled block holds the worklist (and the staged arrays
//      of a host call).  A device call only queues: two memsets, two kernels and the return of the block, all on the caller's stream.
kh_status kh_chain_edits(const void* qtext, uint64_t nq, const void* rtext, uint64_t nr, uint32_t ref_base, const uint32_t* qpos, const uint32_t* rpos,
                         const uint8_t* rev, const int32_t* pred, const int32_t* chain, uint64_t m, uint64_t n_chains, uint32_t k, uint32_t max_edits,
                         kh_mem where, int32_t* out_link, uint32_t* c_edits, uint32_t* c_over, int device, void* stream_) {
  if (!chain_text_limits_ok(k, m, nq, nr, ref_base) || max_edits > 31) return KH_ERR_INVALID;
  if ((where != KH_MEM_HOST && where != KH_MEM_DEVICE) || (n_chains && (!c_edits || !c_over))) return KH_ERR_INVALID;
  if (m && (!qpos || !rpos || !rev || !pred || !chain || !out_link || (nq && !qtext) || (nr && !rtext))) return KH_ERR_INVALID;
  const uint64_t nc = std::min<uint64_t>(n_chains, uint64_t(1) << 31);      // (a chain number is an int32: rows beyond 2^31 are never addressed)
  if (m == 0 && where == KH_MEM_HOST) {
    if (nc) { memset(c_edits, 0, nc * sizeof(uint32_t)); memset(c_over, 0, nc * sizeof(uint32_t)); }
    return KH_OK;
  }
  if (m == 0 && nc == 0) return KH_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  Scratch s(device, stream);
  uint32_t *wl = nullptr, *wl_count = nullptr, *de = nullptr, *dov = nullptr;
  int32_t* dl = nullptr;
  KedArgs P{};
  if (!s.layout([&](Scratch& c) {
        wl = c.take<uint32_t>(m); wl_count = c.take<uint32_t>(m ? 1 : 0);
        chain_text_args(c, P, qtext, nq, rtext, nr, ref_base, qpos, rpos, rev, pred, chain, m, k, where);
        dl = c.out(out_link, m, where); de = c.out(c_edits, nc, where); dov = c.out(c_over, nc, where);
      })) return s.finish();
  if (nc) { s.zero(de, nc * sizeof(uint32_t)); s.zero(dov, nc * sizeof(uint32_t)); }
  if (m) {
    s.zero(wl_count, sizeof(uint32_t));
    P.n_chains = (uint32_t)nc; P.max_edits = max_edits;
    const uint32_t ncu = (uint32_t)cu_count(device);
    hipLaunchKernelGGL(k_edits_classify, dim3(grid_for(m, KED_THREADS, ncu * 8)), dim3(KED_THREADS), 0, stream, P, dl, dov, wl, wl_count);
    hipLaunchKernelGGL(k_edits_wfa, dim3(grid_for(m, KED_WAVES, ncu * 8)), dim3(KED_THREADS), 0, stream, P, (const uint32_t*)wl, (const uint32_t*)wl_count, dl, de, dov);
    s.launched();
  }
  s.copy_back(dl, m); s.copy_back(de, nc); s.copy_back(dov, nc);
  return s.finish_queued();
}
// ---- alignment operations per chain link (kernels: kh_kernels_cigar.h).  No handle; one pooled block holds the worklist, the run counts
//      and the path words (and the staged arrays of a host call), a second one the staged rows of a host call.  Everything is queued on
//      the caller's stream; the one host wait is the one that learns *n_ops.
kh_status kh_chain_cigars(const void* qtext, uint64_t nq, const void* rtext, uint64_t nr, uint32_t ref_base, const uint32_t* qpos, const uint32_t* rpos,
                          const uint8_t* rev, const int32_t* pred, const int32_t* chain, uint64_t m, uint64_t n_chains, uint32_t k, const int32_t* link,
                          kh_mem where, uint64_t* out_offsets, uint32_t* out_ops, uint64_t cap_ops, uint64_t* n_ops, uint32_t* c_ins, uint32_t* c_del,
                          int device, void* stream_) {
  if (!chain_text_limits_ok(k, m, nq, nr, ref_base)) return KH_ERR_INVALID;
  if ((where != KH_MEM_HOST && where != KH_MEM_DEVICE) || (n_chains && (!c_ins || !c_del)) || !out_offsets || !n_ops) return KH_ERR_INVALID;
  if (m && (!qpos || !rpos || !rev || !pred || !chain || !link || (nq && !qtext) || (nr && !rtext))) return KH_ERR_INVALID;
  const uint64_t nc = std::min<uint64_t>(n_chains, uint64_t(1) << 31);      // (a chain number is an int32: rows beyond 2^31 are never addressed)
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  *n_ops = 0;
  if (m == 0) {      // the offset and the two counters: cleared at once in host memory, by three queued memsets in device memory
    const kh_status st = empty_rows(out_offsets, 1, where, device, stream);
    if (st != KH_OK || nc == 0) return st;
    if (where == KH_MEM_HOST) { memset(c_ins, 0, nc * sizeof(uint32_t)); memset(c_del, 0, nc * sizeof(uint32_t)); return KH_OK; }
    HIPCHK0(hipMemsetAsync(c_ins, 0, nc * sizeof(uint32_t), stream));
    HIPCHK0(hipMemsetAsync(c_del, 0, nc * sizeof(uint32_t), stream));
    return KH_OK;
  }
  HIPCHK0(hipSetDevice(device));
  const uint64_t nst = (m + KI_SCAN_TILE - 1) / KI_SCAN_TILE;
  Scratch s(device, stream);
  uint32_t *wl = nullptr, *wl_count = nullptr, *runs = nullptr, *di = nullptr, *dd = nullptr;
  uint64_t *paths = nullptr, *doff = nullptr; unsigned long long* ssums = nullptr;
  const int32_t* dlink = nullptr;
  KedArgs P{};
  if (!s.layout([&](Scratch& c) {
        wl = c.take<uint32_t>(m); wl_count = c.take<uint32_t>(1); runs = c.take<uint32_t>(m); paths = c.take<uint64_t>(m);
        ssums = c.take<unsigned long long>(nst + 1);
        chain_text_args(c, P, qtext, nq, rtext, nr, ref_base, qpos, rpos, rev, pred, chain, m, k, where);
        dlink = c.in(link, m, where);
        doff = c.out(out_offsets, m + 1, where); di = c.out(c_ins, nc, where); dd = c.out(c_del, nc, where);
      })) return s.finish();
  if (nc) { s.zero(di, nc * sizeof(uint32_t)); s.zero(dd, nc * sizeof(uint32_t)); }
  s.zero(wl_count, sizeof(uint32_t));
  P.n_chains = (uint32_t)nc; P.max_edits = 31;
  const uint32_t ncu = (uint32_t)cu_count(device);
  hipLaunchKernelGGL(k_cigar_classify, dim3(grid_for(m, KED_THREADS, ncu * 8)), dim3(KED_THREADS), 0, stream, P, dlink, runs, wl, wl_count);
  hipLaunchKernelGGL(k_cigar_wfa, dim3(grid_for(m, KED_WAVES, ncu * 8)), dim3(KED_THREADS), 0, stream, P, dlink, (const uint32_t*)wl, (const uint32_t*)wl_count, runs,
                     paths, di, dd);
  scan_counts(stream, (const uint32_t*)runs, m, ssums, doff);
  s.launched();
  unsigned long long total = 0;
  s.read(&total, (const unsigned long long*)(ssums + nst));
  s.copy_back(doff, m + 1); s.copy_back(di, nc); s.copy_back(dd, nc);
  return emit_total(s, total, out_ops, cap_ops, n_ops, where, [&](uint32_t* dops) {
    hipLaunchKernelGGL(k_cigar_emit, dim3(grid_for(m, KED_THREADS, ncu * 8)), dim3(KED_THREADS), 0, stream, P, dlink, (const uint64_t*)doff, (const uint64_t*)paths,
                       (uint64_t)total, dops);
  });
}
// ---- the ends of every kept chain (kernels: kh_kernels_ends.h).  No handle; one pooled block holds the run counts and the path words
//      (and the staged arrays of a host call), a second one the staged rows of a host call.  Everything is queued on the caller's
//      stream; the one host wait is the one that learns *n_ops.
kh_status kh_chain_ends(const void* qtext, uint64_t nq, const void* rtext, uint64_t nr, uint32_t ref_base, const uint32_t* qpos, const uint32_t* rpos,
                        const uint8_t* rev, uint64_t m, const uint32_t* c_first, const uint32_t* c_last, const uint32_t* q_lo, const uint32_t* q_hi,
                        uint64_t n_chains, uint32_t k, uint32_t max_edits, uint32_t clip_cost, kh_mem where, uint32_t* e_q, uint32_t* e_r, uint32_t* e_edits,
                        uint32_t* e_clip, uint64_t* out_offsets, uint32_t* out_ops, uint64_t cap_ops, uint64_t* n_ops, int device, void* stream_) {
  if (!chain_text_limits_ok(k, m, nq, nr, ref_base) || max_edits > 31 || clip_cost < 1 || clip_cost > 255 || n_chains > (uint64_t(1) << 23)) return KH_ERR_INVALID;
  if ((where != KH_MEM_HOST && where != KH_MEM_DEVICE) || !out_offsets || !n_ops) return KH_ERR_INVALID;
  if (n_chains && (!c_first || !c_last || !q_lo || !q_hi || !e_q || !e_r || !e_edits || !e_clip)) return KH_ERR_INVALID;
  if (n_chains && m && (!qpos || !rpos || !rev || (nq && !qtext) || (nr && !rtext))) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  *n_ops = 0;
  if (n_chains == 0) return empty_rows(out_offsets, 1, where, device, stream);
  HIPCHK0(hipSetDevice(device));
  const uint64_t rows = 2 * n_chains, nst = (rows + KI_SCAN_TILE - 1) / KI_SCAN_TILE;
  Scratch s(device, stream);
  uint32_t *runs = nullptr, *dq = nullptr, *dr = nullptr, *de = nullptr, *dc = nullptr;
  uint64_t *paths = nullptr, *doff = nullptr; unsigned long long* ssums = nullptr;
  KenArgs P{};
  if (!s.layout([&](Scratch& c) {
        runs = c.take<uint32_t>(rows); paths = c.take<uint64_t>(rows); ssums = c.take<unsigned long long>(nst + 1);
        chain_text_args(c, P.T, qtext, nq, rtext, nr, ref_base, qpos, rpos, rev, nullptr, nullptr, m, k, where);
        P.c_first = c.in(c_first, n_chains, where); P.c_last = c.in(c_last, n_chains, where);
        P.q_lo = c.in(q_lo, n_chains, where); P.q_hi = c.in(q_hi, n_chains, where);
        dq = c.out(e_q, rows, where); dr = c.out(e_r, rows, where); de = c.out(e_edits, rows, where); dc = c.out(e_clip, rows, where);
        doff = c.out(out_offsets, rows + 1, where);
      })) return s.finish();
  P.T.n_chains = (uint32_t)n_chains; P.T.max_edits = max_edits; P.clip_cost = clip_cost;
  const uint32_t ncu = (uint32_t)cu_count(device);
  hipLaunchKernelGGL(k_ends_wfa, dim3(grid_for(rows, KED_WAVES, ncu * 8)), dim3(KED_THREADS), 0, stream, P, dq, dr, de, dc, runs, paths);
  scan_counts(stream, (const uint32_t*)runs, rows, ssums, doff);
  s.launched();
  unsigned long long total = 0;
  s.read(&total, (const unsigned long long*)(ssums + nst));
  s.copy_back(doff, rows + 1); s.copy_back(dq, rows); s.copy_back(dr, rows); s.copy_back(de, rows); s.copy_back(dc, rows);
  return emit_total(s, total, out_ops, cap_ops, n_ops, where, [&](uint32_t* dops) {
    hipLaunchKernelGGL(k_ends_emit, dim3(grid_for(rows, KED_THREADS, ncu * 8)), dim3(KED_THREADS), 0, stream, P, (const uint64_t*)doff, (const uint64_t*)paths, (uint64_t)total,
                       dops);
  });
}
// ---- primaries, secondaries and a mapping quality per group of chains (kernels: kh_kernels_select.h).  No handle; there is no count to
//      learn, so a device call only queues: at most one memset, two kernels and the return of the pooled block, and never waits.
kh_status kh_chain_select(const uint32_t* q_start, const uint32_t* q_end, const int32_t* score, const uint32_t* count, uint64_t n_chains, const uint64_t* offsets,
                          uint64_t n_grp, uint32_t mask_pct, uint32_t pri_pct, uint32_t best_n, kh_mem where, int32_t* out_parent, uint32_t* out_rank,
                          uint8_t* out_mapq, uint8_t* out_flag, int32_t* out_sub, uint32_t* out_nsub, int32_t* out_best, int device, void* stream_) {
  if (mask_pct > 100 || pri_pct > 100 || n_chains > (uint64_t(1) << 23) || n_grp > n_chains + (uint64_t(1) << 24)) return KH_ERR_INVALID;
  if ((where != KH_MEM_HOST && where != KH_MEM_DEVICE) || (offsets && n_grp == 0)) return KH_ERR_INVALID;
  if (n_chains && (!q_start || !q_end || !score || !count || !out_parent || !out_rank || !out_mapq || !out_flag || !out_sub || !out_nsub)) return KH_ERR_INVALID;
  const uint64_t ng = offsets ? n_grp : 1;
  if (offsets && where == KH_MEM_HOST) {      // (device memory: nobody can look before the kernels run; they clamp)
    if (offsets[0] != 0 || offsets[ng] != n_chains) return KH_ERR_INVALID;
    for (uint64_t g = 0; g < ng; ++g)
      if (offsets[g] > offsets[g + 1]) return KH_ERR_INVALID;
  }
  if (n_chains == 0 && (where == KH_MEM_HOST || !out_best)) {
    for (uint64_t g = 0; out_best && g < ng; ++g) out_best[g] = -1;
    return KH_OK;
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  if (n_chains == 0) { HIPCHK0(hipMemsetAsync(out_best, 0xFF, ng * sizeof(int32_t), stream)); return KH_OK; }
  const uint64_t big = n_chains > 64 ? n_chains : 0;      // no group of more than 64 chains without that many chains
  const uint64_t stride = (big + 63) & ~uint64_t(63);     // words per scratch array (whole 256 bytes)
  Scratch s(device, stream);
  KselArgs P{};
  KselScratch W{};
  if (!s.layout([&](Scratch& c) {
        W.base = c.take<uint32_t>(KSEL_SCRATCH_ARRAYS * stride);
        P.qs = c.in(q_start, n_chains, where); P.qe = c.in(q_end, n_chains, where); P.score = c.in(score, n_chains, where); P.count = c.in(count, n_chains, where);
        P.off = c.in(offsets, offsets ? ng + 1 : 0, where);
        P.parent = c.out(out_parent, n_chains, where); P.rank = c.out(out_rank, n_chains, where); P.mapq = c.out(out_mapq, n_chains, where);
        P.flag = c.out(out_flag, n_chains, where); P.sub = c.out(out_sub, n_chains, where); P.nsub = c.out(out_nsub, n_chains, where);
        P.best = c.out(out_best, out_best ? ng : 0, where);
      })) return s.finish();
  W.stride = (uint32_t)stride;
  P.n = (uint32_t)n_chains; P.n_grp = (uint32_t)ng; P.mask_pct = mask_pct; P.pri_pct = pri_pct; P.best_n = best_n;
  const uint32_t ncu = (uint32_t)cu_count(device);
  hipLaunchKernelGGL(k_select_wave, dim3(grid_for(ng, KSEL_WAVES, ncu * 8)), dim3(KSEL_THREADS), 0, stream, P);
  if (big) hipLaunchKernelGGL(k_select_block, dim3(grid_for(ng, 1, ncu * 2)), dim3(KSEL_THREADS), 0, stream, P, W);
  s.launched();
  s.copy_back(P.parent, n_chains); s.copy_back(P.rank, n_chains); s.copy_back(P.mapq, n_chains); s.copy_back(P.flag, n_chains);
  s.copy_back(P.sub, n_chains); s.copy_back(P.nsub, n_chains); s.copy_back(P.best, ng);
  return s.finish_queued();      // (host memory: copies are pending, so this waits)
}
// ---- one record per chain (kernels: kh_kernels_records.h).  No handle; one pooled block holds the run counts and the scan's tile sums
//      (and the staged arrays of a host call), a second one the staged rows of a host call.  Everything is queued on the caller's
//      stream; the one host wait of a pass is the one that learns *n_ops.
kh_status kh_chain_records(const uint32_t* qpos, const uint32_t* rpos, const uint8_t* rev, const int32_t* chain, uint64_t m, const uint64_t* lk_offsets,
                           const uint32_t* lk_ops, uint64_t n_lk, const uint32_t* c_first, const uint32_t* c_last, const uint32_t* q_lo, const uint32_t* q_hi,
                           uint64_t n_chains, const uint32_t* e_q, const uint32_t* e_r, const uint32_t* e_clip, const uint64_t* en_offsets, const uint32_t* en_ops,
                           uint64_t n_en, uint32_t k, uint32_t ref_order, kh_mem where, uint8_t* out_valid, uint32_t* out_qs, uint32_t* out_qe, uint32_t* out_rs,
                           uint32_t* out_re, uint32_t* out_qlen, uint32_t* out_match, uint32_t* out_block, uint32_t* out_nm, uint64_t* out_offsets,
                           uint32_t* out_ops, uint64_t cap_ops, uint64_t* n_ops, int device, void* stream_) {
  const uint64_t lim = uint64_t(1) << 31;
  if (k < 1 || k > 64 || ref_order > 1 || m > (uint64_t(1) << 24) || n_chains > (uint64_t(1) << 23) || n_lk > lim || n_en > lim) return KH_ERR_INVALID;
  if ((where != KH_MEM_HOST && where != KH_MEM_DEVICE) || !out_offsets || !n_ops) return KH_ERR_INVALID;
  if (n_chains && (!c_first || !c_last || !q_lo || !q_hi || !e_q || !e_r || !e_clip || !en_offsets || (n_en && !en_ops))) return KH_ERR_INVALID;
  if (n_chains && (!out_valid || !out_qs || !out_qe || !out_rs || !out_re || !out_qlen || !out_match || !out_block || !out_nm)) return KH_ERR_INVALID;
  if (n_chains && m && (!qpos || !rpos || !rev || !chain || !lk_offsets || (n_lk && !lk_ops))) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  *n_ops = 0;
  if (n_chains == 0) return empty_rows(out_offsets, 1, where, device, stream);
  HIPCHK0(hipSetDevice(device));
  const uint64_t nst = (n_chains + KI_SCAN_TILE - 1) / KI_SCAN_TILE;
  Scratch s(device, stream);
  uint32_t* runs = nullptr; uint64_t* doff = nullptr; unsigned long long* ssums = nullptr;
  KrcArgs P{};
  KrcOut O{};
  if (!s.layout([&](Scratch& c) {
        runs = c.take<uint32_t>(n_chains); ssums = c.take<unsigned long long>(nst + 1);
        P.qpos = c.in(qpos, m, where); P.rpos = c.in(rpos, m, where); P.rev = c.in(rev, m, where); P.chain = c.in(chain, m, where);
        P.lk_off = c.in(lk_offsets, m ? m + 1 : 0, where); P.lk_ops = c.in(lk_ops, m ? n_lk : 0, where);
        P.c_first = c.in(c_first, n_chains, where); P.c_last = c.in(c_last, n_chains, where); P.q_lo = c.in(q_lo, n_chains, where); P.q_hi = c.in(q_hi, n_chains, where);
        P.e_q = c.in(e_q, 2 * n_chains, where); P.e_r = c.in(e_r, 2 * n_chains, where); P.e_clip = c.in(e_clip, 2 * n_chains, where);
        P.en_off = c.in(en_offsets, 2 * n_chains + 1, where); P.en_ops = c.in(en_ops, n_en, where);
        O.valid = c.out(out_valid, n_chains, where); O.qs = c.out(out_qs, n_chains, where); O.qe = c.out(out_qe, n_chains, where);
        O.rs = c.out(out_rs, n_chains, where); O.re = c.out(out_re, n_chains, where); O.qlen = c.out(out_qlen, n_chains, where);
        O.n_match = c.out(out_match, n_chains, where); O.n_block = c.out(out_block, n_chains, where); O.nm = c.out(out_nm, n_chains, where);
        doff = c.out(out_offsets, n_chains + 1, where);
      })) return s.finish();
  P.n_lk = m ? n_lk : 0; P.n_en = n_en; P.m = (uint32_t)m; P.n_chains = (uint32_t)n_chains; P.k = k; P.ref_order = ref_order;
  const uint32_t ncu = (uint32_t)cu_count(device);
  hipLaunchKernelGGL(k_records_count, dim3(grid_for(n_chains, KRC_WAVES, ncu * 8)), dim3(KRC_THREADS), 0, stream, P, O, runs);
  scan_counts(stream, (const uint32_t*)runs, n_chains, ssums, doff);
  s.launched();
  unsigned long long total = 0;
  s.read(&total, (const unsigned long long*)(ssums + nst));
  s.copy_back(doff, n_chains + 1); s.copy_back(O.valid, n_chains); s.copy_back(O.qs, n_chains); s.copy_back(O.qe, n_chains); s.copy_back(O.rs, n_chains);
  s.copy_back(O.re, n_chains); s.copy_back(O.qlen, n_chains); s.copy_back(O.n_match, n_chains); s.copy_back(O.n_block, n_chains); s.copy_back(O.nm, n_chains);
  return emit_total(s, total, out_ops, cap_ops, n_ops, where, [&](uint32_t* dops) {
    s.zero(dops, total * sizeof(uint32_t));      // (the runs are added onto zeroes)
    hipLaunchKernelGGL(k_records_emit, dim3(grid_for(n_chains, KRC_WAVES, ncu * 8)), dim3(KRC_THREADS), 0, stream, P, (const uint64_t*)doff, (uint64_t)total, dops);
  });
}
// ---- a run CSR as text (kernels: kh_kernels_records.h).  The same protocol: count, scan, one host wait for *n_text, emit.
kh_status kh_cigar_text(const uint64_t* offsets, uint64_t n_rows, const uint32_t* ops, uint64_t n_ops, kh_mem where, uint64_t* out_offsets, uint8_t* out_text,
                        uint64_t cap_text, uint64_t* n_text, int device, void* stream_) {
  const uint64_t lim = uint64_t(1) << 31;
  if (n_rows > lim || n_ops > lim || (where != KH_MEM_HOST && where != KH_MEM_DEVICE) || !out_offsets || !n_text) return KH_ERR_INVALID;
  if ((n_rows && !offsets) || (n_rows && n_ops && !ops)) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  *n_text = 0;
  if (n_rows == 0 || n_ops == 0) return empty_rows(out_offsets, n_rows + 1, where, device, stream);
  HIPCHK0(hipSetDevice(device));
  const uint64_t nst = (n_ops + KI_SCAN_TILE - 1) / KI_SCAN_TILE;
  Scratch s(device, stream);
  uint32_t* bytes = nullptr; uint64_t *boff = nullptr, *doff = nullptr; unsigned long long *ssums = nullptr, *dtotal = nullptr;
  const uint64_t* din = nullptr; const uint32_t* dops = nullptr;
  if (!s.layout([&](Scratch& c) {
        bytes = c.take<uint32_t>(n_ops); boff = c.take<uint64_t>(n_ops + 1); ssums = c.take<unsigned long long>(nst + 1); dtotal = c.take<unsigned long long>(1);
        din = c.in(offsets, n_rows + 1, where); dops = c.in(ops, n_ops, where);
        doff = c.out(out_offsets, n_rows + 1, where);
      })) return s.finish();
  const uint32_t ncu = (uint32_t)cu_count(device);
  hipLaunchKernelGGL(k_text_count, dim3(grid_for(n_ops, KTX_THREADS, ncu * 8)), dim3(KTX_THREADS), 0, stream, dops, n_ops, bytes);
  scan_counts(stream, (const uint32_t*)bytes, n_ops, ssums, boff);
  hipLaunchKernelGGL(k_text_rows, dim3(grid_for(n_rows + 1, KTX_THREADS, ncu * 8)), dim3(KTX_THREADS), 0, stream, din, n_rows, n_ops, (const uint64_t*)boff, doff, dtotal);
  s.launched();
  unsigned long long total = 0;
  s.read(&total, (const unsigned long long*)dtotal);
  s.copy_back(doff, n_rows + 1);
  return emit_total(s, total, out_text, cap_text, n_text, where, [&](uint8_t* dtext) {
    hipLaunchKernelGGL(k_text_emit, dim3(grid_for(n_ops, KTX_THREADS, ncu * 8)), dim3(KTX_THREADS), 0, stream, dops, din, n_rows, n_ops, (const uint64_t*)boff, (uint64_t)total,
                       dtext);
  });
}
// ---- the anchors of every segment regrouped by target (kernels: kh_kernels_targets.h).  No handle; one pooled block holds the ids, the
//      group counts and the scan's workspace (and the staged arrays of a host call).  Everything is queued on the caller's stream; the
//      one host wait is the one that learns *n_grp.
static_assert(KTG_NONE == KH_TARGET_NONE && KTG_NONE == KH_POS_INVALID, "one word for no target and no position");
kh_status kh_anchor_targets(const uint32_t* qpos, const uint32_t* rpos, const uint8_t* rev, uint64_t m, const uint64_t* seg_offsets, uint64_t n_seg,
                            const uint32_t* t_start, const uint32_t* t_end, uint64_t n_t, uint32_t k, kh_mem where, uint32_t* out_q, uint32_t* out_r, uint8_t* out_v,
                            uint32_t* out_tid, uint32_t* out_src, uint64_t* g_offsets, uint32_t* g_seg, uint32_t* g_tid, uint64_t* n_grp, int device, void* stream_) {
  if (k < 1 || k > 64 || m > (uint64_t(1) << 24) || n_t < 1 || n_t > (uint64_t(1) << 24)) return KH_ERR_INVALID;
  if ((where != KH_MEM_HOST && where != KH_MEM_DEVICE) || !g_offsets || !n_grp) return KH_ERR_INVALID;
  if (seg_offsets && (n_seg > m + (uint64_t(1) << 24) || (n_seg == 0 && m))) return KH_ERR_INVALID;
  if (m && (!qpos || !rpos || !rev || !t_start || !t_end || !out_q || !out_r || !out_v || !out_tid || !out_src || !g_seg || !g_tid)) return KH_ERR_INVALID;
  *n_grp = 0;
  if (m == 0 && where == KH_MEM_HOST) { g_offsets[0] = 0; return KH_OK; }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  if (m == 0) { HIPCHK0(hipMemsetAsync(g_offsets, 0, sizeof(uint64_t), stream)); return KH_OK; }
  const uint64_t ns = seg_offsets ? n_seg : 1, nst = (ns + KI_SCAN_TILE - 1) / KI_SCAN_TILE;
  Scratch s(device, stream);
  uint32_t *tid = nullptr, *counts = nullptr, *bad = nullptr; uint64_t* first_grp = nullptr; unsigned long long* ssums = nullptr;
  const uint32_t *ts = nullptr, *te = nullptr;
  KtgIn P{};
  KtgOut O{};
  if (!s.layout([&](Scratch& c) {
        tid = c.take<uint32_t>(m); counts = c.take<uint32_t>(ns); first_grp = c.take<uint64_t>(ns + 1); ssums = c.take<unsigned long long>(nst + 1);
        bad = c.take<uint32_t>(1);
        P.qpos = c.in(qpos, m, where); P.rpos = c.in(rpos, m, where); P.rev = c.in(rev, m, where);
        P.seg = c.in(seg_offsets, seg_offsets ? n_seg + 1 : 0, where);
        ts = c.in(t_start, n_t, where); te = c.in(t_end, n_t, where);
        O.q = c.out(out_q, m, where); O.r = c.out(out_r, m, where); O.v = c.out(out_v, m, where); O.tid = c.out(out_tid, m, where); O.src = c.out(out_src, m, where);
        O.g_off = c.out(g_offsets, m + 1, where); O.g_seg = c.out(g_seg, m, where); O.g_tid = c.out(g_tid, m, where);
      })) return s.finish();
  s.zero(bad, sizeof(uint32_t));
  P.m = (uint32_t)m; P.n_seg = (uint32_t)n_seg;
  const uint32_t ncu = (uint32_t)cu_count(device), gseg = grid_for(ns, KTG_WAVES, ncu * 8);
  if (n_t <= KH_TARGETS_STAGED_MAX) {
    // both tables in LDS, 8 n_t bytes per workgroup: as many workgroups per CU as 160 KiB hold, at most 8
    const size_t lds = (size_t)n_t * 2 * sizeof(uint32_t);
    const uint32_t per_cu = (uint32_t)std::min<size_t>(8, (size_t(160) << 10) / lds);
    hipLaunchKernelGGL((k_target_find<true>), dim3(grid_for(m, KTG_THREADS, ncu * per_cu)), dim3(KTG_THREADS), lds, stream, P.rpos, P.m, ts, te, (uint32_t)n_t, k, tid);
  } else {
    hipLaunchKernelGGL((k_target_find<false>), dim3(grid_for(m, KTG_THREADS, ncu * 8)), dim3(KTG_THREADS), 0, stream, P.rpos, P.m, ts, te, (uint32_t)n_t, k, tid);
  }
  hipLaunchKernelGGL((k_target_group<false>), dim3(gseg), dim3(KTG_THREADS), 0, stream, P, (const uint32_t*)tid, counts, (const uint64_t*)first_grp, bad, O);
  scan_counts(stream, (const uint32_t*)counts, ns, ssums, first_grp);
  hipLaunchKernelGGL((k_target_group<true>), dim3(gseg), dim3(KTG_THREADS), 0, stream, P, (const uint32_t*)tid, counts, (const uint64_t*)first_grp, bad, O);
  s.launched();
  unsigned long long total = 0;
  uint32_t hbad = 0;
  s.read(&total, (const unsigned long long*)(ssums + nst));
  s.read(&hbad, (const uint32_t*)bad);
  s.sync();      // the one host wait of a device call: *n_grp
  if (s.ok() && !hbad && total <= m) {
    s.copy_back(O.q, m); s.copy_back(O.r, m); s.copy_back(O.v, m); s.copy_back(O.tid, m); s.copy_back(O.src, m);
    s.copy_back(O.g_off, total + 1); s.copy_back(O.g_seg, total); s.copy_back(O.g_tid, total);
  }
  const kh_status fs = s.finish();
  if (fs != KH_OK) return fs;
  if (hbad || total > m) return KH_ERR_INVALID;
  *n_grp = total;
  return KH_OK;
}
// ---- the cs or MD string of every record row (kernels: kh_kernels_sam.h).  The protocol of kh_cigar_text: count, scan, one host wait for
//      *n_text, emit.  One pooled block holds the byte counts and the scan's tile sums (and the staged arrays of a host call), a second
//      one the staged text of a host call.
kh_status kh_record_diffs(const void* qtext, uint64_t nq, const void* rtext, uint64_t nr, uint32_t ref_base, const uint64_t* offsets, const uint32_t* ops, uint64_t n_ops,
                          const uint8_t* valid, const uint8_t* rev, const uint32_t* q_lo, const uint32_t* q_hi, const uint32_t* rs, uint64_t n_rows, uint32_t kind,
                          kh_mem where, uint8_t* out_ok, uint64_t* out_offsets, uint8_t* out_text, uint64_t cap_text, uint64_t* n_text, int device, void* stream_) {
  const uint64_t lim = uint64_t(1) << 31, tlim = uint64_t(1) << 32;
  if (kind > KH_DIFF_MD || n_rows > lim || n_ops > lim || nq > tlim || nr > tlim) return KH_ERR_INVALID;
  if ((where != KH_MEM_HOST && where != KH_MEM_DEVICE) || !out_offsets || !n_text) return KH_ERR_INVALID;
  if (n_rows && (!offsets || !valid || !rev || !q_lo || !q_hi || !rs || !out_ok || (n_ops && !ops) || (nq && !qtext) || (nr && !rtext))) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  *n_text = 0;
  if (n_rows == 0) return empty_rows(out_offsets, 1, where, device, stream);
  HIPCHK0(hipSetDevice(device));
  const uint64_t nst = (n_rows + KI_SCAN_TILE - 1) / KI_SCAN_TILE;
  Scratch s(device, stream);
  uint32_t* bytes = nullptr; uint64_t* doff = nullptr; unsigned long long* ssums = nullptr; uint8_t* dok = nullptr;
  KdfArgs P{};
  if (!s.layout([&](Scratch& c) {
        bytes = c.take<uint32_t>(n_rows); ssums = c.take<unsigned long long>(nst + 1);
        P.qtext = c.in(static_cast<const uint8_t*>(qtext), nq, where); P.rtext = c.in(static_cast<const uint8_t*>(rtext), nr, where);
        P.off = c.in(offsets, n_rows + 1, where); P.ops = c.in(ops, n_ops, where);
        P.valid = c.in(valid, n_rows, where); P.rev = c.in(rev, n_rows, where); P.q_lo = c.in(q_lo, n_rows, where); P.q_hi = c.in(q_hi, n_rows, where);
        P.rs = c.in(rs, n_rows, where);
        dok = c.out(out_ok, n_rows, where); doff = c.out(out_offsets, n_rows + 1, where);
      })) return s.finish();
  P.nq = nq; P.nr = nr; P.n_ops = n_ops; P.ref_base = ref_base; P.n_rows = (uint32_t)n_rows;
  const uint32_t ncu = (uint32_t)cu_count(device);
  const dim3 grid(grid_for(n_rows, KDF_WAVES, ncu * 8));
  if (kind == KH_DIFF_CS) hipLaunchKernelGGL((k_diffs_count<KDF_CS>), grid, dim3(KDF_THREADS), 0, stream, P, dok, bytes);
  else hipLaunchKernelGGL((k_diffs_count<KDF_MD>), grid, dim3(KDF_THREADS), 0, stream, P, dok, bytes);
  scan_counts(stream, (const uint32_t*)bytes, n_rows, ssums, doff);
  s.launched();
  unsigned long long total = 0;
  s.read(&total, (const unsigned long long*)(ssums + nst));
  s.copy_back(doff, n_rows + 1); s.copy_back(dok, n_rows);
  return emit_total(s, total, out_text, cap_text, n_text, where, [&](uint8_t* dtext) {
    if (kind == KH_DIFF_CS) hipLaunchKernelGGL((k_diffs_emit<KDF_CS>), grid, dim3(KDF_THREADS), 0, stream, P, (const uint8_t*)dok, (const uint64_t*)doff, (uint64_t)total, dtext);
    else hipLaunchKernelGGL((k_diffs_emit<KDF_MD>), grid, dim3(KDF_THREADS), 0, stream, P, (const uint8_t*)dok, (const uint64_t*)doff, (uint64_t)total, dtext);
  });
}
// ---- byte ranges of a text as rows, reverse-strand rows back to front (kernels: kh_kernels_sam.h).  The same protocol.
kh_status kh_oriented_rows(const void* text, uint64_t n, const uint32_t* lo, const uint32_t* hi, const uint8_t* rev, uint64_t n_rows, uint32_t complement, kh_mem where,
                           uint64_t* out_offsets, uint8_t* out_text, uint64_t cap_text, uint64_t* n_text, int device, void* stream_) {
  if (complement > 1 || n_rows > (uint64_t(1) << 31) || n > (uint64_t(1) << 32)) return KH_ERR_INVALID;
  if ((where != KH_MEM_HOST && where != KH_MEM_DEVICE) || !out_offsets || !n_text) return KH_ERR_INVALID;
  if (n_rows && (!lo || !hi || !rev || (n && !text))) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  *n_text = 0;
  if (n_rows == 0) return empty_rows(out_offsets, 1, where, device, stream);
  HIPCHK0(hipSetDevice(device));
  const uint64_t nst = (n_rows + KI_SCAN_TILE - 1) / KI_SCAN_TILE;
  Scratch s(device, stream);
  uint32_t* len = nullptr; uint64_t* doff = nullptr; unsigned long long* ssums = nullptr;
  const uint8_t *din = nullptr, *drev = nullptr; const uint32_t *dlo = nullptr, *dhi = nullptr;
  if (!s.layout([&](Scratch& c) {
        len = c.take<uint32_t>(n_rows); ssums = c.take<unsigned long long>(nst + 1);
        din = c.in(static_cast<const uint8_t*>(text), n, where); dlo = c.in(lo, n_rows, where); dhi = c.in(hi, n_rows, where); drev = c.in(rev, n_rows, where);
        doff = c.out(out_offsets, n_rows + 1, where);
      })) return s.finish();
  const uint32_t ncu = (uint32_t)cu_count(device);
  hipLaunchKernelGGL(k_orient_len, dim3(grid_for(n_rows, KOR_THREADS, ncu * 8)), dim3(KOR_THREADS), 0, stream, dlo, dhi, n_rows, n, len);
  scan_counts(stream, (const uint32_t*)len, n_rows, ssums, doff);
  s.launched();
  unsigned long long total = 0;
  s.read(&total, (const unsigned long long*)(ssums + nst));
  s.copy_back(doff, n_rows + 1);
  return emit_total(s, total, out_text, cap_text, n_text, where, [&](uint8_t* dtext) {
    hipLaunchKernelGGL(k_orient_copy, dim3(grid_for(n_rows, KOR_WAVES, ncu * 8)), dim3(KOR_THREADS), 0, stream, din, n, dlo, dhi, drev, (uint32_t)n_rows, complement,
                       (const uint64_t*)doff, (uint64_t)total, dtext);
  });
}
// ---- the concordant chain pair of every read pair (kernel: kh_kernels_pair.h).  No handle and no count to learn: a device call queues
//      one kernel and never waits; a host call stages through one pooled block.
static_assert(KPR_NONE == KH_TARGET_NONE && KPR_CAP == KH_PAIR_CANDIDATES, "one word for no target, one cap");
kh_status kh_pair_chains(const uint32_t* rs, const uint32_t* re, const uint8_t* rev, const int32_t* score, const uint32_t* tid, const uint8_t* use, const uint8_t* mapq_in,
                         uint64_t n_chains, const uint64_t* offsets, uint64_t n_reads, uint32_t min_ins, uint32_t max_ins, uint32_t unpaired_pen, kh_mem where,
                         int32_t* out_row, uint8_t* out_mapq, int32_t* out_tlen, uint8_t* out_flag, int32_t* out_score, uint32_t* out_nconc, int device, void* stream_) {
  if ((n_reads & 1) || min_ins > max_ins || n_chains > (uint64_t(1) << 23) || n_reads > n_chains + (uint64_t(1) << 24)) return KH_ERR_INVALID;
  if ((where != KH_MEM_HOST && where != KH_MEM_DEVICE) || !offsets) return KH_ERR_INVALID;
  if (n_reads && (!out_row || !out_mapq || !out_tlen || !out_flag || !out_score || !out_nconc)) return KH_ERR_INVALID;
  if (n_chains && (!rs || !re || !rev || !score)) return KH_ERR_INVALID;
  if (where == KH_MEM_HOST) {      // (device memory: nobody can look before the kernel runs; it clamps)
    if (offsets[0] != 0 || offsets[n_reads] != n_chains) return KH_ERR_INVALID;
    for (uint64_t g = 0; g < n_reads; ++g)
      if (offsets[g] > offsets[g + 1]) return KH_ERR_INVALID;
  }
  if (n_reads == 0) return KH_OK;
  const uint64_t n_pairs = n_reads / 2;
  if (n_chains == 0 && where == KH_MEM_HOST) {
    for (uint64_t s = 0; s < n_reads; ++s) { out_row[s] = -1; out_mapq[s] = 0; out_tlen[s] = 0; }
    for (uint64_t p = 0; p < n_pairs; ++p) { out_flag[p] = 0; out_score[p] = 0; out_nconc[p] = 0; }
    return KH_OK;
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  if (n_chains == 0) {
    HIPCHK0(hipMemsetAsync(out_row, 0xFF, n_reads * sizeof(int32_t), stream));
    HIPCHK0(hipMemsetAsync(out_mapq, 0, n_reads, stream));
    HIPCHK0(hipMemsetAsync(out_tlen, 0, n_reads * sizeof(int32_t), stream));
    HIPCHK0(hipMemsetAsync(out_flag, 0, n_pairs, stream));
    HIPCHK0(hipMemsetAsync(out_score, 0, n_pairs * sizeof(int32_t), stream));
    HIPCHK0(hipMemsetAsync(out_nconc, 0, n_pairs * sizeof(uint32_t), stream));
    return KH_OK;
  }
  Scratch s(device, stream);
  KprArgs P{};
  if (!s.layout([&](Scratch& c) {
        P.rs = c.in(rs, n_chains, where); P.re = c.in(re, n_chains, where); P.rev = c.in(rev, n_chains, where); P.score = c.in(score, n_chains, where);
        P.tid = c.in(tid, tid ? n_chains : 0, where); P.use = c.in(use, use ? n_chains : 0, where); P.mapq_in = c.in(mapq_in, mapq_in ? n_chains : 0, where);
        P.off = c.in(offsets, n_reads + 1, where);
        P.row = c.out(out_row, n_reads, where); P.mapq = c.out(out_mapq, n_reads, where); P.tlen = c.out(out_tlen, n_reads, where);
        P.flag = c.out(out_flag, n_pairs, where); P.score_out = c.out(out_score, n_pairs, where); P.nconc = c.out(out_nconc, n_pairs, where);
      })) return s.finish();
  P.n = (uint32_t)n_chains; P.n_pairs = (uint32_t)n_pairs; P.min_ins = min_ins; P.max_ins = max_ins; P.pen = unpaired_pen;
  const uint32_t ncu = (uint32_t)cu_count(device);
  hipLaunchKernelGGL(k_pair_wave, dim3(grid_for(n_pairs, KPR_WAVES, ncu * 8)), dim3(KPR_THREADS), 0, stream, P);
  s.launched();
  s.copy_back(P.row, n_reads); s.copy_back(P.mapq, n_reads); s.copy_back(P.tlen, n_reads);
  s.copy_back(P.flag, n_pairs); s.copy_back(P.score_out, n_pairs); s.copy_back(P.nconc, n_pairs);
  return s.finish_queued();      // (host memory: copies are pending, so this waits)
}
// ---- a mate without a row aligned inside the window its partner allows (kernels: kh_kernels_rescue.h).  No handle; one pooled block
//      holds the run counts and the path words (and the staged arrays of a host call), a second one the staged rows of a host call.
//      Everything is queued on the caller's stream; the one host wait is the one that learns *n_ops.
static_assert(KRS_NONE == KH_RESCUE_NONE && KRS_OVER == KH_RESCUE_OVER && KRS_MAX_READ == KH_RESCUE_MAX_READ && KRS_MAX_WINDOW == KH_RESCUE_MAX_WINDOW,
              "one word for no answer, one for too far, one set of limits");
kh_status kh_mate_rescue(const void* qtext, uint64_t nq, const void* rtext, uint64_t nr, uint32_t ref_base, const uint32_t* q_lo, const uint32_t* q_hi,
                         const uint32_t* w_lo, const uint32_t* w_hi, const uint8_t* rev, uint64_t n, uint32_t max_edits, kh_mem where, int32_t* out_edits,
                         uint32_t* out_rs, uint32_t* out_re, uint32_t* out_span, uint64_t* out_offsets, uint32_t* out_ops, uint64_t cap_ops, uint64_t* n_ops,
                         int device, void* stream_) {
  if (!chain_text_limits_ok(1, n, nq, nr, ref_base) || max_edits > 31) return KH_ERR_INVALID;
  if ((where != KH_MEM_HOST && where != KH_MEM_DEVICE) || !out_offsets || !n_ops) return KH_ERR_INVALID;
  if (n && (!q_lo || !q_hi || !w_lo || !w_hi || !rev || !out_edits || !out_rs || !out_re || !out_span || (nq && !qtext) || (nr && !rtext))) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  *n_ops = 0;
  if (n == 0) return empty_rows(out_offsets, 1, where, device, stream);
  HIPCHK0(hipSetDevice(device));
  const uint64_t nst = (n + KI_SCAN_TILE - 1) / KI_SCAN_TILE;
  Scratch s(device, stream);
  uint32_t *runs = nullptr, *ds = nullptr, *de = nullptr, *dsp = nullptr;
  int32_t* dd = nullptr;
  uint64_t *paths = nullptr, *doff = nullptr; unsigned long long* ssums = nullptr;
  KrsArgs P{};
  if (!s.layout([&](Scratch& c) {
        runs = c.take<uint32_t>(n); paths = c.take<uint64_t>(n); ssums = c.take<unsigned long long>(nst + 1);
        P.T.qtext = c.in(static_cast<const uint8_t*>(qtext), nq, where); P.T.rtext = c.in(static_cast<const uint8_t*>(rtext), nr, where);
        P.q_lo = c.in(q_lo, n, where); P.q_hi = c.in(q_hi, n, where); P.w_lo = c.in(w_lo, n, where); P.w_hi = c.in(w_hi, n, where); P.rev = c.in(rev, n, where);
        dd = c.out(out_edits, n, where); ds = c.out(out_rs, n, where); de = c.out(out_re, n, where); dsp = c.out(out_span, n, where);
        doff = c.out(out_offsets, n + 1, where);
      })) return s.finish();
  P.T.nq = (uint32_t)nq; P.T.nr = (uint32_t)nr; P.T.ref_base = ref_base; P.T.max_edits = max_edits; P.n = (uint32_t)n;      // (no anchors: the rest of T stays null)
  const uint32_t ncu = (uint32_t)cu_count(device);
  const dim3 gscan(grid_for(n, KRS_THREADS, ncu * 16)), bscan(KRS_THREADS);
  hipLaunchKernelGGL((k_rescue_scan<1>), gscan, bscan, 0, stream, P, dd, ds, de, dsp, runs);
  hipLaunchKernelGGL((k_rescue_scan<2>), gscan, bscan, 0, stream, P, dd, ds, de, dsp, runs);
  hipLaunchKernelGGL((k_rescue_scan<3>), gscan, bscan, 0, stream, P, dd, ds, de, dsp, runs);
  hipLaunchKernelGGL((k_rescue_scan<4>), gscan, bscan, 0, stream, P, dd, ds, de, dsp, runs);
  hipLaunchKernelGGL((k_rescue_scan<8>), gscan, bscan, 0, stream, P, dd, ds, de, dsp, runs);
  hipLaunchKernelGGL(k_rescue_wfa, dim3(grid_for(n, KED_WAVES, ncu * 8)), dim3(KED_THREADS), 0, stream, P, dd, ds, de, dsp, runs, paths);
  scan_counts(stream, (const uint32_t*)runs, n, ssums, doff);
  s.launched();
  unsigned long long total = 0;
  s.read(&total, (const unsigned long long*)(ssums + nst));
  s.copy_back(doff, n + 1); s.copy_back(dd, n); s.copy_back(ds, n); s.copy_back(de, n); s.copy_back(dsp, n);
  return emit_total(s, total, out_ops, cap_ops, n_ops, where, [&](uint32_t* dops) {
    hipLaunchKernelGGL(k_rescue_emit, dim3(grid_for(n, KED_THREADS, ncu * 8)), dim3(KED_THREADS), 0, stream, P, (const int32_t*)dd, (const uint32_t*)de,
                       (const uint64_t*)doff, (const uint64_t*)paths, (uint64_t)total, dops);
  });
}
// ---- SAM lines from line columns and byte CSRs (kernels: kh_kernels_samtext.h).  The protocol of kh_cigar_text: count, scan, one host
//      wait for *n_text, emit.  One pooled block holds the line lengths and the scan's tile sums (and the staged arrays of a host call), a
//      second one the staged text of a host call.
static_assert(KST_CSRS == 7 && KST_COLS == 19, "the seven CSRs and the nineteen line columns of the entry point");
static_assert(KST_TAGS_BASE == KH_SAMTAG_BASE && KST_TAGS_S2 == KH_SAMTAG_S2 && KST_TAGS_MD == KH_SAMTAG_MD && KST_TAGS_CS == KH_SAMTAG_CS &&
              KST_ROW_SAME == KH_SAM_RNEXT_SAME, "one set of tag bits, one word for the line's own target");
kh_status kh_sam_lines(const uint64_t* names_off, const uint8_t* names_text, uint64_t n_names, uint64_t names_bytes, const uint64_t* tnames_off, const uint8_t* tnames_text,
                       uint64_t n_tnames, uint64_t tnames_bytes, const uint64_t* cigar_off, const uint8_t* cigar_text, uint64_t n_cigar, uint64_t cigar_bytes,
                       const uint64_t* seq_off, const uint8_t* seq_text, uint64_t n_seq, uint64_t seq_bytes, const uint64_t* qual_off, const uint8_t* qual_text,
                       uint64_t n_qual, uint64_t qual_bytes, const uint64_t* md_off, const uint8_t* md_text, uint64_t n_md, uint64_t md_bytes, const uint64_t* cs_off,
                       const uint8_t* cs_text, uint64_t n_cs, uint64_t cs_bytes, const int32_t* l_name, const uint32_t* l_flag, const int32_t* l_rname,
                       const uint32_t* l_pos, const uint8_t* l_mapq, const int32_t* l_cigar, const int32_t* l_rnext, const uint32_t* l_pnext, const int32_t* l_tlen,
                       const int32_t* l_seq, const int32_t* l_qual, const uint8_t* l_tags, const uint32_t* l_nm, const uint8_t* l_tp, const uint32_t* l_cm,
                       const int32_t* l_s1, const int32_t* l_s2, const int32_t* l_md, const int32_t* l_cs, uint64_t n_lines, kh_mem where, uint64_t* out_offsets,
                       uint8_t* out_text, uint64_t cap_text, uint64_t* n_text, int device, void* stream_) {
  const uint64_t lim = uint64_t(1) << 31, tlim = uint64_t(1) << 32;
  struct In { const uint64_t* off; const uint8_t* txt; uint64_t n_rows, n_bytes; };
  const In in[7] = {{names_off, names_text, n_names, names_bytes}, {tnames_off, tnames_text, n_tnames, tnames_bytes}, {cigar_off, cigar_text, n_cigar, cigar_bytes},
                    {seq_off, seq_text, n_seq, seq_bytes}, {qual_off, qual_text, n_qual, qual_bytes}, {md_off, md_text, n_md, md_bytes}, {cs_off, cs_text, n_cs, cs_bytes}};
  if (n_lines > lim || (where != KH_MEM_HOST && where != KH_MEM_DEVICE) || !out_offsets || !n_text) return KH_ERR_INVALID;
  uint64_t longest = KH_SAM_LINE_FIXED + tnames_bytes;      // (a line can print a target name twice: RNAME and RNEXT)
  for (const In& c : in) {
    if (c.n_rows > lim || c.n_bytes > tlim || (c.n_rows && !c.off) || (c.n_bytes && !c.txt)) return KH_ERR_INVALID;
    longest += c.n_bytes;
  }
  if (longest >= tlim) return KH_ERR_INVALID;
  if (n_lines && (!l_name || !l_flag || !l_rname || !l_pos || !l_mapq || !l_cigar || !l_rnext || !l_pnext || !l_tlen || !l_seq || !l_qual || !l_tags || !l_nm || !l_tp ||
                  !l_cm || !l_s1 || !l_s2 || !l_md || !l_cs)) return KH_ERR_INVALID;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  *n_text = 0;
  if (n_lines == 0) return empty_rows(out_offsets, 1, where, device, stream);
  HIPCHK0(hipSetDevice(device));
  const uint64_t nst = (n_lines + KI_SCAN_TILE - 1) / KI_SCAN_TILE;
  Scratch s(device, stream);
  uint32_t* bytes = nullptr; uint64_t* doff = nullptr; unsigned long long* ssums = nullptr;
  KstArgs P{};
  if (!s.layout([&](Scratch& c) {
        bytes = c.take<uint32_t>(n_lines); ssums = c.take<unsigned long long>(nst + 1);
        for (int j = 0; j < 7; ++j) {      // (a CSR without rows stays null: every row index lies outside it)
          P.csr[j].off = c.in(in[j].off, in[j].n_rows ? in[j].n_rows + 1 : 0, where); P.csr[j].txt = c.in(in[j].txt, in[j].n_rows ? in[j].n_bytes : 0, where);
          P.csr[j].n_rows = in[j].n_rows; P.csr[j].n_bytes = in[j].n_rows ? in[j].n_bytes : 0;
        }
        int j = 0;
        for (const uint32_t* p : {l_flag, l_pos, l_pnext, l_nm, l_cm}) { static const int at[5] = {1, 3, 7, 12, 14}; P.col[at[j++]] = c.in(p, n_lines, where); }
        j = 0;
        for (const int32_t* p : {l_name, l_rname, l_cigar, l_rnext, l_tlen, l_seq, l_qual, l_s1, l_s2, l_md, l_cs}) {
          static const int at[11] = {0, 2, 5, 6, 8, 9, 10, 15, 16, 17, 18};
          P.col[at[j++]] = c.in(p, n_lines, where);
        }
        P.col[KST_COL_MAPQ] = c.in(l_mapq, n_lines, where); P.col[KST_COL_TAGS] = c.in(l_tags, n_lines, where); P.col[KST_COL_TP] = c.in(l_tp, n_lines, where);
        doff = c.out(out_offsets, n_lines + 1, where);
      })) return s.finish();
  P.n_lines = (uint32_t)n_lines;
  const uint32_t ncu = (uint32_t)cu_count(device);
  hipLaunchKernelGGL(k_samtext_count, dim3(grid_for(n_lines, KST_WAVES, ncu * 8)), dim3(KST_THREADS), 0, stream, P, bytes);
  scan_counts(stream, (const uint32_t*)bytes, n_lines, ssums, doff);
  s.launched();
  unsigned long long total = 0;
  s.read(&total, (const unsigned long long*)(ssums + nst));
  s.copy_back(doff, n_lines + 1);
  return emit_total(s, total, out_text, cap_text, n_text, where, [&](uint8_t* dtext) {
    hipLaunchKernelGGL(k_samtext_emit, dim3(grid_for(n_lines, KST_WAVES, ncu * 8)), dim3(KST_THREADS), 0, stream, P, (const uint64_t*)doff, (uint64_t)total, dtext);
  });
}
// ---- the record structure of a FASTQ text (kernels: kh_kernels_fastq.h).  One call is one pass: tile sums, scan, line ends, records,
//      then the one host wait that learns the three counts.  The record kernel derives the record count itself, where the host does not
//      know it yet: a call with too little room writes no column.  One pooled block holds the counts, the tile sums, the line ends (and
//      the staged arrays of a host call).
static_assert(KFQ_STRIP_MATE == KH_FASTQ_STRIP_MATE && KFQ_NO_AT == KH_FASTQ_NO_AT && KFQ_NO_PLUS == KH_FASTQ_NO_PLUS && KFQ_LENGTHS == KH_FASTQ_LENGTHS &&
              KFQ_NO_NAME == KH_FASTQ_NO_NAME, "one flag, one set of status bits");
kh_status kh_fastq_records(const void* text, uint64_t n, uint32_t flags, kh_mem where, uint32_t* name_lo, uint32_t* name_hi, uint32_t* seq_lo, uint32_t* seq_hi,
                           uint32_t* qual_lo, uint8_t* status, uint64_t cap, uint64_t* n_records, uint64_t* n_bad, uint32_t* tail_lines, int device, void* stream_) {
  const int given = (name_lo != nullptr) + (name_hi != nullptr) + (seq_lo != nullptr) + (seq_hi != nullptr) + (qual_lo != nullptr);
  if (n >= (uint64_t(1) << 32) || (flags & ~KH_FASTQ_STRIP_MATE) || (where != KH_MEM_HOST && where != KH_MEM_DEVICE) || !n_records || (n && !text) ||
      (given != 0 && given != 5)) return KH_ERR_INVALID;
  const bool emit = given == 5;
  if (n == 0) {
    *n_records = 0;
    if (n_bad) *n_bad = 0;
    if (tail_lines) *tail_lines = 0;
    return KH_OK;
  }
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  const uint64_t ntl = cmp_tiles(n);
  const uint64_t room = emit ? std::min<uint64_t>(cap, uint64_t(1) << 30) : 0;      // (n < 2^32 bytes: at most 2^30 records)
  const uint64_t cap_lines = emit ? std::min<uint64_t>(n, 4 * room + 4) : n;        // a newline per line; the count pass knows no bound but n
  Scratch s(device, stream);
  KfqArgs P{};
  uint32_t* sums = nullptr; uint64_t* offs = nullptr; uint32_t* line_end = nullptr;
  if (!s.layout([&](Scratch& c) {
        P.counts = c.take<uint32_t>(4); sums = c.take<uint32_t>(ntl); offs = c.take<uint64_t>(ntl + 1); line_end = c.take<uint32_t>(cap_lines);
        P.text = c.in(static_cast<const uint8_t*>(text), n, where);
        if (emit) {
          P.name_lo = c.out(name_lo, room, where); P.name_hi = c.out(name_hi, room, where); P.seq_lo = c.out(seq_lo, room, where); P.seq_hi = c.out(seq_hi, room, where);
          P.qual_lo = c.out(qual_lo, room, where); P.status = c.out(status, status ? room : 0, where);
        }
      })) return s.finish();
  P.line_end = line_end; P.n_newlines = offs + ntl; P.n = n; P.cap_lines = cap_lines; P.cap = room; P.flags = flags;
  s.zero(P.counts, 4 * sizeof(uint32_t));
  hipLaunchKernelGGL(k_newline_tile_sums, dim3((uint32_t)ntl), dim3(256), 0, stream, P.text, n, sums);
  hipLaunchKernelGGL(k_scan_u32_to_u64, dim3(1), dim3(KH_SCAN_THREADS), 0, stream, (const uint32_t*)sums, ntl, offs);
  hipLaunchKernelGGL(k_fastq_line_ends, dim3((uint32_t)ntl), dim3(256), 0, stream, P.text, n, (const uint64_t*)offs, line_end, cap_lines);
  hipLaunchKernelGGL(k_fastq_records, dim3(grid_for(cap_lines / 4 + 1, KFQ_THREADS, (uint32_t)cu_count(device) * 8)), dim3(KFQ_THREADS), 0, stream, P);
  s.launched();
  uint32_t counts[4] = {0, 0, 0, 0};
  s.read(counts, (const uint32_t*)P.counts, 4);
  if (!s.sync()) return s.finish();
  *n_records = counts[0];
  if (emit && counts[0] > cap) { s.finish(); return KH_ERR_INVALID; }
  if (n_bad) *n_bad = counts[1];
  if (tail_lines) *tail_lines = counts[2];
  if (emit) {
    s.copy_back(P.name_lo, counts[0]); s.copy_back(P.name_hi, counts[0]); s.copy_back(P.seq_lo, counts[0]); s.copy_back(P.seq_hi, counts[0]);
    s.copy_back(P.qual_lo, counts[0]); s.copy_back(P.status, status ? counts[0] : 0);
  }
  return s.finish();
}
// ---- byte rows gathered to given places (kernel: kh_kernels_fastq.h).  No count to learn: a device call queues one kernel and never waits.
kh_status kh_pack_rows(const void* text, uint64_t n, const uint32_t* lo, const uint32_t* hi, const uint64_t* dst, uint64_t n_rows, int sep, kh_mem where, uint8_t* out,
                       uint64_t out_n, int device, void* stream_) {
  const uint64_t tlim = uint64_t(1) << 32;
  if (n >= tlim || out_n >= tlim || n_rows > (uint64_t(1) << 31) || sep < -1 || sep > 255 || (where != KH_MEM_HOST && where != KH_MEM_DEVICE)) return KH_ERR_INVALID;
  if (n_rows && (!lo || !hi || !dst || (n && !text) || (out_n && !out))) return KH_ERR_INVALID;
  if (n_rows == 0 || out_n == 0) return KH_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIPCHK0(hipSetDevice(device));
  Scratch s(device, stream);
  const uint8_t* din = nullptr; const uint32_t *dlo = nullptr, *dhi = nullptr; const uint64_t* ddst = nullptr; uint8_t* dout = nullptr;
  if (!s.layout([&](Scratch& c) {
        din = c.in(static_cast<const uint8_t*>(text), n, where); dlo = c.in(lo, n_rows, where); dhi = c.in(hi, n_rows, where); ddst = c.in(dst, n_rows, where);
        dout = c.inout(out, out_n, where);
      })) return s.finish();
  hipLaunchKernelGGL(k_pack_rows, dim3(grid_for(n_rows, KFQ_WAVES, (uint32_t)cu_count(device) * 8)), dim3(KFQ_THREADS), 0, stream, din, n, dlo, dhi, ddst, (uint32_t)n_rows, sep,
                     dout, out_n);
  s.launched();
  s.copy_back(dout, out_n);
  return s.finish_queued();
}
}  // extern "C"
