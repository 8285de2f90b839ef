"""The k-mer position index sharded across the GPUs of one node (one process per GPU, torch.distributed): ShardedKmerPositionIndex.

The pattern of kmerhash_amd.dist.ShardedTable over a local KmerPositionIndex instead of a local table.  The two are siblings: both derive
from kmerhash_amd.dist.ShardExchange (the exchange helpers, the collectives counter, the failure protocol, host staging under gloo); no
table operation exists on the index.
    owner rank = dist_hash(key, seed 9876543) & (p-1)   (or % p); the local index hashes with its own seed (43)
    append : (key, position) pairs permuted into p segments with the position as the value (kh_shard_permute), counts exchanged, keys
             and positions SoA in ONE grouped payload launch, then the local kh_index_append of what arrived.  The result of an append
             depends on the set of pairs alone, so the order in which the peers' pairs arrive does not matter: the local index of rank r
             is the index of all pairs of all ranks whose key r owns.
    find   : keys permuted with vals = 0..n-1 (which gives `origin`), counts and keys exchanged, ONE local find of everything received
             (a CSR in receive order = grouped by source rank, so every source's share of the positions is contiguous), a second count
             exchange with the position totals per source (the status word of the local find with it), one grouped payload exchange
             that brings the per-key counts to their place in the permuted order and the segments concatenated by owner rank -- the
             CSR in permuted order --, and kh_csr_unpermute puts it into QUERY order.
Texts: every rank samples ITS text (all windows, the (w,k)-minimizers of an index made with w, or the closed syncmers of one made with
s) and appends the pairs; nothing is
stitched across two ranks' texts -- a window or a minimizer window never spans them, as it never spans two reads.

Collectives per call (p > 1, or KH_DIST_FORCE_COLLECTIVES=1), as `collectives` counts them ("reduce": an all-reduce(sum) of the call's
global numbers, the sum of the ranks' status words with them -- it closes the call the way a vote does):
    append / build (and the *_sequences / *_fastq forms) : 1 counts, 1 payload, 3 votes
    count                                               : 1 counts, 2 payload, 2 votes
    find / find_sequences                               : 2 counts, 2 payload, 2 votes
    erase                                               : 1 counts, 1 payload, 2 votes, 1 reduce
    erase_counts / drop_above / size / total / clear    : 1 reduce
With one rank and no KH_DIST_FORCE_COLLECTIVES=1 every method is the local call and nothing else.

Failure protocol: ShardExchange's, as ShardedTable has it.  A rank that fails locally keeps taking part in the collectives the call still has to run and sends
empty or zero payloads; every rank raises -- the failing rank its own exception, the others ShardPeerError; no rank waits without bound.
All calls are synchronous (the local find waits for its total anyway), so there is no late status: a vote or a reduce closes each call.
After a failed append the failing rank's local index is EMPTY (the contract of kh_index_append) while the others hold their share:
the global index is then undefined until a collective clear().

Batches are torch tensors on the backend's device (int64 keys -- rows of an (n, 2) tensor for a backend of 16-byte keys --, int32
positions) or numpy arrays, which are copied there; results are tensors on that device.  `backend` objects supply the device-specific
pieces so that the exchange logic runs on the CPU over gloo in the tests; the product backends are IndexGpuBackend and
WideIndexGpuBackend.  Not built here: pipelined pieces, kh_shard_plan_* use, a fused text -> pairs-by-rank front end, the
C++ RCCL library, stitching across ranks' texts, 64-bit positions, a sharded anchors() (a stranded backend stores and returns stamped
positions; orienting the hits is the caller's, kmerhash_amd.stamp_strand on its query and kmerhash_amd.anchors_from_csr)."""
import numpy as np

from .dist import DIST_SEED, GpuBackend, GpuSharding, ShardedTable, ShardExchange, ShardPeerError, WideGpuBackend, dist, torch  # noqa: F401


class IndexGpuBackend(GpuSharding):
    """local index = KmerPositionIndex on this rank's GPU (64-bit k-mers, k <= 32; w: minimizer sampling, s: closed syncmers); sharding =
    kh_shard_permute"""

    def __init__(self, device, k=31, canonical=True, hash="farm", seed=43, w=None, order_hash="murmur", order_seed=42, min_lf=0.35,
                 max_lf=0.8, dist_hash="murmur3avx64", dist_seed=DIST_SEED, s=None, stranded=False):
        """stranded: every rank stamps the pairs of ITS text with its pos_base (kmerhash_amd.stamp_strand) before the exchange, so the
        sharded index stores and find returns stamped positions ((pos_base + p) << 1) | rc(p); pos_base + len(text) <= 2^31"""
        self.index = self._make_index(k, canonical, hash, min_lf, max_lf, device, seed, w, order_hash, order_seed, s, stranded)
        self.stranded = bool(stranded)
        super().__init__(device, dist_hash, dist_seed)

    @staticmethod
    def _make_index(k, canonical, hash, min_lf, max_lf, device, seed, w, order_hash, order_seed, s, stranded=False):
        from .index import KmerPositionIndex
        return KmerPositionIndex(k, canonical, hash, min_lf, max_lf, device, seed, w=w, order_hash=order_hash, order_seed=order_seed, s=s,
                                 stranded=stranded)

    def stamp(self, text, pos, pos_base):
        """the stamped positions of this rank's pairs (a stranded backend): device text, device positions, this rank's pos_base"""
        from .kmers import stamp_strand
        return stamp_strand(self._text(text), pos, self.index.k, pos_base, self.device)

    def _text(self, text):
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(text, dtype=np.uint8)
        if isinstance(text, np.ndarray):
            text = torch.from_numpy(np.ascontiguousarray(text, dtype=np.uint8).copy())
        return text.to(self.torch_device)

    def text_pairs(self, text, fastq=False):
        """-> device (k-mers, positions) of this rank's text, sampled as the index samples"""
        from .kmers import kmers_from_sequence, minimizers_from_sequence
        x, t = self.index, self._text(text)
        if x.s is not None:
            return x._syncmers(t, fastq)
        if x.w is None:
            return kmers_from_sequence(t, x.k, x.canonical, self.device, _fastq=fastq, with_positions=True)
        return minimizers_from_sequence(t, x.k, x.w, x.canonical, x.order_hash, x.order_seed, self.device, _fastq=fastq)

    def csr_unpermute(self, counts_perm, pos_perm, origin):
        """kh_csr_unpermute.  pos_perm None: -> counts int32[n] in query order; else -> (offsets int64[n + 1], positions int32[total])"""
        n = counts_perm.numel()
        n_out = self.C.c_uint64()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if pos_perm is None:
            out = torch.empty(n, dtype=torch.int32, device=self.torch_device)
            st = self.K.lib().kh_csr_unpermute(counts_perm.data_ptr(), None, origin.data_ptr(), n, out.data_ptr(), None, None, 0,
                                               self.C.byref(n_out), self.device, stream)
            if st != self.K.KH_OK:
                raise self.K.KhError(st, "kh_csr_unpermute (counts)")
            return out
        offs = torch.empty(n + 1, dtype=torch.int64, device=self.torch_device)
        cap = pos_perm.numel()
        out = torch.empty(max(cap, 1), dtype=torch.int32, device=self.torch_device)
        st = self.K.lib().kh_csr_unpermute(counts_perm.data_ptr(), pos_perm.data_ptr(), origin.data_ptr(), n, None, offs.data_ptr(),
                                           out.data_ptr(), cap, self.C.byref(n_out), self.device, stream)
        if st != self.K.KH_OK or n_out.value != cap:
            raise self.K.KhError(st or self.K.KH_ERR_INVALID, "kh_csr_unpermute: the counts add up to %d positions, %d arrived" % (n_out.value, cap))
        return offs, out[:cap]


class WideIndexGpuBackend(IndexGpuBackend):
    """local index = WideKmerPositionIndex (16-byte k-mers, k <= 64; keys are (n, 2) int64 CUDA tensors); sharding = kh_wide_shard_permute.
    No minimizer sampling; s: closed syncmers.  The unpermute step never sees a key: it is the parent's."""
    key_words = 2

    def __init__(self, device, k=63, canonical=True, hash="farm", seed=43, min_lf=0.35, max_lf=0.8, dist_hash="murmur3avx64",
                 dist_seed=DIST_SEED, s=None, order_hash="murmur", order_seed=42, stranded=False):
        super().__init__(device, k, canonical, hash, seed, None, order_hash, order_seed, min_lf, max_lf, dist_hash, dist_seed, s, stranded)

    @staticmethod
    def _make_index(k, canonical, hash, min_lf, max_lf, device, seed, w, order_hash, order_seed, s, stranded=False):
        from .index import WideKmerPositionIndex
        return WideKmerPositionIndex(k, canonical, hash, min_lf, max_lf, device, seed, order_hash=order_hash, order_seed=order_seed, s=s,
                                     stranded=stranded)

    def text_pairs(self, text, fastq=False):
        from .wide import kmers128_from_sequence
        x = self.index
        if x.s is not None:
            return x._syncmers(self._text(text), fastq)
        return kmers128_from_sequence(self._text(text), x.k, x.canonical, self.device, _fastq=fastq, with_positions=True)


class ShardedKmerPositionIndex(ShardExchange):
    """k-mer -> ascending positions of ALL its occurrences in the texts of all ranks.  Every method is COLLECTIVE: every rank calls
    it, each with its own batch, which may be empty.  Test hook: `_fail_stage` = 1..4 makes the next append / count / find / erase
    fail locally at that stage (1: permute, 2: receive buffers, 3: exchange (append, erase) or local lookup (count, find), 4: local
    append / erase or the unpermute)."""

    def __init__(self, backend, group=None, timing=False):
        super().__init__(backend, group, timing)
        self.collectives["reduce"] = 0

    @property
    def local(self):
        return self.b.index

    def synchronize(self):
        """waits for the queued work of this rank (every call is closed by a vote or a reduce: there is no late status)"""
        if self.b.torch_device.type == "cuda":
            torch.cuda.synchronize(self.b.torch_device)

    # ---- plumbing ---------------------------------------------------------------------------------------
    def _keys(self, keys):
        if isinstance(keys, np.ndarray):
            keys = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64).copy())
        keys = keys.to(self.b.torch_device)
        if self.key_words == 2 and (keys.dim() != 2 or keys.shape[1] != 2):
            raise ValueError("16-byte keys: expected shape (n, 2), got %s" % (tuple(keys.shape),))
        return keys

    def _pos(self, pos):
        if isinstance(pos, np.ndarray):
            pos = torch.from_numpy(np.ascontiguousarray(pos).astype(np.uint32, copy=False).view(np.int32).copy())
        return pos.to(self.b.torch_device)

    # ---- append ------------------------------------------------------------------------------------------
    def append(self, keys, pos):
        """more (k-mer, position) pairs of this rank onto the global index; returns the number of pairs this rank gave"""
        return self._append(keys, pos, False, None)

    def build(self, keys, pos):
        """append onto an EMPTY global index (a rank whose local index holds anything fails the call on every rank)"""
        return self._append(keys, pos, True, None)

    def _append(self, keys, pos, must_be_empty, ex):
        if self._single():
            if ex is not None:
                raise ex
            with self._span("local_append"):
                return (self.local.build if must_be_empty else self.local.append)(self._keys(keys), self._pos(pos))

        def batch():
            k, q = self._keys(keys), self._pos(pos)
            if q.numel() != k.shape[0]:
                raise ValueError("keys and positions must have the same length")
            if must_be_empty and self.local.total() != 0:
                raise ValueError("build: the index is not empty (clear() first, or append)")
            return k, q
        # ---- stages 1..3: the pairs grouped by owner rank, keys and positions SoA in one grouped launch
        x = self._to_owners(batch, ex, sent="while the pairs were exchanged; nothing was appended on any rank")
        ex = None                                                 # (no rank has failed so far, or _to_owners had raised)
        # ---- stage 4: the local append of what arrived
        try:
            self._inject(4)
            if x.rk.shape[0]:
                with self._span("local_append"):
                    self.local.append(x.rk, x.rv)
        except Exception as e:
            ex = e
        self._vote(ex, "in the local append: the failing rank's index is empty, the global index is undefined until a collective clear()")
        return x.pk.shape[0]

    def _text_pairs(self, text, pos_base, fastq, query=False):
        """(k-mers, positions + pos_base, None) of this rank's text, or (None, None, the exception).  A stranded backend stamps the
        positions instead ((pos_base + p) << 1 | rc(p)), except those of a query text, which stay plain offsets"""
        try:
            pos_base = int(pos_base)
            stranded = bool(getattr(self.b, "stranded", False)) and not query
            top = 31 if stranded else 32
            if not 0 <= pos_base or pos_base + len(text) > 2 ** top:
                raise ValueError("pos_base + len(text) must stay within 2^%d (%s), got %d + %d"
                                 % (top, "a stamped position has 31 bits" if stranded else "positions are 32-bit", pos_base, len(text)))
            if stranded:
                text = self.b._text(text)                         # (on the device once: sampled and stamped from the same copy)
            with self._span("text_pairs"):
                km, pos = self.b.text_pairs(text, fastq)
            if stranded:
                with self._span("text_pairs"):
                    pos = self.b.stamp(text, pos, pos_base)
            elif pos_base:
                pos = pos + (pos_base - (1 << 32) if pos_base >= (1 << 31) else pos_base)      # (32-bit positions in an int32 tensor)
            return km, pos, None
        except Exception as e:
            return None, None, e

    def _append_text(self, text, pos_base, fastq, must_be_empty):
        km, pos, ex = self._text_pairs(text, pos_base, fastq)
        return self._append(km, pos, must_be_empty, ex)

    def append_sequences(self, text, pos_base=0):
        """the windows (or, for an index made with w, the minimizers) of this rank's text onto the global index, position = pos_base +
        byte offset in `text`; returns the number of pairs this rank gave.  Nothing is stitched across the texts of two ranks."""
        return self._append_text(text, pos_base, False, False)

    def append_fastq(self, text, pos_base=0):
        """the same over raw FASTQ text (whole 4-line records)"""
        return self._append_text(text, pos_base, True, False)

    def build_sequences(self, text, pos_base=0):
        return self._append_text(text, pos_base, False, True)

    def build_fastq(self, text, pos_base=0):
        return self._append_text(text, pos_base, True, True)

    # ---- lookup ------------------------------------------------------------------------------------------
    def count(self, keys):
        """occurrences of every query key over all ranks (int32 tensor holding uint32; 0 on a miss), in QUERY order"""
        return self._lookup(keys, False, None)

    def find(self, keys):
        """-> (offsets int64[n + 1], positions): the CSR of KmerPositionIndex.find in QUERY order -- the positions of query i are
        positions[offsets[i]:offsets[i + 1]], ascending, over the texts of all ranks; a repeated key repeats its positions"""
        return self._lookup(keys, True, None)

    def find_sequences(self, text):
        """this rank's query text sampled as the index samples, then find: -> (qpos, offsets, positions)"""
        km, qpos, ex = self._text_pairs(text, 0, False, query=True)
        offsets, positions = self._lookup(km, True, ex)
        return qpos, offsets, positions

    def _lookup(self, keys, want_pos, ex):
        if self._single():
            if ex is not None:
                raise ex
            with self._span("local_query"):
                return self.local.find(self._keys(keys)) if want_pos else self.local.count(self._keys(keys))

        def batch():
            k = self._keys(keys)
            if k.shape[0] >= 2 ** 31:
                raise ValueError("a query batch holds fewer than 2^31 keys")
            return k, None
        # ---- stages 1, 2 and the keys out: grouped by owner rank; the value that travels with a key through the permutation is its
        #      index in the caller's batch (origin)
        x = self._to_owners(batch, ex, origin=True, more=lambda pk: self.b.empty(pk.shape[0], torch.int32))
        p, ex, origin, cperm = self.p, None, x.pv, x.more
        sc, so, rkeys, rcounts, ro = x.sc, x.so, x.rk, x.rc, x.ro
        rtot = sum(rcounts)
        # ---- stage 3 (local): ONE lookup of everything received.  Receive order is grouped by source rank, so the positions of every
        #      source are one contiguous stretch of the local CSR.  A failure is kept; the rank goes on with zero counts and no positions
        lc, lpos, ptot = None, None, [0] * p
        try:
            self._inject(3)
            with self._span("local_query"):
                if not want_pos:
                    lc = self.local.count(rkeys) if rtot else self.b.empty(0, torch.int32)
                elif rtot:
                    offs, lpos = self.local.find(rkeys)
                    lc = (offs[1:] - offs[:-1]).to(torch.int32)
                    bnd = offs[torch.tensor(ro + [rtot], dtype=torch.int64, device=offs.device)].cpu().tolist()
                    ptot = [int(bnd[s + 1] - bnd[s]) for s in range(p)]
                    lpos = lpos[:bnd[-1]]
        except Exception as e:
            ex = e
            ptot = [0] * p
        if ex is not None or lc is None:                          # failed, or nothing was received
            lc = torch.zeros(rtot, dtype=torch.int32, device=rkeys.device)
            lpos = self.b.empty(0, torch.int32)
        arrays = [(lc, ro, rcounts, cperm, so, sc)]
        status_in = pos_perm = None
        if want_pos:
            # the position totals per source, the status word of the local find with them
            rc2, worst = self._exchange_counts([[ptot[s]] for s in range(p)], ex)
            pcounts = [rc2[o][0] for o in range(p)]               # what every owner sends here: the segments of its share of the keys
            pos_perm = self.b.empty(sum(pcounts), torch.int32)
            arrays.append((lpos, self._offs(ptot), ptot, pos_perm, self._offs(pcounts), pcounts))
        else:
            _, status_in, words = self._words(ex, rkeys.device)
            arrays.append(words)
        # the per-key counts to their place in the permuted order, the segments concatenated by owner rank: the permuted-order CSR
        with self._span("exchange"):
            self._exchange(arrays)
        if not want_pos:
            worst = int(status_in.max().item())
        # ---- stage 4 (local): query order
        out = None
        if ex is None and not worst:
            try:
                self._inject(4)
                with self._span("unpermute"):
                    out = self.b.csr_unpermute(cperm, pos_perm, origin)
            except Exception as e:
                ex = e
        where = "in the lookup; no rank has results"
        self._vote(ex, where)                                     # (a peer's failure in its local lookup reaches every rank here)
        if worst:
            raise ShardPeerError(worst, where)
        return out

    # ---- erase -------------------------------------------------------------------------------------------
    def erase(self, keys):
        """every occurrence of the given k-mers out of the global index -> GLOBAL (distinct keys erased, positions erased)"""
        if self._single():
            return self.local.erase(self._keys(keys))
        x = self._to_owners(lambda: (self._keys(keys), None), sent="while the keys were exchanged; nothing was erased on any rank")
        ex = None
        nk = npos = 0
        try:
            self._inject(4)
            if x.rk.shape[0]:
                with self._span("local_erase"):
                    nk, npos = self.local.erase(x.rk)
        except Exception as e:
            ex = e
        return tuple(self._reduce([nk, npos], ex, "in the local erase: the ranks that did not fail erased their share"))

    def _local_then_reduce(self, fn, where):
        if self._single():
            return fn()
        ex, vals = None, None
        try:
            vals = fn()
        except Exception as e:
            ex = e
        return tuple(self._reduce(vals if vals is not None else (0, 0), ex, where))

    def erase_counts(self, lo, hi):
        """every k-mer whose GLOBAL number of occurrences lies in [lo, hi] out of the index -> global (keys erased, positions erased).
        A k-mer lives whole on its owner rank, so its occurrence count is local and exact: nothing is exchanged."""
        return self._local_then_reduce(lambda: self.local.erase_counts(lo, hi), "in erase_counts: the ranks that did not fail erased their share")

    def drop_above(self, max_occ):
        """mask repeats: every k-mer that occurs more than max_occ times over all ranks -> global (keys erased, positions erased)"""
        return self._local_then_reduce(lambda: self.local.drop_above(max_occ), "in drop_above: the ranks that did not fail erased their share")

    # ---- state -------------------------------------------------------------------------------------------
    def size(self):
        """distinct k-mers over all ranks"""
        return self._local_then_reduce(lambda: (self.local.size(),), "in size")[0]

    def total(self):
        """positions over all ranks"""
        return self._local_then_reduce(lambda: (self.local.total(),), "in total")[0]

    def local_size(self):
        return self.local.size()

    def clear(self):
        """every rank's local index emptied (collective: the way out of a failed append)"""
        def fn():
            self.local.clear()
            return ()
        self._local_then_reduce(fn, "in clear")
