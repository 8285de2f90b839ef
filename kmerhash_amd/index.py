"""k-mer position index (kh_index in include/kmerhash_amd.h): k-mer -> ALL its positions, built on the GPU.

The PositionIndex shape of the reference's driver (BenchmarkKmerIndex.cpp:342-449, over kmerind's multimap, which is not part of the
reference tree): built from (k-mer, position) pairs or straight from sequence / FASTQ text, queried, and changed batch by batch
(append*, erase, erase_counts, drop_above).
numpy arrays are host buffers, torch CUDA tensors device buffers, as in kmerhash_amd.table; results come back in the same kind of
container.  There is no CPU fallback."""
import ctypes as C

import numpy as np

from . import mapper
from ._call import HOST, _Buf, _Handle, alloc, check_same, torch
from ._xp import namespace_of
from .mapper import ChainTable, ReadLayout, anchors_from_csr, group_anchors, read_segments, stamp_strand  # noqa: F401  (ChainTable re-exported)
from .seqs import is_syncmer, is_syncmer128, kmers_from_sequence, minimizers_from_sequence, syncmers128_from_sequence, syncmers_from_sequence
from .table import _hash_id

# entries of positions a workgroup of the build sorts in LDS at a time (KI_SORT_TILE in csrc/kh_kernels_index.h): a segment that crosses
# a multiple of it takes the radix path
SORT_TILE = 4096


class KmerPositionIndex(_Handle):
    """k-mer -> ascending positions of all its occurrences.  64-bit k-mers (k <= 32), one GPU."""
    PREFIX = "kh_index_"          # the C entry points of this key width
    KMAX = 32
    WORDS = 1                     # 64-bit words per key

    def __init__(self, k=31, canonical=True, hash="farm", min_load_factor=0.35, max_load_factor=0.8, device=0, seed=43,
                 w=None, order_hash="murmur", order_seed=42, s=None, stranded=False):
        """w: index the (w,k)-minimizers of a text instead of all its windows (kmerhash_amd.minimizers_from_sequence: of every w
        consecutive windows the one whose k-mer has the smallest order_hash(k-mer, order_seed), about 2 / (w + 1) of them);
        build_sequences, build_fastq, append_sequences, append_fastq and find_sequences then sample with it.  None: every window.
        s: index the closed syncmers instead (kmerhash_amd.syncmers_from_sequence: the k-mers whose smallest s-mer by
        order_hash(s-mer, order_seed) is their first or last, about 2 / (k - s + 1) of them; s = 1..min(k, 32)).  Selection is a function
        of the k-mer alone, so it works for either key width and sampled(keys) can tell what the index can hold.  Not together with w.
        stranded: every text form (build_sequences, build_fastq, append_sequences, append_fastq, with or without a sampler) stores
        STAMPED positions ((pos_base + p) << 1) | rc(p) instead of p -- rc(p) = 1 where the canonical k-mer is the reverse complement of
        the window at p (kmerhash_amd.stamp_strand) --, find / export / find_sequences return them (kmerhash_amd.unstamp splits them) and
        anchors(seq) gives oriented hits.  Needs canonical=True; the coordinate space is 2^31; build / append over caller-supplied pairs
        store what the caller gives."""
        if stranded and not canonical:
            raise ValueError("stranded=True needs canonical=True: the strand bit says which strand the canonical k-mer came from")
        self.stranded = bool(stranded)
        if not 1 <= int(k) <= self.KMAX:
            raise ValueError("k must be 1..%d, got %r" % (self.KMAX, k))
        if s is not None:
            if w is not None:
                raise ValueError("s (closed syncmers) and w (minimizers) are two samplers: give one of them")
            if not 1 <= int(s) <= min(int(k), 32):
                raise ValueError("s must be 1..min(k, 32) or None, got %r" % (s,))
        self.s = None if s is None else int(s)
        if w is not None:
            if self.WORDS != 1:
                raise ValueError("minimizer sampling (w=) is not supported for 16-byte k-mers: use KmerPositionIndex (k <= 32)")
            if not 1 <= int(w) <= 256:
                raise ValueError("w must be 1..256 or None, got %r" % (w,))
        self.w = None if w is None else int(w)
        self.order_hash, self.order_seed = _hash_id(order_hash), int(order_seed)
        self.k, self.canonical, self.device = int(k), bool(canonical), int(device)
        self._create(_hash_id(hash), seed, min_load_factor, max_load_factor, self.device)
        if self.stranded:
            self._chk(self._fn("set_stranded")(self._h, 1))

    # -- plumbing --------------------------------------------------------------------------------
    def _pairs(self, keys, pos):
        """a batch of (k-mer, position) pairs, the current stream adopted"""
        kb, pb = _Buf.keys(keys, self.WORDS), _Buf(pos, np.uint32)
        check_same("keys and positions must have the same length and live in the same memory", kb, pb)
        self._adopt_stream(kb, pb)
        return kb, pb

    def _query(self, keys):
        """a key batch, the current stream adopted"""
        q = _Buf.keys(keys, self.WORDS)
        self._adopt_stream(q)
        return q

    # -- build -----------------------------------------------------------------------------------
    def build(self, keys, pos):
        """(k-mer, position) pairs in any order: uint64 keys and uint32 positions, both numpy or both CUDA tensors.  The index must
        be empty (clear() first); duplicate pairs are kept."""
        kb, pb = self._pairs(keys, pos)
        self._chk(self._fn("build")(self._h, kb.ptr, pb.ptr, kb.n, kb.where))
        return kb.n

    def _build_text(self, fn, text, *more):
        b = _Buf.text(text)
        self._adopt_stream(b)
        if self.w is not None or self.s is not None:      # the same four calls over the minimizers / closed syncmers of the text
            verb, _, form = fn.partition("_from_")
            sampler, arg = ("_from_minimizers", self.w) if self.s is None else ("_from_syncmers", self.s)
            self._chk(self._fn(verb + sampler)(self._h, b.ptr, b.n, self.k, arg, 1 if self.canonical else 0, self.order_hash,
                                               self.order_seed, b.where, 1 if form == "fastq" else 0, *more))
            return self.total()
        self._chk(self._fn(fn)(self._h, b.ptr, b.n, self.k, 1 if self.canonical else 0, b.where, *more))
        return self.total()

    def build_sequences(self, seq):
        """every window of k valid bases of `seq` with its byte offset in `seq`; returns the number of positions indexed"""
        return self._build_text("build_from_sequence", seq)

    def build_fastq(self, text):
        """the same over raw FASTQ text (whole 4-line records); positions are byte offsets into the text"""
        return self._build_text("build_from_fastq", text)

    def clear(self):
        self._chk(self._fn("clear")(self._h))

    # -- change a built index --------------------------------------------------------------------
    def append(self, keys, pos):
        """more (k-mer, position) pairs onto an index in any state (on an empty one: build).  Afterwards the index is that of all pairs
        given so far; the table is laid out like a counting table fed the same batches one by one."""
        kb, pb = self._pairs(keys, pos)
        self._chk(self._fn("append")(self._h, kb.ptr, pb.ptr, kb.n, kb.where))
        return kb.n

    def _base(self, pos_base):
        top = 31 if self.stranded else 32                     # (a stamped position has 31 bits)
        if not 0 <= int(pos_base) < 2 ** top:
            raise ValueError("pos_base must be 0..2^%d-1, got %r" % (top, pos_base))
        return int(pos_base)

    def append_sequences(self, seq, pos_base=0):
        """every window of `seq` onto the index, its position = pos_base + byte offset in `seq`; returns the positions indexed so far"""
        return self._build_text("append_from_sequence", seq, self._base(pos_base))

    def append_fastq(self, text, pos_base=0):
        """the same over raw FASTQ text (whole 4-line records)"""
        return self._build_text("append_from_fastq", text, self._base(pos_base))

    def erase(self, keys):
        """every occurrence of the given k-mers out of the index (misses and repeats are harmless) -> (distinct keys erased, positions erased)"""
        q = self._query(keys)
        nk, npos = C.c_uint64(), C.c_uint64()
        self._chk(self._fn("erase")(self._h, q.ptr, q.n, q.where, C.byref(nk), C.byref(npos)))
        return nk.value, npos.value

    def erase_counts(self, lo, hi):
        """every k-mer whose number of occurrences lies in the closed range [lo, hi] out of the index (lo > hi: the empty range)
        -> (distinct keys erased, positions erased)"""
        for v in (lo, hi):
            if not 0 <= int(v) < 2 ** 32:
                raise ValueError("occurrence counts are 0..2^32-1, got %r" % (v,))
        nk, npos = C.c_uint64(), C.c_uint64()
        self._chk(self._fn("erase_counts")(self._h, int(lo), int(hi), C.byref(nk), C.byref(npos)))
        return nk.value, npos.value

    def drop_above(self, max_occ):
        """mask repeats: every k-mer that occurs more than max_occ times out of the index -> (keys erased, positions erased)"""
        if int(max_occ) >= 2 ** 32 - 1:
            return 0, 0
        return self.erase_counts(int(max_occ) + 1, 2 ** 32 - 1)

    # -- state -----------------------------------------------------------------------------------
    def size(self):
        """distinct k-mers"""
        return self._scalar("size")

    def total(self):
        """positions (= pairs the index was built from)"""
        return self._scalar("total")

    def capacity(self):
        return self._scalar("capacity")

    def __len__(self):
        return self.size()

    def export(self):
        """(keys uint64[size] in slot order, offsets uint32[size + 1], positions uint32[total]) as numpy arrays: the positions of
        keys[r] are positions[offsets[r]:offsets[r + 1]], ascending"""
        size, total = self.size(), self.total()
        keys, kptr = alloc(HOST, size if self.WORDS == 1 else (size, self.WORDS), np.uint64)
        offsets, optr = alloc(HOST, size + 1, np.uint32)
        positions, pptr = alloc(HOST, total, np.uint32)
        self._chk(self._fn("export")(self._h, kptr, optr, pptr))
        return keys, offsets, positions

    # -- lookup ----------------------------------------------------------------------------------
    def count(self, keys):
        """occurrences of every query key (uint32; 0 on a miss)"""
        q = self._query(keys)
        out, optr = alloc(q, q.n, np.uint32, zero=True)
        self._chk(self._fn("count")(self._h, q.ptr, q.n, q.where, optr))
        return out

    def find(self, keys, positions=True, cap_out=None):
        """-> (offsets, positions): a CSR in query order -- offsets has len(keys) + 1 entries (uint64 / int64), the positions of query i
        are positions[offsets[i]:offsets[i + 1]], ascending; a repeated key repeats its positions.  positions=False: offsets only
        (positions is None).  cap_out: room to offer for the positions (default: exactly what is needed, found by an offsets-only pass);
        too little raises KhError(KH_ERR_INVALID)."""
        q = self._query(keys)
        n_out = C.c_uint64()
        offs, optr = alloc(q, q.n + 1, np.uint64, zero=True)
        if not positions or cap_out is None:
            self._chk(self._fn("find")(self._h, q.ptr, q.n, q.where, optr, None, 0, C.byref(n_out)))
            if not positions:
                return offs, None
            cap_out = n_out.value
        cap_out = int(cap_out)
        out, pptr = alloc(q, max(cap_out, 1), np.uint32)
        self._chk(self._fn("find")(self._h, q.ptr, q.n, q.where, optr, pptr, cap_out, C.byref(n_out)))
        return offs, out[: n_out.value]

    def find_sequences(self, seq):
        """the index's own sampling of a query text, then find: -> (qpos, offsets, positions).  The k-mers of `seq` are taken with
        the index's k, canonical flag and -- when it was made with w or s -- that sampler, order hash and order seed (all windows otherwise);
        qpos[i] is the byte offset in `seq` of query k-mer i and positions[offsets[i]:offsets[i + 1]] are its occurrences in the index.
        Two device calls composed here; numpy in, numpy out, CUDA tensor in, tensors out.  On a stranded index the positions are the
        stamped values (qpos stays a plain offset); anchors(seq) returns them oriented."""
        km, qpos = self._sample(seq)
        offsets, positions = self.find(km)
        return qpos, offsets, positions

    def _sample(self, seq):
        """(k-mers, window offsets) of a query text, sampled as the index samples"""
        if self.WORDS != 1 and self.s is None:
            raise ValueError("find_sequences is not supported for 16-byte k-mers without s")
        if self.s is not None:
            return self._syncmers(seq)
        if self.w is None:
            return kmers_from_sequence(seq, self.k, self.canonical, self.device, with_positions=True)
        return minimizers_from_sequence(seq, self.k, self.w, self.canonical, self.order_hash, self.order_seed, self.device)

    def anchors(self, seq):
        """oriented hits of a query text on a stranded index -> (qpos, rpos, rev), one entry per hit, in query order and then ascending
        rpos: the query is sampled as find_sequences samples it, its positions are stamped over the query text, looked up, and the CSR
        is expanded on the device (kh_anchors_from_csr).  rev[j] == 0: the k bases at rpos[j] in the indexed text equal those at qpos[j]
        in `seq`; rev[j] == 1: they are their reverse complement.  numpy in, numpy out (uint32, uint32, uint8); a CUDA tensor in, tensors
        out (int32, int32, uint8) on the current stream.  chains(seq) chains them per read."""
        self._need_stranded("anchors")
        seq = _Buf.text(seq).obj          # (bytes as an array: the text goes to two calls)
        km, qpos = self._sample(seq)
        sq = stamp_strand(seq, qpos, self.k, 0, self.device)
        offsets, positions = self.find(km)
        return anchors_from_csr(sq, offsets, positions, self.device)

    def anchor_groups(self, seq, read_starts=None, targets=None):
        """anchors(seq), then kmers.group_anchors: the anchors of every read (read_starts as chains() takes them; None: one read)
        regrouped by the target they fall in -> AnchorGroups.  targets: a kmerhash_amd.Targets (or a (starts, ends) pair)."""
        self._need_stranded("anchor_groups")
        if targets is None:
            raise ValueError("anchor_groups() needs targets=")
        q, r, v = self.anchors(seq)
        return group_anchors(q, r, v, targets, self.k, read_segments(namespace_of(q), q, ReadLayout(read_starts, None, None)), self.device)

    def _need_stranded(self, name):
        """the refusal every call that orients its hits opens with"""
        if not self.stranded:
            raise ValueError("%s() needs an index made with stranded=True: without the strand bit a hit has no orientation" % name)

    def chains(self, seq, read_starts=None, targets=None, **params):
        """candidate loci of the reads in a query text on a stranded index: anchors(seq), then collinear chains per read on the device
        (kmers.chain_anchors with the index's k; params: lookback, max_gap, band, min_score, min_count).  read_starts: ascending byte
        offsets of the reads in `seq`, the first one 0 (None: one read); a chain never holds anchors of two reads.
        -> ChainTable(seg, rev, q_start, q_end, r_start, r_end, count, score, anchors, chain): one row per kept chain -- its read, its
        strand, the query interval [q_start, q_end) and the reference interval [r_start, r_end) its first and last anchor span, its
        number of anchors and its score -- then anchors = (qpos, rpos, rev) as anchors() returns them and chain[j] = the row of anchor
        j or -1.  numpy in, numpy out; a CUDA tensor in, tensors out on the current stream.
        targets: a kmerhash_amd.Targets when the index holds several sequences laid out by it (build_sequences(targets.text)): the
        anchors of every read are first regrouped by target (kmers.group_anchors) and chained per (read, target), so no chain crosses a
        contig; `anchors` are then the regrouped ones, seg stays the read, and targets.locate(r_start) names a row's target.  None:
        exactly the calls of an index of one sequence."""
        self._need_stranded("chains")
        return mapper.chains(self, seq, read_starts, targets, **params)

    def chain_edits(self, seq, ref_text, read_starts=None, ref_base=0, max_edits=31, targets=None, **params):
        """chains(seq, read_starts, **params), then every kept chain verified against the texts on the device: kmers.chain_edits over the
        chains' own anchors, with `seq` as the query text and ref_text as the text the index was built from -- the index keeps none;
        ref_text covers the indexed positions [ref_base, ref_base + len(ref_text)) and lives where seq lives.
        -> (ChainTable, ChainEdits(link, edits, over)): the table of chains(), the edit distance per anchor link (-1: no link, -2: outside
        the texts or more than max_edits, 0..31) and, per row of the table, the sum of its links' distances and the number of its -2
        links.  The chain's last seed adds k matching bases and no edits.
        targets: as for chains(); ref_text must then be targets.text (or a copy where seq lives) with ref_base 0."""
        self._need_stranded("chain_edits")
        return mapper.index_chain_edits(self, seq, ref_text, read_starts, ref_base, max_edits, targets, **params)

    def chain_cigars(self, seq, ref_text, read_starts=None, ref_base=0, max_edits=31, targets=None, **params):
        """chain_edits(seq, ref_text, ...), then the alignment behind every distance: kmers.chain_cigars over the same anchors and texts
        with the link array chain_edits wrote -> (ChainTable, ChainEdits, ChainCigars(offsets, ops, ins, dels)): a CSR of run-length rows in
        anchor order and the inserted and deleted bases per row of the table.  kmers.cigar_string(cigars, table, row, k) is the CIGAR
        of one chain as text.  targets: as for chain_edits()."""
        self._need_stranded("chain_cigars")
        return mapper.index_chain_cigars(self, seq, ref_text, read_starts, ref_base, max_edits, targets, **params)

    def chain_ends(self, seq, ref_text, read_starts=None, read_ends=None, ref_base=0, max_edits=31, clip_cost=4, targets=None, **params):
        """chain_cigars(seq, ref_text, ...), then both ends of every chain extended to the ends of its read or to a soft clip:
        kmers.chain_ends over the same anchors and texts, with the chains' first and last anchors and the byte interval of each chain's
        read -- [read_starts[seg], read_ends[seg]); read_ends defaults to the next read's start and len(seq) for the last read, so give
        it where the reads are separated by bytes that belong to none of them.
        -> (ChainTable, ChainEdits, ChainCigars, ChainEnds(q, r, edits, clip, offsets, ops)): rows 2c and 2c + 1 of the ends are the head
        and tail of row c of the table.  kmers.read_cigar(cigars, ends, table, row, k) is the CIGAR of a whole read,
        kmers.extended_intervals(table, ends) the intervals it maps.  targets: as for chain_edits(); an end never runs into a spacer:
        every spacer byte costs clip_cost and gains nothing."""
        self._need_stranded("chain_ends")
        return mapper.index_chain_ends(self, seq, ref_text, read_starts, read_ends, ref_base, max_edits, clip_cost, targets, **params)

    def map(self, seq, ref_text, read_starts=None, read_ends=None, ref_base=0, max_edits=31, clip_cost=4, mask_pct=50, pri_pct=80, best_n=5, ref_order=True,
            targets=None, **params):
        """the whole mapper in one call: chain_ends(seq, ref_text, ...), kmers.select_table over its table with one group per read, and
        kmers.chain_records over all of it -> Mapping(table, edits, cigars, ends, select, records): row c of table, select and records is
        one candidate alignment -- its read, strand and intervals, whether it is the read's primary and how sure, and its CIGAR as a
        row of runs with the PAF numbers beside it.  ref_order (default True): the CIGAR rows of reverse-strand chains run in reference
        order, as PAF and SAM want them; False gives read order, what kmers.read_cigar() prints.  kmers.write_paf() writes the lines.
        targets: a kmerhash_amd.Targets for an index of several sequences (see chains()); ref_text is then targets.text, the rows of one
        read on different targets compete in select, and write_paf(..., targets=targets) names each row's target."""
        self._need_stranded("map")
        return mapper.map_reads(self, seq, ref_text, read_starts, read_ends, ref_base, max_edits, clip_cost, mask_pct, pri_pct, best_n, ref_order, targets, **params)

    def map_pairs(self, seq, ref_text, read_starts, read_ends=None, ref_base=0, max_edits=31, clip_cost=4, mask_pct=50, pri_pct=80, best_n=5,
                  min_ins=0, max_ins=1000, unpaired_pen=17, targets=None, **params):
        """paired reads: map(seq, ref_text, read_starts, ...) with ref_order=True over reads that are interleaved -- read 2p is mate 1 and
        read 2p + 1 mate 2 of fragment p, both as the sequencer gives them (a forward-reverse library) -- then kmers.pair_mapping over the
        Mapping -> (Mapping, PairSelect(row, mapq, tlen, flag, score, nconc)): per read the row that represents it in its pair, its
        quality and its template length; per pair whether it is proper.  min_ins / max_ins bound the fragment length of a concordant
        pair, unpaired_pen is what two unpaired best rows must win by.  An odd number of reads raises ValueError.
        write_sam_pairs() prints the mate columns."""
        self._need_stranded("map_pairs")
        return mapper.map_pairs(self, seq, ref_text, read_starts, read_ends, ref_base, max_edits, clip_cost, mask_pct, pri_pct, best_n, min_ins, max_ins, unpaired_pen,
                                targets, **params)

    def map_pairs_rescued(self, seq, ref_text, read_starts, read_ends=None, ref_base=0, max_edits=31, clip_cost=4, mask_pct=50, pri_pct=80, best_n=5,
                          min_ins=0, max_ins=1000, unpaired_pen=17, targets=None, **params):
        """map_pairs(seq, ref_text, read_starts, ...) with the same parameters, then mate rescue: kmers.rescue_requests over its result
        -- a mate that pairing left without a row, next to a partner that has one, is looked for where a concordant pair would put it --
        and kmers.rescue_mates over those requests, which aligns each such mate end to end inside its window on the device.
        -> (Mapping, PairSelect, MateRescue(read, edits, rs, re, rev, span, offsets, ops)): the first two are exactly what map_pairs
        returns; the third holds one entry per request, read = the number of the rescued read, edits >= 0 where it was placed within
        max_edits.  write_sam_rescued() prints such a read as mapped."""
        self._need_stranded("map_pairs")
        return mapper.map_pairs_rescued(self, seq, ref_text, read_starts, read_ends, ref_base, max_edits, clip_cost, mask_pct, pri_pct, best_n, min_ins, max_ins,
                                        unpaired_pen, targets, **params)

    def map_fastq(self, text, ref_text, strict=True, strip_mate=None, **kw):
        """FASTQ in: kmerhash_amd.read_fastq(text, strict=strict, strip_mate=strip_mate) where the text lives, then
        map(reads.seq, ref_text, reads.read_starts, reads.read_ends, **kw) -> (Mapping, Reads).  write_sam_bytes(fh, mapping, reads.seq,
        ref_text, reads.names, reads.read_starts, reads.read_ends, qual=reads.qual, ...) writes the file."""
        self._need_stranded("map")
        return mapper.map_fastq(self, text, ref_text, strict, strip_mate, **kw)

    def map_fastq_pairs(self, text, ref_text, text2=None, rescue=False, strict=True, strip_mate=None, **kw):
        """paired FASTQ in: read_fastq(text, text2, ...) -- text2=None: one interleaved file, mate 1, mate 2, ...; else the two files of a
        run, interleaved here, a closing /1 or /2 dropped from the names -- then map_pairs (rescue: map_pairs_rescued) with **kw
        -> (Mapping, PairSelect, Reads) or (Mapping, PairSelect, MateRescue, Reads).  An odd number of reads is the ValueError of map_pairs."""
        self._need_stranded("map_pairs")
        return mapper.map_fastq_pairs(self, text, ref_text, text2, rescue, strict, strip_mate, **kw)

    def chain_select(self, seq, read_starts=None, mask_pct=50, pri_pct=80, best_n=5, **params):
        """chains(seq, read_starts, **params), then which chain of every read is the answer: kmers.select_table over the table with one
        group per read -> (ChainTable, ChainSelect(parent, rank, mapq, flag, sub, nsub, best)): per row of the table its primary, its
        rank in its read, the mapping quality of a primary and the primary / kept flags; best[s] = the best row of read s, -1 for a read
        without chains.  The score is the chaining score; kmers.select_chains takes any other.  The keyword targets= (a
        kmerhash_amd.Targets, see chains()) travels with params: the rows of a read on different targets then compete with each other."""
        self._need_stranded("chain_select")
        return mapper.chain_select(self, seq, read_starts, mask_pct, pri_pct, best_n, **params)

    def _syncmers(self, seq, fastq=False):
        """the closed syncmers of a text under the index's own parameters"""
        return (syncmers_from_sequence if self.WORDS == 1 else syncmers128_from_sequence)(seq, self.k, self.s, self.canonical, self.order_hash, self.order_seed, self.device, _fastq=fastq)

    def sampled(self, keys):
        """bool per key: could the index hold it?  True for every key of an index of all windows; is_syncmer(keys) under the index's
        parameters for one made with s -- count(keys) == 0 then means "absent from the text" where sampled is True and "not sampled"
        where it is False.  An index made with w raises: a minimizer is chosen by its neighbours, not by the k-mer."""
        if self.w is not None:
            raise ValueError("sampled() has no answer for a minimizer index (w=): selection there depends on the neighbouring windows")
        q = _Buf.keys(keys, self.WORDS)
        if self.s is None:
            return torch.ones(q.n, dtype=torch.bool, device=q.device) if q.dev else np.ones(q.n, dtype=bool)
        return (is_syncmer if self.WORDS == 1 else is_syncmer128)(keys, self.k, self.s, self.canonical, self.order_hash, self.order_seed, self.device)

    # -- measurement -----------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._chk(self._fn("profile_enable")(self._h, 1 if on else 0))

    def profile(self):
        """{kernel name: (launches, total ms)} since profile_enable(True)"""
        return self._profile()


class WideKmerPositionIndex(KmerPositionIndex):
    """KmerPositionIndex over 16-byte k-mers (k = 1..64; kh_wide_index_*): keys are (n, 2) uint64 numpy arrays or (n, 2) int64 CUDA
    tensors, {w0, w1} per k-mer as kmerhash_amd.wide takes them; export() returns keys of shape (size, 2).  The keys that share a
    home bucket stand in ascending order of (w1 << 64) | w0."""
    PREFIX = "kh_wide_index_"
    KMAX = 64
    WORDS = 2

    def __init__(self, k=63, canonical=True, hash="farm", min_load_factor=0.35, max_load_factor=0.8, device=0, seed=43, w=None,
                 order_hash="murmur", order_seed=42, s=None, stranded=False):
        super().__init__(k, canonical, hash, min_load_factor, max_load_factor, device, seed, w=w, order_hash=order_hash, order_seed=order_seed, s=s,
                         stranded=stranded)

    def export_info(self):
        """the Robin Hood info byte of every bucket of the index's table (uint8[capacity]): the counting twin's"""
        info, ptr = alloc(HOST, self.capacity(), np.uint8)
        self._chk(self._L.kh_wide_index_export_info(self._h, ptr))
        return info
