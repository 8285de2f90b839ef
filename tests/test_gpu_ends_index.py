"""GPU: ix.chain_ends end to end on both index classes: a random reference of a few thousand bases, reads of 150 bases with substitutions
and an insertion or deletion in their first and last 20 bases, forward and reverse.  For every kept chain with a whole-chain alignment,
read_cigar parses, its clips and query bases add up to the read, and applied to the read it reproduces, base by base, the reference
interval extended_intervals names -- reverse-complemented for a reverse chain.  chains, chain_edits and chain_cigars return what they
return without the new call."""
import os
import random
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import cigar_model as CM  # noqa: E402
from edits_cases import bases, other, revcomp  # noqa: E402
from stream_checks import to_dev  # noqa: E402

READ = 150
BACK = {"I": CM.OP_I, "D": CM.OP_D, "=": CM.OP_EQ, "X": CM.OP_X}


def make_reads(n_reads=24, ref_len=4000, seed=9):
    rng = random.Random(seed)
    ref = bases(rng, ref_len)
    reads = []
    for t in range(n_reads):
        p = rng.randrange(0, ref_len - READ - 4)
        r = bytearray(ref[p:p + READ + 4])
        for x in (rng.randrange(4, 20), rng.randrange(READ - 20, READ - 4)):      # one substitution in either end
            r[x] = other(rng, r[x])
        for x in (rng.randrange(6, 18), rng.randrange(READ - 18, READ - 6)):      # and an indel in some
            if t % 3 == 0:
                del r[x]
            elif t % 3 == 1:
                r.insert(x, rng.choice(b"ACGT"))
        r = bytes(r[:READ])
        reads.append(revcomp(r) if t & 1 else r)
    seq = b"\n".join(reads) + b"\n"
    starts = np.arange(n_reads, dtype=np.int64) * (READ + 1)
    return ref, seq, starts


@pytest.mark.parametrize("cls,k", [("KmerPositionIndex", 15), ("WideKmerPositionIndex", 35)])
@pytest.mark.parametrize("dev", [False, True])
def test_chain_ends_of_planted_reads(cls, k, dev):
    ref, seq, starts = make_reads()
    ends_at = starts + READ                                          # the newline behind a read is no base of it
    ix = getattr(kh, cls)(k=k, stranded=True, **({"s": 25} if cls == "WideKmerPositionIndex" else {}))
    try:
        rt, qt = np.frombuffer(ref, dtype=np.uint8).copy(), np.frombuffer(seq, dtype=np.uint8).copy()
        mk = to_dev if dev else (lambda a: a)
        ix.build_sequences(mk(rt))
        params = dict(read_starts=starts, min_score=20, min_count=2)
        before = ix.chain_cigars(mk(qt), mk(rt), **params)
        table, edits, cig, ends = ix.chain_ends(mk(qt), mk(rt), read_ends=ends_at, clip_cost=2, **params)
        if dev:
            torch.cuda.synchronize()
            assert ends.offsets.dtype == torch.int64 and all(x.dtype == torch.int32 for x in (ends.q, ends.r, ends.edits, ends.clip, ends.ops))
        host = lambda x: x.cpu().numpy() if dev else np.asarray(x)          # noqa: E731
        # the three older results are what they are without the new call
        flat = lambda t, e, c: list(t[:8]) + list(t.anchors) + [t.chain] + list(e) + list(c)      # noqa: E731
        for a, b in zip(flat(*before), flat(table, edits, cig)):
            assert np.array_equal(host(a), host(b))
        seg, rev, over = host(table.seg), host(table.rev), host(edits.over)
        q0, q1, r0, r1 = kh.extended_intervals(table, ends)
        clip, eq = host(ends.clip).view(np.uint32), host(ends.q).view(np.uint32)
        n_rows, checked, extended, clipped, fwd = len(seg), 0, 0, 0, 0
        assert n_rows >= 12 and len(eq) == 2 * n_rows
        qc, rc = CM._codes(qt), CM._codes(rt)
        for row in range(n_rows):
            s = kh.read_cigar(cig, ends, table, row, k)
            if over[row]:
                assert s is None
                continue
            assert re.fullmatch(r"(\d+S)?(\d+[ID=X])+(\d+S)?", s), s
            parts = re.findall(r"(\d+)([SID=X])", s)
            assert all(a[1] != b[1] for a, b in zip(parts, parts[1:])), s
            lo, hi = int(starts[int(seg[row])]), int(ends_at[int(seg[row])])
            head_s = int(parts[0][0]) if parts[0][1] == "S" else 0
            tail_s = int(parts[-1][0]) if parts[-1][1] == "S" else 0
            assert (head_s, tail_s) == (int(clip[2 * row]), int(clip[2 * row + 1]))
            assert head_s + tail_s + sum(int(n) for n, o in parts if o in "=XI") == hi - lo == READ, (row, s)
            assert (int(q0[row]), int(q1[row])) == (lo + head_s, hi - tail_s), (row, s)
            assert 0 <= r0[row] <= r1[row] <= len(rt)
            A = [int(c) for c in qc[int(q0[row]):int(q1[row])]]
            Bc = CM._oriented(rc[int(r0[row]):int(r1[row])], int(rev[row]) & 1)
            w = CM.apply_ops(A, Bc, [(BACK[o], int(n)) for n, o in parts if o != "S"])
            assert w is not None and w[:2] == (len(A), len(Bc)), (row, s, w)
            checked += 1
            extended += int(eq[2 * row]) + int(eq[2 * row + 1]) > 0
            clipped += head_s + tail_s > 0
            fwd += int(rev[row]) & 1 == 0
        assert checked >= 12 and extended >= 8 and 0 < fwd < checked, (checked, extended, clipped, fwd)
    finally:
        ix.close()


def test_default_read_ends_and_refusals():
    ref, seq, starts = make_reads(6)
    ix = kh.KmerPositionIndex(k=15, stranded=True)
    try:
        rt, qt = np.frombuffer(ref, dtype=np.uint8).copy(), np.frombuffer(seq, dtype=np.uint8).copy()
        ix.build_sequences(rt)
        table, _, _, ends = ix.chain_ends(qt, rt, read_starts=starts, min_score=20, min_count=2)
        given = ix.chain_ends(qt, rt, read_starts=starts, read_ends=np.append(starts[1:], len(qt)), min_score=20, min_count=2)[3]
        assert all(np.array_equal(a, b) for a, b in zip(ends, given))      # the default: the next read's start, len(seq) for the last
        assert (ends.clip[1::2] >= 1).all()                                # ... which makes the newline a base of the read: a tail never aligns it
        with pytest.raises(ValueError, match="read_ends"):
            ix.chain_ends(qt, rt, read_starts=starts, read_ends=starts[:-1])
        with pytest.raises(ValueError, match="read_ends"):
            ix.chain_ends(qt, rt, read_starts=starts, read_ends=starts + len(qt))
    finally:
        ix.close()
    ix = kh.KmerPositionIndex(k=15)
    try:
        with pytest.raises(ValueError, match="stranded=True"):
            ix.chain_ends(b"ACGT" * 10, b"ACGT" * 10)
    finally:
        ix.close()
