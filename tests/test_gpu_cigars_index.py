"""GPU: ix.chain_cigars end to end on both index classes: a random reference of a few thousand bases, reads of 150 bases with
substitutions and one insertion or deletion each, forward and reverse.  For every kept chain without an over link, cigar_string parses,
consumes exactly the chain's query and reference interval, agrees with the two texts base by base in its '=' and X runs, and holds
as many edits as chain_edits counted."""
import os
import random
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


def make_reads(n_reads=24, ref_len=4000, seed=5):
    rng = random.Random(seed)
    ref = bases(rng, ref_len)
    reads = []
    for t in range(n_reads):
        p = rng.randrange(0, ref_len - READ - 2)
        r = bytearray(ref[p:p + READ + 2])
        for x in rng.sample(range(5, READ - 5), 3):
            r[x] = other(rng, r[x])
        x = rng.randrange(40, READ - 40)
        if t % 3 == 0:
            del r[x]                                             # a base of the reference missing in the read
        elif t % 3 == 1:
            r.insert(x, rng.choice(b"ACGT"))                     # a base more in the read
        r = bytes(r[:READ])
        reads.append(revcomp(r) if t & 1 else r)
    seq = b"\n".join(reads) + b"\n"
    starts = np.arange(n_reads, dtype=np.int64) * (READ + 1)
    return ref, seq, starts


@pytest.mark.parametrize("cls,k", [("KmerPositionIndex", 15), ("WideKmerPositionIndex", 35)])
@pytest.mark.parametrize("dev", [False, True])
def test_chain_cigars_of_planted_reads(cls, k, dev):
    ref, seq, starts = make_reads()
    ix = getattr(kh, cls)(k=k, stranded=True, **({"s": 25} if cls == "WideKmerPositionIndex" else {}))
    try:
        rt, qt = np.frombuffer(ref, dtype=np.uint8).copy(), np.frombuffer(seq, dtype=np.uint8).copy()
        ix.build_sequences(to_dev(rt) if dev else rt)
        table, edits, cig = ix.chain_cigars(to_dev(qt) if dev else qt, to_dev(rt) if dev else rt, read_starts=starts, min_score=20, min_count=2)
        if dev:
            torch.cuda.synchronize()
            assert cig.offsets.dtype == torch.int64 and cig.ops.dtype == torch.int32
        host = lambda x: x.cpu().numpy() if dev else x          # noqa: E731
        rev, qs, qe, rs, re_, over, ed = (host(x) for x in (table.rev, table.q_start, table.q_end, table.r_start, table.r_end, edits.over, edits.edits))
        n_rows, checked, with_indel = len(qs), 0, 0
        assert n_rows >= 12
        qc, rc = CM._codes(qt), CM._codes(rt)
        for row in range(n_rows):
            s = kh.cigar_string(cig, table, row, k)
            if over[row]:
                assert s is None
                continue
            runs = CM.parse(s)
            assert all(a[0] != b[0] for a, b in zip(runs, runs[1:]))
            A = [int(c) for c in qc[int(qs[row]):int(qe[row])]]
            Bc = CM._oriented(rc[int(rs[row]):int(re_[row])], int(rev[row]) & 1)
            w = CM.apply_ops(A, Bc, runs)
            assert w is not None, (row, s)
            assert w[:2] == (len(A), len(Bc)) and sum(w[2:]) == int(ed[row].view(np.uint32) if dev else ed[row]), (row, s, w)
            assert (w[3], w[4]) == (int(host(cig.ins)[row]), int(host(cig.dels)[row]))
            checked += 1
            with_indel += w[3] + w[4] > 0
        assert checked >= 12 and with_indel >= 4
    finally:
        ix.close()


def test_chain_cigars_needs_a_stranded_index():
    ix = kh.KmerPositionIndex(k=15)
    try:
        with pytest.raises(ValueError, match="stranded=True"):
            ix.chain_cigars(b"ACGT" * 10, b"ACGT" * 10)
    finally:
        ix.close()
