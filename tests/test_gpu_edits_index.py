"""GPU: chain_edits of the index classes end to end: reads cut from a 20 kb reference, mutated at a known rate, forward and reverse, a
few with one indel.  ix.chain_edits equals the model of tests/edits_model.py run over the anchors of ix.chains with the pred of
chain_anchors; the table it returns is that of ix.chains; for reads with substitutions only, a chain's edits are the planted
substitutions between its first seed and its last."""
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import edits_model as EM  # noqa: E402
from stream_checks import to_dev  # noqa: E402

COMP = {65: 84, 67: 71, 71: 67, 84: 65}
INDEXES = {"syncmers": (lambda: kh.KmerPositionIndex(k=15, s=11, stranded=True), 0.02),
           "wide-syncmers": (lambda: kh.WideKmerPositionIndex(k=63, s=31, stranded=True), 0.004)}


def make_reads(rng, ref, rate, n_reads=50):
    """-> query text, read starts, planted substitution positions (query coordinates) per read, reads that hold an indel"""
    text, starts, subs, indel = bytearray(), [], [], set()
    for t in range(n_reads):
        n = rng.randrange(150, 301)
        p = rng.randrange(0, len(ref) - n)
        read = bytearray(ref[p:p + n])
        if t & 1:
            read = bytearray(COMP[b] for b in reversed(read))
        if t % 10 == 9:                                          # one indel in the middle
            indel.add(t)
            if t % 20 == 9:
                del read[n // 2]
            else:
                read.insert(n // 2, rng.choice(b"ACGT"))
        planted = []
        for i in range(len(read)):
            if rng.random() < rate:
                read[i] = rng.choice([c for c in b"ACGT" if c != read[i]])
                planted.append(len(text) + i)
        starts.append(len(text))
        subs.append(planted)
        text += read
    return np.frombuffer(bytes(text), dtype=np.uint8).copy(), np.array(starts, dtype=np.int64), subs, indel


@pytest.mark.parametrize("name", sorted(INDEXES))
def test_chain_edits_end_to_end(name):
    make, rate = INDEXES[name]
    rng = random.Random(31)
    ref = np.frombuffer(bytes(rng.choice(b"ACGT") for _ in range(20000)), dtype=np.uint8).copy()
    query, starts, subs, indel = make_reads(rng, bytes(ref), rate)
    ix = make()
    k = ix.k
    try:
        ix.build_sequences(ref)
        base = ix.chains(query, read_starts=starts)
        q, r, v = base.anchors
        seg = np.concatenate([np.searchsorted(q, starts, side="left"), [len(q)]]).astype(np.uint64)
        pred = kh.chain_anchors(q, r, v, k, seg).pred
        nc = len(base.count)
        exp = EM.chain_edits_model(query, ref, q, r, v, pred, base.chain, nc, k, 0, 31, banded=True)
        assert nc >= 20 and (exp[0] >= 0).sum() >= 3 * nc // 2 and (exp[0] > 0).sum() >= 10
        for dev in (False, True):
            host = (lambda x: x.cpu().numpy()) if dev else (lambda x: x)
            table, ed = ix.chain_edits(to_dev(query) if dev else query, to_dev(ref) if dev else ref, read_starts=starts)
            if dev:
                torch.cuda.synchronize()
            for f in ("seg", "rev", "q_start", "q_end", "r_start", "r_end", "count", "score", "chain"):
                assert np.array_equal(host(getattr(table, f)), getattr(base, f)), f
            for a, b in zip(table.anchors, base.anchors):
                assert np.array_equal(host(a).view(b.dtype), b)
            assert np.array_equal(host(ed.link), exp[0])
            assert np.array_equal(host(ed.edits).view(np.uint32), exp[1]) and np.array_equal(host(ed.over).view(np.uint32), exp[2])
        # substitutions only: what lies between the first seed and the last is A against B link by link, and every planted
        # substitution there costs one edit (a seed holds none: it matched)
        verified = strands = 0
        for c in range(nc):
            s = int(base.seg[c])
            if s in indel or exp[2][c]:
                continue
            lo, hi = int(base.q_start[c]), int(base.q_end[c]) - k
            assert exp[1][c] == sum(lo <= p < hi for p in subs[s]), (c, s, lo, hi)
            verified += 1
            strands |= 1 << int(base.rev[c])
        assert verified >= 15 and strands == 3
        # the reference text from position 5 on, with ref_base = 5: the same links, except where B would start below it
        cut = EM.chain_edits_model(query, ref[5:], q, r, v, pred, base.chain, nc, k, 5, 31, banded=True)
        _, ed = ix.chain_edits(query, ref[5:], read_starts=starts, ref_base=5)
        assert all(np.array_equal(x, y) for x, y in zip(ed, cut))
        assert ((cut[0] == exp[0]) | (cut[0] == EM.OVER)).all()
    finally:
        ix.close()
