"""GPU: index.chain_select end to end.  A reference of 7 kb holds one 1000-base segment three times: exact (at 1000), with 2 %
substitutions (at 2600) and reverse-complemented (at 4200).  Reads of 600 bases drawn from the segment come back with one primary --
the exact copy: the reverse-complemented one scores the same and has the larger chain number -- two kept secondaries and a low mapping
quality; reads from unique sequence, on either strand, with one primary of quality 60; a read of random bases with best = -1.  The
numpy and the tensor form equal tests/select_model.py over the returned table, and chains() over the same input returns what it
returned.  pri_pct = 50 here: how much of the score the 2 % copy keeps depends on where the seeds fall."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from select_model import NAMES, select_model  # noqa: E402
from stream_checks import to_dev  # noqa: E402

COMP = bytes.maketrans(b"ACGT", b"TGCA")
SEG, EXACT, SUBST, RC, READ = 1000, 1000, 2600, 4200, 600
INDEXES = {"syncmers": lambda: kh.KmerPositionIndex(k=15, s=11, stranded=True), "wide": lambda: kh.WideKmerPositionIndex(k=33, s=27, stranded=True)}


def revcomp(b):
    return bytes(b).translate(COMP)[::-1]


@pytest.fixture(scope="module")
def texts():
    rng = np.random.default_rng(17)
    ref = bytearray(rng.choice(list(b"ACGT"), 7000).astype(np.uint8).tobytes())
    seg = bytes(ref[EXACT:EXACT + SEG])
    sub = bytearray(seg)
    for p in rng.choice(SEG, SEG // 50, replace=False):      # 2 %
        sub[p] = b"ACGT"[(b"ACGT".index(sub[p]) + 1 + int(rng.integers(0, 3))) % 4]
    ref[SUBST:SUBST + SEG] = sub
    ref[RC:RC + SEG] = revcomp(seg)
    reads = [seg[100:700], seg[300:900], bytes(ref[5200:5800]), revcomp(ref[200:800]), rng.choice(list(b"ACGT"), READ).astype(np.uint8).tobytes()]
    assert all(len(r) == READ for r in reads)
    starts = [READ * i for i in range(len(reads))]
    return np.frombuffer(bytes(ref), dtype=np.uint8).copy(), np.frombuffer(b"".join(reads), dtype=np.uint8).copy(), starts


@pytest.mark.parametrize("name", sorted(INDEXES))
def test_chain_select_end_to_end(texts, name):
    ref, reads, starts = texts
    ix = INDEXES[name]()
    k = ix.k
    try:
        ix.build_sequences(ref)
        before = ix.chains(reads, read_starts=starts)
        table, sel = ix.chain_select(reads, read_starts=starts, pri_pct=50)
        for f in ("seg", "rev", "q_start", "q_end", "r_start", "r_end", "count", "score", "chain"):
            assert np.array_equal(getattr(table, f), getattr(before, f)), f
        for f in ("seg", "score", "chain"):                    # ... and chains() afterwards too
            assert np.array_equal(getattr(ix.chains(reads, read_starts=starts), f), getattr(before, f)), f
        offs = np.searchsorted(table.seg.astype(np.int64), np.arange(len(starts) + 1)).astype(np.uint64)
        exp = select_model(table.q_start, table.q_end, table.score, table.count, offs, pri_pct=50)
        for nm, g, e in zip(NAMES, sel, exp):
            assert g.dtype == e.dtype and np.array_equal(g, e), (name, nm)
        ttab, tsel = ix.chain_select(to_dev(reads), read_starts=starts, pri_pct=50)
        assert np.array_equal(ttab.score.cpu().numpy(), table.score)
        for nm, g, e in zip(NAMES, tsel, exp):
            assert np.array_equal(g.cpu().numpy().view(e.dtype), e), (name, nm, "tensors")
        assert [x.dtype for x in tsel] == [torch.int32, torch.int32, torch.uint8, torch.uint8, torch.int32, torch.int32, torch.int32]
        # the defaults are those of select_chains
        assert all(np.array_equal(a, b) for a, b in zip(ix.chain_select(reads, read_starts=starts)[1], kh.select_table(table, len(starts))))
        parent, rank, mapq, flag, sub, nsub, best = sel
        assert len(best) == 5
        for g in (0, 1):                                       # the reads from the repeat
            rows = np.flatnonzero(table.seg == g)
            b = int(best[g])
            assert b in rows and flag[b] == 3 and (flag[rows] & 1).sum() == 1, (name, g, flag[rows])
            assert (flag[rows] == 2).sum() == 2 and nsub[b] >= 2, (name, g, flag[rows], table.score[rows])
            assert mapq[b] < 10 and sub[b] > 0, (name, g, mapq[b], table.score[rows])
            assert EXACT - k <= table.r_start[b] and table.r_end[b] <= EXACT + SEG + k and table.rev[b] == 0, (name, g, table.r_start[b], table.r_end[b])
        for g, strand in ((2, 0), (3, 1)):                     # the reads from unique sequence
            rows = np.flatnonzero(table.seg == g)
            b = int(best[g])
            assert b in rows and (flag[rows] & 1).sum() == 1 and table.rev[b] == strand, (name, g)
            assert table.count[b] >= 10 and table.score[b] >= 100 and nsub[b] == 0 and mapq[b] == 60, (name, g, table.count[b], table.score[b], mapq[b])
        assert best[4] == -1 and not (table.seg == 4).any()
    finally:
        ix.close()
