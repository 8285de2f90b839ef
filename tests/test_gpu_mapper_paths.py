"""GPU: the two memories of the mapper's pipeline against each other.  kmerhash_amd/mapper.py states every glue step once over an array
namespace; here map, map_pairs and map_pairs_rescued run once on numpy inputs and once on CUDA tensors, with read_ends given and
omitted, and every column of every returned tuple must hold the same bits in both memories -- and write_sam_rescued must print the same
file.  A random text of 4096 bases in two targets, a stranded closed-syncmer index (k = 15, s = 11: the mapper's timing workload), eight
pairs of 100-base mates: five plain ones, one with its mates on different targets, one with a mate whose seeds are all destroyed (a
substitution every 12 bases: it has no chain row and is rescued), one with a mate of pure N.
That the columns are the right ones is what test_gpu_pair_index.py, test_gpu_rescue_index.py and test_gpu_sam_index.py assert against
the models; this file does not repeat it."""
import functools
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edits_cases import revcomp  # noqa: E402

K, S, MATE, GAP, N_PAIRS = 15, 11, 100, 4, 8
CROSS, HIT, BLANK = 5, 6, 7          # the pair on two targets, the pair with the damaged mate, the pair with the mate of N


@functools.lru_cache(maxsize=None)
def make():
    """-> (Targets, reads text, starts, ends)"""
    import kmerhash_amd as kh
    rng = np.random.default_rng(4096)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    T = kh.Targets.from_sequences(["ctgA", "ctgB"], [rng.choice(bases, size=2016).tobytes() for _ in range(2)], spacer=64)
    text = T.text.tobytes()
    assert len(text) == 4096
    reads = []
    for p in range(N_PAIRS):
        t, frag = p % 2, int(rng.integers(300, 401))
        g = int(T.starts[t]) + int(rng.integers(10, 2016 - 410))
        head, tail = text[g:g + MATE], text[g + frag - MATE:g + frag]
        if p == CROSS:      # the downstream mate comes from the other target
            o = int(T.starts[1 - t]) + 700
            tail = text[o:o + MATE]
        if p == HIT:
            m = bytearray(tail)
            for at in range(5, MATE - 5, 12):
                m[at] = b"ACGT"[(b"ACGT".index(m[at]) + 1) % 4]
            tail = bytes(m)
        if p == BLANK:
            head = b"N" * MATE
        reads += [head, revcomp(tail)]
    starts = np.arange(2 * N_PAIRS, dtype=np.int64) * (MATE + GAP)
    return T, (b"N" * GAP).join(reads) + b"N" * GAP, starts, starts + MATE


def columns(x):
    """every column of a (nested) tuple of arrays or tensors, as host bytes with its length"""
    if isinstance(x, tuple):
        return [c for y in x for c in columns(y)]
    a = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return [(len(a), a.dtype.itemsize, a.tobytes())]


@pytest.mark.gpu
@pytest.mark.parametrize("give_ends", [True, False])
def test_numpy_and_cuda_inputs_give_the_same_bits(give_ends):
    pytest.importorskip("torch")
    import kmerhash_amd as kh
    from stream_checks import to_dev
    T, seq, starts, ends = make()
    qt, rt = np.frombuffer(seq, dtype=np.uint8).copy(), T.text.copy()
    names = ["frag%d" % (s // 2) for s in range(2 * N_PAIRS)]
    got = {}
    ix = kh.KmerPositionIndex(k=K, s=S, stranded=True)
    try:
        ix.build_sequences(rt)
        for mem, mk in (("numpy", lambda x: x), ("cuda", to_dev)):
            q, r, rs, re_ = mk(qt), mk(rt), mk(starts), (mk(ends) if give_ends else None)
            kw = dict(min_score=20, min_count=2, max_ins=1000, targets=T)
            mp = ix.map(q, r, rs, re_, targets=T, min_score=20, min_count=2)
            mp2, pr = ix.map_pairs(q, r, rs, re_, **kw)
            mp3, pr3, res = ix.map_pairs_rescued(q, r, rs, re_, **kw)
            fh = io.StringIO()
            counts = kh.write_sam_rescued(fh, mp3, pr3, res, q, r, names, rs, re_, cs=True, targets=T)
            got[mem] = (columns(mp), columns((mp2, pr)), columns((mp3, pr3, res)), fh.getvalue(), counts, pr3, res)
    finally:
        ix.close()
    a, b = got["numpy"], got["cuda"]
    for what, x, y in zip(("map", "map_pairs", "map_pairs_rescued"), a, b):
        assert len(x) == len(y), what
        for i, (cx, cy) in enumerate(zip(x, y)):
            assert cx == cy, (what, i)
    assert a[3] == b[3] and a[4] == b[4]
    # the inputs are the ones the docstring names: the damaged mate and nobody else is placed by rescue, the pair on two targets is not proper
    pr, res = a[5], a[6]
    hit = 2 * HIT + 1
    assert res.read.tolist().count(hit) == 1 and pr.row[hit] == -1 and pr.row[hit - 1] >= 0
    # (8 substitutions; without read_ends the read runs to the next start and takes its 4 separating N along, which match nothing)
    assert [int(s) for s, e in zip(res.read, res.edits) if e >= 0] == [hit] and int(res.edits[res.read.tolist().index(hit)]) == (8 if give_ends else 8 + GAP)
    assert pr.row[2 * CROSS] >= 0 and pr.row[2 * CROSS + 1] >= 0 and not pr.flag[CROSS] & 1 and not pr.flag[CROSS] & 4
    assert pr.row[2 * BLANK] == -1 and all(pr.flag[p] & 1 for p in range(CROSS))
    lines = [l.split("\t") for l in a[3].splitlines() if not l.startswith("@")]
    assert [int(l[1]) & 0x4 for l in lines if l[0] == "frag%d" % HIT] == [0, 0] and any("tp:A:R" in l for l in lines)
