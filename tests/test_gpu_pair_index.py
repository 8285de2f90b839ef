"""GPU: ix.map_pairs and write_sam_pairs end to end, on both index classes, against one reference and against a contig table.  The
genome is 20 kb of random bases that hold an exact 1.5 kb duplicate, plus a second short target; 200 fragments of 300-500 bases give 100-base
mates (mate 2 reverse-complemented, a few substitutions per mate at least 20 bases from either end).  Every pair with both mates mapped
on one target is proper and its template length is the planted fragment length; a mate inside the duplicate whose partner lies outside
takes the copy the partner names with quality 60 where select alone gives 0; a pair inside the duplicate altogether has quality 0; a pair
planted across the two targets is not proper, has template length 0 and names the other target in RNEXT.  The SAM file is parsed back."""
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from edits_cases import revcomp  # noqa: E402
from stream_checks import to_dev  # noqa: E402

LEN_A, LEN_B, DUP_A, DUP_B, DUP_LEN, MATE, N_PAIRS = 20_000, 3_000, 3_000, 12_000, 1_500, 100, 200
GAP = 4                           # bytes that are no base between two reads: no seed spans two reads
X_PAIR, LOST_PAIR = 198, 199      # the pair across the two targets; the pair whose mate 2 is no part of the genome


def make_pairs():
    """-> (target A, target B, the reads' text, plan): plan[p] = (kind, target of mate 1, fragment start on it, fragment length, reverse?)"""
    rng = np.random.default_rng(77)
    a = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=LEN_A)
    a[DUP_B:DUP_B + DUP_LEN] = a[DUP_A:DUP_A + DUP_LEN]
    b = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=LEN_B)
    A, B = a.tobytes(), b.tobytes()
    free = [(100, 2400), (4700, 11400), (13700, 19400)]      # fragment starts on A well away from both copies
    plan = []
    for p in range(N_PAIRS):
        frag = int(rng.integers(300, 501))
        if p < 8:          # the last mate 10..90 bases inside a copy, the first one outside it
            start = (DUP_A, DUP_B)[(p // 2) % 2] + int(rng.integers(10, 91)) + MATE - frag
            plan.append(("straddle", 0, start, frag))
        elif p < 14:       # the whole fragment inside a copy
            plan.append(("inside", 0, (DUP_A, DUP_B)[(p // 2) % 2] + int(rng.integers(20, DUP_LEN - frag - 20)), frag))
        elif p < 24:
            plan.append(("plain", 1, int(rng.integers(100, LEN_B - 600)), frag))
        else:
            lo, hi = free[int(rng.integers(0, 3))]
            plan.append(("plain", 0, int(rng.integers(lo, hi)), frag))
    plan[X_PAIR] = ("across", 0, 15000, 400)
    plan[LOST_PAIR] = ("lost", 0, 16000, 400)

    def mutate(read):
        r = bytearray(read)
        for at in rng.choice(np.arange(20, 45), size=3, replace=False):
            r[at] = ord("ACGT"[("ACGT".index(chr(r[at])) + 1 + int(rng.integers(0, 3))) % 4])
        return bytes(r)

    reads, full = [], []
    for p, (kind, t, start, frag) in enumerate(plan):
        text = (A, B)[t]
        head, tail = text[start:start + MATE], text[start + frag - MATE:start + frag]
        if kind == "across":
            tail = B[1000:1000 + MATE]
        if kind == "lost":
            tail = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=MATE).tobytes()
        rev = p % 2 == 1      # the fragment comes from the reverse strand: mate 1 is its downstream end
        m1, m2 = (revcomp(tail), head) if rev else (head, revcomp(tail))
        reads += [mutate(m1), mutate(m2)]
        full.append((kind, t, start, frag, rev))
    return A, B, (b"N" * GAP).join(reads), full


@pytest.mark.parametrize("with_targets", [False, True])
@pytest.mark.parametrize("cls,k", [("KmerPositionIndex", 15), ("WideKmerPositionIndex", 33)])
def test_pairs_end_to_end(cls, k, with_targets):
    A, B, seq, plan = make_pairs()
    T = kh.Targets.from_sequences(["ctgA", "ctgB"], [A, B])
    startA, startB = int(T.starts[0]), int(T.starts[1])
    dev = (cls == "WideKmerPositionIndex") != with_targets      # tensors in two of the four runs, numpy in the others
    mk = to_dev if dev else (lambda x: x)
    rt, qt = T.text.copy(), np.frombuffer(seq, dtype=np.uint8).copy()
    n_reads = 2 * N_PAIRS
    starts = np.arange(n_reads, dtype=np.int64) * (MATE + GAP)
    ends_at = starts + MATE
    names = ["frag%d" % (s // 2) for s in range(n_reads)]
    where = dict(targets=T) if with_targets else dict(ref_name="ref", ref_len=len(rt))
    ix = getattr(kh, cls)(k=k, stranded=True, **({"s": 25} if cls == "WideKmerPositionIndex" else {}))
    try:
        ix.build_sequences(mk(rt))
        with pytest.raises(ValueError, match="even number of reads"):
            ix.map_pairs(mk(qt), mk(rt), starts[:-1], ends_at[:-1], min_score=20, min_count=2)
        mp, pr = ix.map_pairs(mk(qt), mk(rt), starts, ends_at, min_score=20, min_count=2, targets=T if with_targets else None)
        fh, f1 = io.StringIO(), io.StringIO()
        kh.write_sam_pairs(fh, mp, pr, mk(qt), mk(rt), names, starts, ends_at, **where)
        kh.write_sam(f1, mp, mk(qt), mk(rt), names, starts, ends_at, **where)
    finally:
        ix.close()
    # write_sam knows nothing of pairs: its lines keep * 0 0 and none of 0x1 0x2 0x8 0x20 0x40 0x80
    assert all(l.split("\t")[6:9] == ["*", "0", "0"] and not int(l.split("\t")[1]) & 0xEB for l in f1.getvalue().splitlines() if not l.startswith("@"))
    host = lambda x, dt: (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).view(dt)      # noqa: E731
    row, mapq, tlen, flag = host(pr.row, np.int32), host(pr.mapq, np.uint8), host(pr.tlen, np.int32), host(pr.flag, np.uint8)
    rs, smq, rv = host(mp.records.rs, np.uint32).astype(np.int64), host(mp.select.mapq, np.uint8), host(mp.table.rev, np.uint8)
    seen = {"straddle": 0, "inside": 0, "plain": 0}
    for p, (kind, t, start, frag, rev) in enumerate(plan):
        r1, r2 = int(row[2 * p]), int(row[2 * p + 1])
        if kind == "lost":
            gone, kept = (r1, r2) if rev else (r2, r1)      # (the downstream end is no part of the genome; it is mate 1 of a reverse fragment)
            assert kept >= 0 and gone == -1 and flag[p] == 0 and (tlen[2 * p], tlen[2 * p + 1]) == (0, 0)
            continue
        if kind == "across":
            assert r1 >= 0 and r2 >= 0 and not flag[p] & 1
            if with_targets:
                assert flag[p] == 2 and (tlen[2 * p], tlen[2 * p + 1]) == (0, 0)
            continue
        if r1 < 0 or r2 < 0:
            continue
        assert flag[p] == 7, (p, kind, flag[p])
        sign = -1 if rev else 1
        assert (tlen[2 * p], tlen[2 * p + 1]) == (sign * frag, -sign * frag), (p, kind)
        seen[kind] += 1
        g0 = (startA, startB)[t] + start      # the fragment's first base in global coordinates
        up, down = (r2, r1) if rev else (r1, r2)      # the rows of the upstream (forward) and the downstream (reverse) mate
        if kind == "inside":
            assert (mapq[2 * p], mapq[2 * p + 1]) == (0, 0), p
            assert rs[up] - g0 in (0, DUP_B - DUP_A, DUP_A - DUP_B), p
        else:
            assert rs[up] == g0 and rs[down] == g0 + frag - MATE and (rv[up] & 1, rv[down] & 1) == (0, 1), (p, kind)
        if kind == "straddle":      # the downstream mate lies in the repeat: alone it has quality 0, its partner pins it
            q = 2 * p + (0 if rev else 1)
            assert smq[down] == 0 and mapq[q] == 60 and mapq[q ^ 1] == 60, (p, smq[down], mapq[q])
    assert seen["straddle"] >= 6 and seen["inside"] >= 4 and seen["plain"] >= 150, seen
    # ---- the file, parsed back
    body = [l.split("\t") for l in fh.getvalue().splitlines() if not l.startswith("@")]
    by_read = {}
    for f in body:
        assert f[0].startswith("frag") and int(f[1]) & 1 and bool(int(f[1]) & 0x40) != bool(int(f[1]) & 0x80)
        by_read.setdefault((int(f[0][4:]), 1 if int(f[1]) & 0x80 else 0), []).append(f)
    assert sorted(by_read) == [(p, m) for p in range(N_PAIRS) for m in (0, 1)], "every read has a line, under its mate number"
    order = [(int(f[0][4:]), 1 if int(f[1]) & 0x80 else 0) for f in body]
    assert order == sorted(order), "mate 1 before mate 2, pairs ascending"
    n_unmapped = 0
    for p in range(N_PAIRS):
        reps = []
        for m in (0, 1):
            main = [f for f in by_read[p, m] if not int(f[1]) & 0x900]
            assert len(main) == 1, (p, m)
            reps.append(main[0])
        for me, mate in ((reps[0], reps[1]), (reps[1], reps[0])):
            fl, mfl = int(me[1]), int(mate[1])
            assert bool(fl & 0x20) == bool(mfl & 0x10) and bool(fl & 0x8) == bool(mfl & 0x4)
            assert bool(fl & 0x2) == bool(flag[p] & 1 and not fl & 0x4)
            if not (fl & 0x4 and mfl & 0x4):
                assert me[7] == mate[3] and (me[6] == "=") == (me[2] == mate[2]) and (me[6] == "=" or me[6] == mate[2]), (p, me[:9], mate[:9])
            else:
                assert me[2:9] == ["*", "0", "0", "*", "*", "0", "0"]
            if fl & 0x4 and not mfl & 0x4:
                n_unmapped += 1
                assert me[2:4] == mate[2:4] and me[6:9] == ["=", mate[3], "0"] and mfl & 0x8
            for other in by_read[p, 0 if me is reps[0] else 1]:
                if other is not me:      # the secondary and supplementary lines carry the mate columns and no 0x2
                    assert not int(other[1]) & 0x2 and other[7] == mate[3] and other[8] == "0"
                    assert bool(int(other[1]) & 0x20) == bool(mfl & 0x10) and bool(int(other[1]) & 0x8) == bool(mfl & 0x4)
        assert int(reps[0][8]) + int(reps[1][8]) == 0
        assert (int(reps[0][8]), int(reps[1][8])) == (int(tlen[2 * p]), int(tlen[2 * p + 1])) and int(reps[0][4]) == mapq[2 * p] * (row[2 * p] >= 0)
    gone = 0 if plan[LOST_PAIR][4] else 1
    assert n_unmapped >= 1 and int(by_read[LOST_PAIR, gone][0][1]) & 0x4 and int(by_read[LOST_PAIR, gone ^ 1][0][1]) & 0x8
    if with_targets:
        x1, x2 = [[f for f in by_read[X_PAIR, m] if not int(f[1]) & 0x900][0] for m in (0, 1)]
        assert (x1[2], x1[6], x2[2], x2[6]) == ("ctgA", "ctgB", "ctgB", "ctgA") and (x1[8], x2[8]) == ("0", "0") and not int(x1[1]) & 0x2
