"""GPU: ix.map end to end on both index classes: 60 reads of 150 to 400 bases cut from a random reference of 20 kb -- both strands,
substitutions, an insertion and a deletion between seeds, an end mutated until it clips, one read with a stretch no link of 31 edits
spans (no whole alignment), one read of a region that stands in the reference twice (a secondary).  With ref_order=False every row is
exactly what the host helpers read_cigar and extended_intervals give; nm is the edits of the links and the ends; ref_order=True turns
exactly the reverse-strand rows round; write_paf prints the lines this test assembles from the host helpers; map() leaves chain_ends and
select_table as they were."""
import io
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
from edits_cases import bases, other, revcomp  # noqa: E402
from stream_checks import to_dev  # noqa: E402

N_READS, REF_LEN = 60, 20000


def make_reads(seed=21):
    rng = random.Random(seed)
    ref = bytearray(bases(rng, REF_LEN))
    ref[15000:15300] = ref[5000:5300]                       # a region that stands twice
    ref = bytes(ref)
    reads = []
    for t in range(N_READS):
        n = rng.randrange(150, 401)
        p = 5010 if t == 7 else rng.choice([x for x in range(100, REF_LEN - 500, 37) if not (4600 < x < 5400 or 14600 < x < 15400)])
        r = bytearray(ref[p:p + (280 if t == 7 else n)])
        if t != 7:
            for _ in range(t % 4):                              # substitutions between seeds
                x = rng.randrange(30, len(r) - 30)
                r[x] = other(rng, r[x])
            if t % 5 == 1:
                r.insert(len(r) // 2, rng.choice(b"ACGT"))
            if t % 5 == 2:
                del r[len(r) // 3]
            if t % 6 == 3:                                      # an end that clips: every other base of the last 16 changed
                for x in range(len(r) - 16, len(r), 2):
                    r[x] = other(rng, r[x])
            if t == 11:                                         # 40 substitutions in a row of 80 bases: more than 31 edits in one link
                for x in range(len(r) // 2 - 40, len(r) // 2 + 40, 2):
                    r[x] = other(rng, r[x])
        r = bytes(r)
        reads.append(revcomp(r) if t & 1 else r)
    starts, ends, parts, at = [], [], [], 0
    for r in reads:
        starts.append(at); ends.append(at + len(r)); parts.append(r + b"\n"); at += len(r) + 1
    return ref, b"".join(parts), np.array(starts, dtype=np.int64), np.array(ends, dtype=np.int64)


def paf_cigar(s, rev):
    parts = re.findall(r"\d+[SID=X]", s)
    return "".join(parts[::-1] if rev else parts)


@pytest.mark.parametrize("cls,k", [("KmerPositionIndex", 15), ("WideKmerPositionIndex", 35)])
@pytest.mark.parametrize("dev", [False, True])
def test_map_of_planted_reads(cls, k, dev):
    ref, seq, starts, ends_at = make_reads()
    ix = getattr(kh, cls)(k=k, stranded=True, **({"s": 25} if cls == "WideKmerPositionIndex" else {}))
    try:
        rt, qt = np.frombuffer(ref, dtype=np.uint8).copy(), np.frombuffer(seq, dtype=np.uint8).copy()
        mk = to_dev if dev else (lambda a: a)
        ix.build_sequences(mk(rt))
        params = dict(read_starts=starts, read_ends=ends_at, min_score=20, min_count=2, pri_pct=50)
        before = ix.chain_ends(mk(qt), mk(rt), read_starts=starts, read_ends=ends_at, min_score=20, min_count=2)
        mp = ix.map(mk(qt), mk(rt), ref_order=False, **params)
        mo = ix.map(mk(qt), mk(rt), **params)                                  # ref_order=True is the default
        if dev:
            torch.cuda.synchronize()
        host = lambda x: x.cpu().numpy() if dev else np.asarray(x)          # noqa: E731
        flat = lambda t, e, c, n: list(t[:8]) + list(t.anchors) + [t.chain] + list(e) + list(c) + list(n)      # noqa: E731
        for a, b in zip(flat(*before), flat(*mp[:4])):
            assert np.array_equal(host(a), host(b))
        sel = kh.select_table(mp.table, N_READS, pri_pct=50)
        assert all(np.array_equal(host(a), host(b)) for a, b in zip(sel, mp.select))
        rec, rec_o = [host(x) for x in mp.records], [host(x) for x in mo.records]
        valid, qs, qe, rs, re_, qlen, n_match, n_block, nm, offs, ops = (x.view(np.uint8 if i == 0 else np.uint64 if i == 9 else np.uint32) for i, x in enumerate(rec))
        seg, rev = host(mp.table.seg), host(mp.table.rev)
        q0, q1, r0, r1 = kh.extended_intervals(mp.table, mp.ends)
        link_edits, end_edits = host(mp.edits.edits).view(np.uint32), host(mp.ends.edits).view(np.uint32)
        n_rows = len(valid)
        assert n_rows >= N_READS - 2
        toff, text = kh.cigar_text(mp.records.offsets, mp.records.ops)
        toff, text = host(toff), host(text).tobytes().decode()
        strings, n_rev = [], 0
        for c in range(n_rows):
            s = kh.read_cigar(mp.cigars, mp.ends, mp.table, c, k)
            strings.append(s)
            lo = int(starts[int(seg[c])])
            assert bool(valid[c]) == (s is not None), c
            assert text[toff[c]:toff[c + 1]] == (s or ""), c
            assert (int(qs[c]) + lo, int(qe[c]) + lo, int(rs[c]), int(re_[c])) == (int(q0[c]), int(q1[c]), int(r0[c]), int(r1[c])), c
            assert int(qlen[c]) == int(ends_at[int(seg[c])]) - lo
            row, row_o = ops[offs[c]:offs[c + 1]], rec_o[10].view(np.uint32)[offs[c]:offs[c + 1]]
            if valid[c]:
                assert int(nm[c]) == int(link_edits[c]) + int(end_edits[2 * c]) + int(end_edits[2 * c + 1]), c
                parts = [(int(n), o) for n, o in re.findall(r"(\d+)([SID=X])", s)]
                assert int(n_match[c]) == sum(n for n, o in parts if o == "=") and int(n_block[c]) == sum(n for n, o in parts if o in "=XID")
            assert np.array_equal(row_o, row[::-1] if rev[c] & 1 else row), c
            n_rev += int(rev[c]) & 1
        for a, b in zip(rec[:10], rec_o[:10]):                                  # the numbers and offsets do not depend on ref_order
            assert np.array_equal(a, b)
        flag = host(mp.select.flag)
        assert 0 < n_rev < n_rows and (valid == 0).sum() >= 1 and ((flag & 1) == 0).sum() >= 1      # both strands, an invalid row, a secondary
        assert any("I" in s for s in strings if s) and any("D" in s for s in strings if s) and any("X" in s for s in strings if s)
        assert (host(mp.ends.clip).view(np.uint32) > 0).any()                     # an end that clips
        # the PAF lines
        names = ["read%d" % i for i in range(N_READS)]
        for kept_only in (True, False):
            fh = io.StringIO()
            written, skipped = kh.write_paf(fh, mo, names, "ref", REF_LEN, k, kept_only=kept_only)
            mapq, sub, count, score = host(mp.select.mapq), host(mp.select.sub), host(mp.table.count).view(np.uint32), host(mp.table.score)
            exp, exp_skipped = [], 0
            for c in range(n_rows):
                if kept_only and not flag[c] & 2:
                    continue
                if strings[c] is None:
                    exp_skipped += 1
                    continue
                parts = [(int(n), o) for n, o in re.findall(r"(\d+)([SID=X])", strings[c])]
                lo = int(starts[int(seg[c])])
                f = [names[int(seg[c])], int(ends_at[int(seg[c])]) - lo, int(q0[c]) - lo, int(q1[c]) - lo, "-" if rev[c] & 1 else "+", "ref", REF_LEN, int(r0[c]), int(r1[c]),
                     sum(n for n, o in parts if o == "="), sum(n for n, o in parts if o in "=XID"), int(mapq[c]), "tp:A:" + ("P" if flag[c] & 1 else "S"),
                     "cm:i:%d" % count[c], "s1:i:%d" % score[c]] + (["s2:i:%d" % sub[c]] if flag[c] & 1 else [])
                f += ["NM:i:%d" % sum(n for n, o in parts if o in "XID"), "cg:Z:" + paf_cigar(strings[c], rev[c] & 1)]
                exp.append("\t".join(str(x) for x in f))
            assert fh.getvalue().splitlines() == exp
            assert (written, skipped) == (len(exp), exp_skipped)
    finally:
        ix.close()


def test_map_refuses_an_unstranded_index():
    ix = kh.KmerPositionIndex(k=15)
    try:
        with pytest.raises(ValueError, match="stranded=True"):
            ix.map(b"ACGT" * 10, b"ACGT" * 10)
    finally:
        ix.close()
