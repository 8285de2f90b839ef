"""GPU: ix.map_pairs_rescued and write_sam_rescued end to end, on both index classes, against one reference and against a contig table.
The reference is 20 000 random bases laid out as two targets; 40 fragments of 300-500 bases give 100-base mates.  In 20 fragments one
mate carries a substitution every 12 bases, none within 5 bases of either end: with k = 15 no seed survives, the mate has no chain row
and pairing leaves it unmapped.  In 5 of those the mate also lacks 2 bases of the reference.  A 41st fragment has a mate of random bases.
First, without the GPU: the MODEL places every damaged mate at its planted interval (a condition on the inputs: the seed below is
chosen so that it holds).  Then: map_pairs leaves exactly these mates without a row; map_pairs_rescued returns the model's MateRescue
bit for bit over requests the test derives from the plan alone; write_sam_rescued prints the 20 with the planted POS, strand, 0x2 and
|TLEN| = the fragment length, their partners to match, and every other read byte for byte as write_sam_pairs does; the random mate
comes back -2 and stays unmapped."""
import functools
import io
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import diffs_model as DM  # noqa: E402
import rescue_model as RM  # noqa: E402
from edits_cases import revcomp  # noqa: E402

LEN_A, LEN_B, MATE, N_FRAGS, N_HIT, N_DEL, GAP = 12_000, 8_000, 100, 41, 20, 5, 4
SUBS = list(range(5, MATE - 5, 12))          # 5, 17, ..., 89: 8 substitutions, 11 bases between two of them
LOST = N_FRAGS - 1
MAX_INS, MAX_EDITS = 1000, 31


@functools.lru_cache(maxsize=None)
def make():
    """-> (Targets, reads text, starts, ends, plan): plan[p] = (global start, fragment length, reverse fragment?, damaged read or -1,
    the damaged mate's (rs, re, strand, edits) or None)"""
    import kmerhash_amd as kh
    rng = np.random.default_rng(2026)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    T = kh.Targets.from_sequences(["ctgA", "ctgB"], [rng.choice(bases, size=LEN_A).tobytes(), rng.choice(bases, size=LEN_B).tobytes()])
    text = T.text.tobytes()
    reads, plan = [], []
    for p in range(N_FRAGS):
        t, frag = p % 2, int(rng.integers(300, 501))
        g = int(T.starts[t]) + int(rng.integers(20, int(T.lengths[t]) - 520))
        rev = p % 4 >= 2                     # the fragment comes from the reverse strand: mate 1 is its downstream end
        head, tail = text[g:g + MATE], text[g + frag - MATE:g + frag]
        hit, placed = -1, None
        if p < N_HIT or p == LOST:
            down = p % 3 == 0                # the damaged mate: the downstream (reverse-strand) or the upstream one
            span = MATE + (2 if p < N_DEL else 0)
            lo = g + frag - span if down else g
            m = bytearray(text[lo:lo + span])
            if p < N_DEL:
                del m[50:52]
            for at in SUBS:
                m[at] = b"ACGT"[(b"ACGT".index(m[at]) + 1 + int(rng.integers(0, 3))) % 4]
            if p == LOST:
                m = bytearray(rng.choice(bases, size=MATE).tobytes())
            head, tail = (head, bytes(m)) if down else (bytes(m), tail)
            hit = 2 * p + (int(down) ^ int(rev))          # mate 2 is the downstream end of a forward fragment, mate 1 of a reverse one
            placed = (lo, lo + span, int(down), len(SUBS) + (2 if p < N_DEL else 0))
        m1, m2 = (revcomp(tail), head) if rev else (head, revcomp(tail))
        reads += [m1, m2]
        plan.append((g, frag, rev, hit, placed))
    seq = (b"N" * GAP).join(reads)
    starts = np.arange(2 * N_FRAGS, dtype=np.int64) * (MATE + GAP)
    return T, seq, starts, starts + MATE, plan


@functools.lru_cache(maxsize=None)
def expected(with_targets):
    """the requests as the plan gives them, and the model's answer to them"""
    T, seq, starts, ends, plan = make()
    req = []
    for p, (g, frag, rev, hit, placed) in enumerate(plan):
        if hit < 0:
            continue
        down = placed[2]
        prs, pre = (g, g + MATE) if down else (g + frag - MATE, g + frag)          # the partner's interval: it is exact
        w_lo, w_hi = (prs, prs + MAX_INS) if down else (pre - MAX_INS, pre)      # min_ins 0, m + max_edits > 0
        t = p % 2
        lo, hi = (int(T.starts[t]), int(T.ends[t])) if with_targets else (0, len(T.text))
        w_lo = min(max(w_lo, lo), hi)
        w_hi = max(min(w_hi, hi), w_lo)
        req.append((hit, int(starts[hit]), int(ends[hit]), w_lo, w_hi, down))
    req.sort()
    cols = [np.array(c, dtype=np.uint32) for c in zip(*req)]
    cols[5] = cols[5].astype(np.uint8)
    return cols, RM.rescue_model(seq, T.text, *cols[1:], 0, MAX_EDITS)


@pytest.mark.parametrize("with_targets", [False, True])
def test_the_model_places_every_damaged_mate_where_it_was_planted(with_targets):
    _, _, _, _, plan = make()
    (read, *_), (edits, rs, re, span, offsets, ops) = expected(with_targets)
    assert len(read) == N_HIT + 1
    at = {int(s): j for j, s in enumerate(read)}
    for p, (g, frag, rev, hit, placed) in enumerate(plan):
        if hit < 0:
            continue
        j = at[hit]
        if p == LOST:
            assert edits[j] == RM.OVER
            continue
        assert (int(rs[j]), int(re[j]), int(edits[j]), int(span[j])) == (placed[0], placed[1], placed[3], 0), (p, placed)
    assert len(SUBS) == 8 and all(b - a == 12 for a, b in zip(SUBS, SUBS[1:])) and SUBS[0] >= 5 and SUBS[-1] < MATE - 5


@pytest.mark.gpu
@pytest.mark.parametrize("with_targets", [False, True])
@pytest.mark.parametrize("cls,k", [("KmerPositionIndex", 15), ("WideKmerPositionIndex", 33)])
def test_rescue_end_to_end(cls, k, with_targets):
    torch = pytest.importorskip("torch")
    import kmerhash_amd as kh
    from stream_checks import to_dev
    T, seq, starts, ends, plan = make()
    (read, q_lo, q_hi, w_lo, w_hi, rv), exp = expected(with_targets)
    dev = (cls == "WideKmerPositionIndex") != with_targets      # tensors in two of the four runs, numpy in the others
    mk = to_dev if dev else (lambda x: x)
    rt, qt = T.text.copy(), np.frombuffer(seq, dtype=np.uint8).copy()
    names = ["frag%d" % (s // 2) for s in range(2 * N_FRAGS)]
    where = dict(targets=T) if with_targets else dict(ref_name="ref", ref_len=len(rt))
    tg = T if with_targets else None
    ix = getattr(kh, cls)(k=k, stranded=True, **({"s": 25} if cls == "WideKmerPositionIndex" else {}))
    try:
        ix.build_sequences(mk(rt))
        mp0, pr0 = ix.map_pairs(mk(qt), mk(rt), starts, ends, min_score=20, min_count=2, max_ins=MAX_INS, targets=tg)
        mp, pr, res = ix.map_pairs_rescued(mk(qt), mk(rt), mk(starts), mk(ends), min_score=20, min_count=2, max_ins=MAX_INS, targets=tg)
        f_pairs, f_resc = io.StringIO(), io.StringIO()
        kh.write_sam_pairs(f_pairs, mp, pr, mk(qt), mk(rt), names, starts, ends, cs=True, **where)
        kh.write_sam_rescued(f_resc, mp, pr, res, mk(qt), mk(rt), names, starts, ends, cs=True, **where)
    finally:
        ix.close()
    host = lambda x, dt: (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).view(dt)      # noqa: E731
    # map_pairs_rescued runs map_pairs: the same Mapping columns and the same PairSelect
    for a, b in zip(tuple(pr) + (mp.records.rs, mp.records.re, mp.records.ops), tuple(pr0) + (mp0.records.rs, mp0.records.re, mp0.records.ops)):
        assert host(a, np.uint8).tobytes() == host(b, np.uint8).tobytes()
    row = host(pr.row, np.int32)
    assert sorted(np.flatnonzero(row < 0).tolist()) == sorted(int(s) for s in read), "pairing leaves exactly the damaged mates without a row"
    # the MateRescue is the model's, bit for bit
    got = (res.edits, res.rs, res.re, res.span, res.offsets, res.ops)
    for name, g, e in zip(("edits", "rs", "re", "span", "offsets", "ops"), got, exp):
        assert np.array_equal(host(g, e.dtype), e), name
    assert np.array_equal(host(res.read, np.uint32), read) and np.array_equal(host(res.rev, np.uint8), rv)
    # ---- the two files
    split = lambda fh: [l.split("\t") for l in fh.getvalue().splitlines() if not l.startswith("@")]      # noqa: E731
    key = lambda f: (int(f[0][4:]), 1 if int(f[1]) & 0x80 else 0)      # noqa: E731
    old, new = {}, {}
    for f in split(f_pairs):
        old.setdefault(key(f), []).append(f)
    for f in split(f_resc):
        new.setdefault(key(f), []).append(f)
    assert sorted(old) == sorted(new) == [(p, m) for p in range(N_FRAGS) for m in (0, 1)]
    at = {int(s): j for j, s in enumerate(read)}
    for p, (g, frag, rev, hit, placed) in enumerate(plan):
        if hit < 0 or p == LOST:      # untouched pairs, and the pair whose mate came back -2: byte for byte the lines of write_sam_pairs
            assert new[p, 0] == old[p, 0] and new[p, 1] == old[p, 1], p
            continue
        me, mate = new[p, hit & 1], new[p, (hit & 1) ^ 1]
        assert len(me) == 1 and int(old[p, hit & 1][0][1]) & 0x4 and int(old[p, (hit & 1) ^ 1][0][1]) & 0x8
        f, j, t = me[0], at[hit], p % 2
        fl, t0 = int(f[1]), int(T.starts[t]) if with_targets else 0
        assert not fl & 0x4 and fl & 0x2 and fl & 0x1 and bool(fl & 0x10) == bool(placed[2]) and bool(fl & 0x20) != bool(placed[2])
        assert f[2] == (T.names[t] if with_targets else "ref") and int(f[3]) == placed[0] - t0 + 1 and f[6] == "=" and abs(int(f[8])) == frag
        assert (int(f[8]) > 0) == (not placed[2]) and "tp:A:R" in f and "NM:i:%d" % placed[3] in f and int(f[4]) == int(host(pr.mapq, np.uint8)[hit ^ 1])
        assert sum(int(n) for n in re.findall(r"(\d+)[=XI]", f[5])) == MATE and sum(int(n) for n in re.findall(r"(\d+)[=XD]", f[5])) == placed[1] - placed[0]
        assert len(f[9]) == MATE and f[9] == (placed[2] and revcomp(seq[int(starts[hit]):int(ends[hit])]) or seq[int(starts[hit]):int(ends[hit])]).decode()
        runs = [int(v) for v in exp[5][int(exp[4][j]):int(exp[4][j + 1])]]      # the difference strings: those of the model's row over the two texts
        for tag, kind in (("MD:Z:", DM.MD), ("cs:Z:", DM.CS)):
            want = DM.row_text(seq, rt.tobytes(), 0, runs, 1, placed[2], int(starts[hit]), int(ends[hit]), int(exp[1][j]), kind)
            assert want is not None and [x for x in f if x.startswith(tag)] == [tag + want.decode()], (p, tag)
        if p >= N_DEL:      # by hand: 8 substitutions, 11 matching bases between two of them, in reference order
            md = next(x for x in f if x.startswith("MD:Z:"))[5:]
            assert re.fullmatch(r"5[ACGT](11[ACGT]){7}10", md), (p, md)
        rep = [x for x in mate if not int(x[1]) & 0x900]
        assert len(rep) == 1
        x, o = rep[0], [y for y in old[p, (hit & 1) ^ 1] if not int(y[1]) & 0x900][0]
        assert int(x[1]) == (int(o[1]) & ~0x8) | 0x2 | (0x20 if placed[2] else 0) and x[6] == "=" and x[7] == f[3] and f[7] == x[3]
        assert int(x[8]) == -int(f[8]) and x[:1] + x[2:6] + x[9:] == o[:1] + o[2:6] + o[9:]
    lost = plan[LOST][3]
    assert int(host(res.edits, np.int32)[at[lost]]) == kh.RESCUE_OVER and int(new[LOST, lost & 1][0][1]) & 0x4
