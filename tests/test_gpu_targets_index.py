"""GPU: mapping against several targets end to end, on both index classes (k = 15, s = 11 and k = 63, s = 31): random contigs A, B and
C of 3000, 2000 and 150 bases laid out by kh.Targets with a spacer of 32.  All checks are facts of the construction, not measured
thresholds:
  (a) exact reads of 150 bases cut from known places on both strands of every contig, the read that IS contig C included: the read's
      primary row is valid, targets.locate names the contig it was cut from, the target-local interval is the place it was cut from and
      the CIGAR is 150=.  (Closed syncmers leave no k - s + 1 consecutive windows without one: a read of 150 bases holds at least 27
      seeds at k = 15 and at least 2 at k = 63.)
  (b) a chimeric read, the last 75 bases of A followed by the first 75 of B: exactly two rows, one per contig, each with 75 bases
      soft-clipped -- the spacer costs 32 edits, one more than an alignment may spend, and behind a contig's end every further base
      costs clip_cost and gains at most 1, so an end stops exactly at the junction.
  (c) with a Targets of one contig ix.map(..., targets=T) equals ix.map(...) over the same text array by array, and write_paf line
      by line.
No row of any of them has [rs, re) outside its target."""
import io
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from edits_cases import bases, revcomp  # noqa: E402
from stream_checks import to_dev  # noqa: E402
from syncmer_model import kept_flags  # noqa: E402

LENGTHS = {"A": 3000, "B": 2000, "C": 150}
READ = 150
PARAMS = dict(min_score=20, min_count=1)


def contigs():
    """random contigs: the first seed from 31 on for which each 75-base half of the chimeric read holds a seed at k = 63, s = 31 too.  A
    half has 13 windows of 63 bases, fewer than the k - s + 1 = 33 that guarantee a closed syncmer, so the model of the sampler
    (tests/syncmer_model.py: the CPU hash, never the library's) says which contigs make (b) a fact there; at k = 15, s = 11 a half has
    61 windows and any contigs do."""
    for seed in range(31, 231):
        rng = random.Random(seed)
        ctg = {n: bytes(bases(rng, ln)) for n, ln in LENGTHS.items()}
        if all(kept_flags(np.frombuffer(h, dtype=np.uint8), 63, 31, True, "murmur", 42)[1].any() for h in (ctg["A"][-75:], ctg["B"][:75])):
            return ctg
    raise AssertionError("no seed gives both halves of the chimeric read a closed syncmer at k = 63")


def planted(ctg):
    """[(contig, place, reverse strand?, read)]: both ends and the middle of A and B on both strands, and C itself on both"""
    out = []
    for name in ("A", "B"):
        n = LENGTHS[name]
        for p in (0, 1, 777, n // 2, n - READ - 1, n - READ):
            for rv in (False, True):
                r = ctg[name][p:p + READ]
                out.append((name, p, rv, revcomp(r) if rv else r))
    for rv in (False, True):
        out.append(("C", 0, rv, revcomp(ctg["C"]) if rv else ctg["C"]))
    return out


def lay_out(reads):
    starts, ends, parts, at = [], [], [], 0
    for r in reads:
        starts.append(at); ends.append(at + len(r)); parts.append(r + b"\n"); at += len(r) + 1
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.array(starts, dtype=np.int64), np.array(ends, dtype=np.int64)


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def rows_inside_their_targets(T, mp):
    rs, re_ = host(mp.records.rs).view(np.uint32).astype(np.int64), host(mp.records.re).view(np.uint32).astype(np.int64)
    valid = host(mp.records.valid).astype(bool)
    t, _ = T.locate(rs)
    assert (t[valid] >= 0).all() and (re_[valid] <= T.ends.astype(np.int64)[t[valid]]).all() and (re_[valid] > rs[valid]).all()
    # the chain intervals of every row, valid or not, lie in one target too
    a, b = host(mp.table.r_start).view(np.uint32).astype(np.int64), host(mp.table.r_end).view(np.uint32).astype(np.int64)
    ta, _ = T.locate(a)
    tb, _ = T.locate(b - 1)
    assert (ta >= 0).all() and np.array_equal(ta, tb)


@pytest.fixture(scope="module")
def world():
    ctg = contigs()
    T = kh.Targets.from_sequences(list(LENGTHS), [ctg[n] for n in LENGTHS], spacer=32)
    assert T.starts.tolist() == [0, 3032, 5064] and int(T.ends[-1]) == 5214
    return ctg, T


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("cls,k,s", [("KmerPositionIndex", 15, 11), ("WideKmerPositionIndex", 63, 31)])
def test_reads_find_their_contig(world, cls, k, s, dev):
    ctg, T = world
    mk = to_dev if dev else (lambda a: a)
    plan = planted(ctg)
    chimera = ctg["A"][-75:] + ctg["B"][:75]
    seq, starts, ends_at = lay_out([r for _, _, _, r in plan] + [chimera])
    n_reads = len(plan) + 1
    ix = getattr(kh, cls)(k=k, s=s, stranded=True)
    try:
        ix.build_sequences(mk(T.text))
        mp = ix.map(mk(seq), mk(T.text), read_starts=starts, read_ends=ends_at, targets=T, **PARAMS)
        if dev:
            torch.cuda.synchronize()
        rows_inside_their_targets(T, mp)
        seg, rev, best = host(mp.table.seg).view(np.uint32), host(mp.table.rev), host(mp.select.best)
        flag, valid = host(mp.select.flag), host(mp.records.valid)
        rs, re_ = host(mp.records.rs).view(np.uint32).astype(np.int64), host(mp.records.re).view(np.uint32).astype(np.int64)
        qs, qe = host(mp.records.qs).view(np.uint32), host(mp.records.qe).view(np.uint32)
        toff, text = kh.cigar_text(mp.records.offsets, mp.records.ops)
        toff, text = host(toff), host(text).tobytes().decode()
        tgt, local = T.locate(rs)
        assert len(best) == n_reads and (np.diff(seg.astype(np.int64)) >= 0).all()
        # (a)
        for i, (name, place, rv, _) in enumerate(plan):
            c = int(best[i])
            assert c >= 0 and seg[c] == i and valid[c] and flag[c] & 1, (i, name, place, rv)
            assert T.names[int(tgt[c])] == name, (i, name, place, rv)
            assert (int(local[c]), int(re_[c]) - int(T.starts[tgt[c]])) == (place, place + READ) and (int(qs[c]), int(qe[c])) == (0, READ), (i, name, place, rv)
            assert bool(rev[c] & 1) == rv and text[toff[c]:toff[c + 1]] == "150=", (i, name, place, rv)
        # (b)
        rows = np.flatnonzero(seg == n_reads - 1)
        clips = host(mp.ends.clip).view(np.uint32)
        print("chimeric read: rows", rows.tolist(), "targets", tgt[rows].tolist(), "cigars", [text[toff[c]:toff[c + 1]] for c in rows],
              "clips", [(int(clips[2 * c]), int(clips[2 * c + 1])) for c in rows])
        assert len(rows) == 2 and sorted(T.names[int(t)] for t in tgt[rows]) == ["A", "B"]
        for c in rows:
            assert valid[c] and flag[c] & 2
            on_a = T.names[int(tgt[c])] == "A"
            assert (int(clips[2 * c]), int(clips[2 * c + 1])) == ((0, 75) if on_a else (75, 0))
            assert (int(qs[c]), int(qe[c])) == ((0, 75) if on_a else (75, 150))
            assert (int(local[c]), int(re_[c]) - int(T.starts[tgt[c]])) == ((LENGTHS["A"] - 75, LENGTHS["A"]) if on_a else (0, 75))
            assert text[toff[c]:toff[c + 1]] == ("75=75S" if on_a else "75S75=")
        # the PAF lines name each row's own target
        fh = io.StringIO()
        names = ["r%d" % i for i in range(n_reads)]
        written, skipped = kh.write_paf(fh, mp, names, targets=T)
        lines = [ln.split("\t") for ln in fh.getvalue().splitlines()]
        assert skipped == 0 and written == len(lines) >= n_reads + 1
        by_read = {}
        for f in lines:
            by_read.setdefault(f[0], []).append(f)
            assert int(f[6]) == LENGTHS[f[5]] and 0 <= int(f[7]) < int(f[8]) <= int(f[6])
        for i, (name, place, rv, _) in enumerate(plan):
            pri = [f for f in by_read[names[i]] if "tp:A:P" in f]
            assert len(pri) == 1 and pri[0][4:9] == ["-" if rv else "+", name, str(LENGTHS[name]), str(place), str(place + READ)]
        assert sorted(f[5:9] for f in by_read[names[-1]]) == [["A", "3000", "2925", "3000"], ["B", "2000", "0", "75"]]
        # the other calls take the keyword and agree with map
        tb = ix.chains(mk(seq), read_starts=starts, targets=T, **PARAMS)
        t2, sel = ix.chain_select(mk(seq), read_starts=starts, targets=T, **PARAMS)
        t3 = ix.chain_ends(mk(seq), mk(T.text), read_starts=starts, read_ends=ends_at, targets=T, **PARAMS)[0]
        g = ix.anchor_groups(mk(seq), read_starts=starts, targets=T)
        if dev:
            torch.cuda.synchronize()
        for other in (tb, t2, t3):
            assert all(np.array_equal(host(x), host(y)) for x, y in zip(list(other[:8]) + list(other.anchors) + [other.chain],
                                                                          list(mp.table[:8]) + list(mp.table.anchors) + [mp.table.chain]))
        assert np.array_equal(host(sel.best), best)
        assert all(np.array_equal(host(x), host(y)) for x, y in zip((g.qpos, g.rpos, g.rev), mp.table.anchors))
        gt = host(g.target).view(np.uint32)
        assert (gt != kh.TARGET_NONE).all() and (np.diff(host(g.offsets).view(np.uint64).astype(np.int64)) > 0).all()
    finally:
        ix.close()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("cls,k,s", [("KmerPositionIndex", 15, 11), ("WideKmerPositionIndex", 63, 31)])
def test_one_target_changes_nothing(world, cls, k, s, dev):
    ctg, _ = world
    mk = to_dev if dev else (lambda a: a)
    T1 = kh.Targets.from_sequences(["A"], [ctg["A"]], spacer=32)
    rng = random.Random(5)
    reads = []
    for t in range(24):                                          # both strands, and a few substitutions so that there is more than '='
        p = rng.randrange(0, LENGTHS["A"] - READ)
        r = bytearray(ctg["A"][p:p + READ])
        for _ in range(t % 3):
            x = rng.randrange(0, READ)
            r[x] = ord("ACGT"[("ACGT".index(chr(r[x])) + 1) % 4])
        reads.append(revcomp(bytes(r)) if t & 1 else bytes(r))
    seq, starts, ends_at = lay_out(reads)
    ix = getattr(kh, cls)(k=k, s=s, stranded=True)
    try:
        ix.build_sequences(mk(T1.text))
        a = ix.map(mk(seq), mk(T1.text), read_starts=starts, read_ends=ends_at, **PARAMS)
        b = ix.map(mk(seq), mk(T1.text), read_starts=starts, read_ends=ends_at, targets=T1, **PARAMS)
        if dev:
            torch.cuda.synchronize()
        flat = lambda m: list(m.table[:8]) + list(m.table.anchors) + [m.table.chain] + list(m.edits) + list(m.cigars) + list(m.ends) + list(m.select) + list(m.records)      # noqa: E731
        fa, fb = flat(a), flat(b)
        assert len(fa) == len(fb) and len(host(a.records.valid)) >= 8      # the eight exact reads hold a seed at either k; a substitution can cost a read of k = 63 all of its
        for i, (x, y) in enumerate(zip(fa, fb)):
            assert type(x) is type(y) and host(x).dtype == host(y).dtype and np.array_equal(host(x), host(y)), i
        names = ["r%d" % i for i in range(len(reads))]
        fa, fb = io.StringIO(), io.StringIO()
        assert kh.write_paf(fa, a, names, "A", LENGTHS["A"], k) == kh.write_paf(fb, b, names, targets=T1)
        assert fa.getvalue().splitlines() == fb.getvalue().splitlines() and len(fa.getvalue().splitlines()) >= 8
        rows_inside_their_targets(T1, b)
    finally:
        ix.close()
