"""GPU: FASTQ in, SAM out.  40 reads of 100-150 bases cut from a 20 kb reference of two contigs, both strands, every fifth with a
substitution and a deletion, written as FASTQ; 20 fragments as two files for the paired case.  ix.map_fastq / ix.map_fastq_pairs and
write_sam_bytes over the Reads they return must give the file that the existing path -- a hand-built seq, read_starts, names list and
qual through ix.map / ix.map_pairs and write_sam / write_sam_pairs -- gives, byte for byte, on numpy arrays and on CUDA tensors;
benchmark/read_mapper.main writes the same file.  Mismatched mate names and unequal counts raise under strict; a bad record in the middle
comes out, under strict=False, as an unmapped read with SEQ '*' whose mate is still read 2p + 1."""
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "benchmark"))

import kmerhash_amd as kh  # noqa: E402
from stream_checks import to_dev  # noqa: E402

K_, W_ = 15, 5
CUT, REF_LEN = 9000, 20000
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def edited(rng, s):
    """one substitution and one deleted base"""
    i, j = int(rng.randint(20, 50)), int(rng.randint(60, 90))
    return s[:i] + bytes([COMP[s[i]]]) + s[i + 1:j] + s[j + 1:]


def fastq(names, seqs, quals):
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(names, seqs, quals))


def hand_built(seqs, quals):
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lens + 1)[:-1]]).astype(np.int64)
    join = lambda rows: np.frombuffer(b"".join(r + b"\n" for r in rows), dtype=np.uint8).copy()      # noqa: E731
    return join(seqs), join(quals), starts, starts + lens


@pytest.fixture(scope="module")
def world():
    rng = np.random.RandomState(17)
    ref = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=REF_LEN))
    contigs = [ref[:CUT], ref[CUT:]]
    T = kh.Targets.from_sequences(["ctgA", "ctgB"], contigs)
    fasta = b"".join(b">%s some words\n" % n + b"".join(c[i:i + 70] + b"\n" for i in range(0, len(c), 70)) for n, c in zip((b"ctgA", b"ctgB"), contigs))
    cut = lambda n: (lambda c, a: contigs[c][a:a + n])(int(rng.randint(0, 2)), int(rng.randint(0, CUT - 500)))      # noqa: E731
    seqs = []
    for i in range(40):
        s = cut(int(rng.randint(100, 151)))
        s = edited(rng, s) if i % 5 == 4 else s
        seqs.append(revcomp(s) if i % 2 else s)
    quals = [bytes(rng.randint(35, 74, size=len(s)).astype(np.uint8)) for s in seqs]
    names = ["read%d" % i for i in range(40)]
    single = dict(text=fastq([b"%s extra words" % n.encode() for n in names], seqs, quals), seqs=seqs, quals=quals, names=names)
    m1, m2 = [], []
    for p in range(20):
        f = cut(int(rng.randint(300, 401)))
        f = revcomp(f) if p % 2 else f
        a, b = f[:120], revcomp(f[-110:])
        m1.append(edited(rng, a) if p % 5 == 3 else a)
        m2.append(b)
    q1, q2 = ([bytes(rng.randint(35, 74, size=len(s)).astype(np.uint8)) for s in m] for m in (m1, m2))
    paired = dict(text1=fastq([b"frag%d/1" % p for p in range(20)], m1, q1), text2=fastq([b"frag%d/2 c" % p for p in range(20)], m2, q2), m1=m1, m2=m2, q1=q1, q2=q2,
                  seqs=[s for pair in zip(m1, m2) for s in pair], quals=[q for pair in zip(q1, q2) for q in pair], names=["frag%d" % (s // 2) for s in range(40)])
    return dict(T=T, fasta=fasta, single=single, paired=paired)


def index(rt):
    ix = kh.KmerPositionIndex(k=K_, w=W_, stranded=True)
    ix.build_sequences(rt)
    return ix


def body_flags(sam):
    return [int(l.split(b"\t")[1]) for l in sam.splitlines() if not l.startswith(b"@")]


@pytest.mark.parametrize("dev", [False, True], ids=["numpy", "tensors"])
def test_map_fastq_gives_the_file_of_the_hand_built_path(world, dev):
    T, S = world["T"], world["single"]
    mk = to_dev if dev else (lambda a: a)
    rt = mk(T.text.copy())
    seq, qual, starts, ends = hand_built(S["seqs"], S["quals"])
    ix = index(rt)
    try:
        want_mp = ix.map(mk(seq), rt, read_starts=starts, read_ends=ends, targets=T)
        mp, reads = ix.map_fastq(mk(np.frombuffer(S["text"], dtype=np.uint8).copy()), rt, targets=T)
    finally:
        ix.close()
    fh, bh, gh = io.StringIO(), io.BytesIO(), io.BytesIO()
    kh.write_sam(fh, want_mp, mk(seq), rt, S["names"], starts, ends, qual=mk(qual), targets=T)
    kh.write_sam_bytes(bh, want_mp, mk(seq), rt, S["names"], starts, ends, qual=mk(qual), targets=T)
    got = kh.write_sam_bytes(gh, mp, reads.seq, rt, reads.names, reads.read_starts, reads.read_ends, qual=reads.qual, targets=T)
    assert gh.getvalue() == bh.getvalue() == fh.getvalue().encode()
    flags = body_flags(gh.getvalue())
    assert got[0] >= 20 and 0 in flags and 16 in flags, (got, sorted(set(flags)))      # at least half the reads, of both strands, were mapped and printed
    assert reads.n_reads == 40 and (reads.seq.is_cuda if dev else isinstance(reads.seq, np.ndarray))


@pytest.mark.parametrize("dev", [False, True], ids=["numpy", "tensors"])
def test_map_fastq_pairs_gives_the_file_of_the_hand_built_path(world, dev):
    T, P = world["T"], world["paired"]
    mk = to_dev if dev else (lambda a: a)
    up = lambda b: mk(np.frombuffer(b, dtype=np.uint8).copy())      # noqa: E731
    rt = mk(T.text.copy())
    seq, qual, starts, ends = hand_built(P["seqs"], P["quals"])
    woven = b"".join(x for p in range(20) for x in (fastq([b"frag%d/1" % p], [P["m1"][p]], [P["q1"][p]]), fastq([b"frag%d/2" % p], [P["m2"][p]], [P["q2"][p]])))
    ix = index(rt)
    try:
        want_mp, want_pr = ix.map_pairs(mk(seq), rt, starts, ends, targets=T)
        mp, pr, reads = ix.map_fastq_pairs(up(P["text1"]), rt, up(P["text2"]), targets=T)
        mp2, pr2, reads2 = ix.map_fastq_pairs(up(woven), rt, strip_mate=True, targets=T)
        mp3, pr3, rescue, reads3 = ix.map_fastq_pairs(up(P["text1"]), rt, up(P["text2"]), rescue=True, targets=T)
        with pytest.raises(ValueError, match="an even number of reads is needed, got 39"):
            ix.map_fastq_pairs(up(woven[:woven.rindex(b"@frag19/2")]), rt, strip_mate=True, targets=T)
    finally:
        ix.close()
    fh = io.StringIO()
    kh.write_sam_pairs(fh, want_mp, want_pr, mk(seq), rt, P["names"], starts, ends, qual=mk(qual), targets=T)
    for m, p, r in ((mp, pr, reads), (mp2, pr2, reads2), (mp3, pr3, reads3)):
        gh = io.BytesIO()
        kh.write_sam_bytes(gh, m, r.seq, rt, r.names, r.read_starts, r.read_ends, qual=r.qual, targets=T, pairs=p)
        assert gh.getvalue() == fh.getvalue().encode()
    flags = body_flags(fh.getvalue().encode())
    assert sum(1 for f in flags if f & 0x2) >= 10 and any(f & 0x40 for f in flags) and any(f & 0x80 for f in flags), sorted(set(flags))
    assert isinstance(rescue, kh.MateRescue)


def test_read_mapper_main_writes_the_same_file(world, tmp_path):
    import read_mapper
    T, S, P = world["T"], world["single"], world["paired"]
    for name, data in (("ref.fa", world["fasta"]), ("reads.fq", S["text"]), ("r_1.fq", P["text1"]), ("r_2.fq", P["text2"])):
        (tmp_path / name).write_bytes(data)
    rt = to_dev(T.text.copy())
    ix = index(rt)
    try:
        seq, qual, starts, ends = hand_built(S["seqs"], S["quals"])
        fh = io.StringIO()
        kh.write_sam(fh, ix.map(to_dev(seq), rt, read_starts=starts, read_ends=ends, targets=T), to_dev(seq), rt, S["names"], starts, ends, qual=to_dev(qual), targets=T)
        pseq, pqual, pstarts, pends = hand_built(P["seqs"], P["quals"])
        ph = io.StringIO()
        pm, pp = ix.map_pairs(to_dev(pseq), rt, pstarts, pends, targets=T)
        kh.write_sam_pairs(ph, pm, pp, to_dev(pseq), rt, P["names"], pstarts, pends, qual=to_dev(pqual), targets=T)
    finally:
        ix.close()
    opts = ["-k", str(K_), "-w", str(W_)]
    read_mapper.main([str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq"), "-o", str(tmp_path / "out.sam")] + opts)
    assert (tmp_path / "out.sam").read_bytes() == fh.getvalue().encode()
    read_mapper.main([str(tmp_path / "ref.fa"), str(tmp_path / "r_1.fq"), str(tmp_path / "r_2.fq"), "-o", str(tmp_path / "pairs.sam")] + opts)
    assert (tmp_path / "pairs.sam").read_bytes() == ph.getvalue().encode()


def test_strict_refusals_and_a_bad_record_in_the_middle(world):
    T, P = world["T"], world["paired"]
    up = lambda b: to_dev(np.frombuffer(b, dtype=np.uint8).copy())      # noqa: E731
    rt = to_dev(T.text.copy())
    renamed = fastq([b"frag%d/2" % (p if p != 7 else 70) for p in range(20)], P["m2"], P["q2"])
    fewer = fastq([b"frag%d/2" % p for p in range(18)], P["m2"][:18], P["q2"][:18])
    bad = fastq([b"frag%d/2" % p for p in range(20)], P["m2"], [q if p != 7 else q[:-3] for p, q in enumerate(P["q2"])])
    ix = index(rt)
    try:
        with pytest.raises(ValueError, match="record 7 carries different names"):
            ix.map_fastq_pairs(up(P["text1"]), rt, up(renamed), targets=T)
        with pytest.raises(ValueError, match="hold 20 and 18 records: record 18 has no mate"):
            ix.map_fastq_pairs(up(P["text1"]), rt, up(fewer), targets=T)
        with pytest.raises(ValueError, match="record 7 of text 2 is malformed"):
            ix.map_fastq_pairs(up(P["text1"]), rt, up(bad), targets=T)
        mp, pr, reads = ix.map_fastq_pairs(up(P["text1"]), rt, up(bad), strict=False, targets=T)
    finally:
        ix.close()
    assert reads.n_reads == 40 and reads.status.cpu().tolist() == [4 if s == 15 else 0 for s in range(40)]
    starts, ends = reads.read_starts.cpu().numpy(), reads.read_ends.cpu().numpy()
    seq = reads.seq.cpu().numpy().tobytes()
    assert ends[15] == starts[15] and seq[starts[14]:ends[14]] == P["m1"][7] and seq[starts[16]:ends[16]] == P["m1"][8] and seq[starts[17]:ends[17]] == P["m2"][8]
    gh = io.BytesIO()
    kh.write_sam_bytes(gh, mp, reads.seq, rt, reads.names, reads.read_starts, reads.read_ends, qual=reads.qual, targets=T, pairs=pr)
    lines = [l.split(b"\t") for l in gh.getvalue().splitlines() if l.startswith(b"frag7\t")]
    mate2 = [l for l in lines if int(l[1]) & 0x80]
    assert len(mate2) == 1 and int(mate2[0][1]) & 0x4 and mate2[0][9] == b"*" and mate2[0][10] == b"*"
    assert any(int(l[1]) & 0x40 and not int(l[1]) & 0x4 and l[9] in (P["m1"][7], revcomp(P["m1"][7])) for l in lines)      # its mate is mapped, and is read 2p
