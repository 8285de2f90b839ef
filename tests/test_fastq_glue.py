"""CPU: read_fastq_glue, the array glue of read_fastq(), with the two device calls replaced by their models (tests/fastq_model.py):
over numpy it must give what the model's read_fastq states record by record -- one text and two, strict and not --, its ValueErrors
must name the first offending record, and the torch-CPU namespace must give the same arrays.  No GPU, no library call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _xp, fastq  # noqa: E402
import fastq_cases as FC  # noqa: E402
import fastq_model as FM  # noqa: E402

NP = _xp.NUMPY


def records(text, strip):
    rows, n_bad, tail = FM.fastq_records(bytes(text), FM.STRIP_MATE if strip else 0)
    cols = [np.array([r[i] for r in rows], dtype=np.uint32) for i in range(5)] + [np.array([r[5] for r in rows], dtype=np.uint8)]
    return kh.FastqRecords(*cols, n_bad, tail)


def pack(text, lo, hi, dst, out_len, sep, out):
    """pack_rows through the model, in place, on numpy arrays or CPU tensors"""
    h = lambda x: (x.numpy() if hasattr(x, "numpy") else np.asarray(x))      # noqa: E731
    assert len(out) == out_len
    got = FM.pack_rows(bytes(h(text)), [int(v) for v in h(lo)], [int(v) for v in h(hi)], [int(v) for v in h(dst)], -1 if sep is None else sep, bytearray(h(out).tobytes()))
    h(out)[:] = np.frombuffer(bytes(got), dtype=np.uint8)      # (a CPU tensor shares its memory with its numpy view)
    return out


def glue(xp, texts, strict, strip=None, wrap=lambda a: a):
    strip = len(texts) == 2 if strip is None else strip
    arrays = [np.frombuffer(t, dtype=np.uint8).copy() for t in texts]
    recs = [type(r)(*(wrap(c) for c in r[:6]), r.n_bad, r.tail_lines) for r in (records(t, strip) for t in texts)]
    return fastq.read_fastq_glue(xp, [wrap(a) for a in arrays], recs, strict, pack)


def check(got, want):
    h = lambda x: (x.numpy() if hasattr(x, "numpy") else np.asarray(x))      # noqa: E731
    assert h(got.seq).tobytes() == want["seq"] and h(got.qual).tobytes() == want["qual"]
    assert h(got.read_starts).tolist() == want["read_starts"] and h(got.read_ends).tolist() == want["read_ends"]
    assert h(got.names[0]).astype(np.int64).tolist() == want["names"][0] and h(got.names[1]).tobytes() == want["names"][1]
    assert got.n_reads == want["n_reads"] and h(got.status).tolist() == want["status"]


@pytest.mark.parametrize("case", sorted(FC.CASES))
def test_one_text(case):
    c = FC.CASES[case]
    want = FM.read_fastq([c.text])
    got = glue(NP, [c.text], strict=False)
    check(got, want)
    assert got.seq.dtype == got.qual.dtype == got.names[1].dtype == got.status.dtype == np.uint8 and got.read_starts.dtype == got.read_ends.dtype == np.int64
    assert got.names[0].dtype == np.uint64
    if sum(want["n_bad"]) or sum(want["tail_lines"]):
        with pytest.raises(ValueError, match="record %d of text 1 is malformed" % next(i for i, s in enumerate(want["status"]) if s) if sum(want["n_bad"])
                           else "text 1 ends inside a record: %d lines follow its %d whole records" % (want["tail_lines"][0], want["n_reads"])):
            glue(NP, [c.text], strict=True)
    else:
        check(glue(NP, [c.text], strict=True), want)


def test_two_texts():
    one, two, r1, r2 = FC.pair_texts()
    check(glue(NP, [one, two], strict=True), FM.read_fastq([one, two]))
    check(glue(NP, [one, two], strict=False, strip=False), FM.read_fastq([one, two], False))
    with pytest.raises(ValueError, match="record 0 carries different names"):      # frag0/1 against frag0/2
        glue(NP, [one, two], strict=True, strip=False)
    # a name of another length in record 17; a name of the same length and other bytes in record 23; both: the first one is named
    renamed = lambda recs, p, name: recs[:p] + [(b"@" + name,) + recs[p][1:]] + recs[p + 1:]      # noqa: E731
    other = lambda recs, p, name: FC.write(renamed(recs, p, name))      # noqa: E731
    with pytest.raises(ValueError, match="record 17 carries different names"):
        glue(NP, [one, other(r2, 17, b"frag170/2")], strict=True)
    with pytest.raises(ValueError, match="record 23 carries different names"):
        glue(NP, [one, other(r2, 23, b"frag32/2")], strict=True)
    with pytest.raises(ValueError, match="record 17 carries different names"):
        glue(NP, [other(renamed(r1, 23, b"frag32/1"), 17, b"f/1"), two], strict=True)
    check(glue(NP, [one, other(r2, 23, b"frag32/2")], strict=False), FM.read_fastq([one, other(r2, 23, b"frag32/2")]))
    # unequal counts
    short = FC.write(r2[:-3])
    with pytest.raises(ValueError, match="hold 60 and 57 records: record 57 has no mate"):
        glue(NP, [one, short], strict=True)
    for pair in ([one, short], [short, one]):
        check(glue(NP, pair, strict=False), FM.read_fastq(pair))
    # a bad record in the middle of the second text: an empty read, and its mate is still read 2p
    bad = FC.write(r2[:9] + [(b"@frag9/2", r2[9][1], b"+", r2[9][3][:-1])] + r2[10:])
    got = glue(NP, [one, bad], strict=False)
    check(got, FM.read_fastq([one, bad]))
    assert got.status.tolist() == [4 if s == 19 else 0 for s in range(120)] and got.read_ends[19] == got.read_starts[19]
    assert got.seq[got.read_starts[18]:got.read_ends[18]].tobytes() == r1[9][1] and got.seq[got.read_starts[20]:got.read_ends[20]].tobytes() == r1[10][1]
    with pytest.raises(ValueError, match="record 9 of text 2 is malformed: its quality line is not as long"):
        glue(NP, [one, bad], strict=True)


def test_the_torch_namespace_gives_the_same_arrays():
    torch = pytest.importorskip("torch")
    from test_array_namespace import same, tensor
    TT = _xp.Torch(torch.device("cpu"))
    one, two, r1, r2 = FC.pair_texts()
    for texts, strict in (([FC.CASES["many"].text], True), ([FC.CASES["length_mismatch"].text], False), ([FC.CASES["empty"].text], True), ([one, two], True),
                          ([one, FC.write(r2[:-3])], False)):
        a, b = glue(NP, texts, strict), glue(TT, texts, strict, wrap=tensor)
        for x, y, dt in ((a.seq, b.seq, np.uint8), (a.qual, b.qual, np.uint8), (a.read_starts, b.read_starts, np.int64), (a.read_ends, b.read_ends, np.int64),
                         (a.names[0], b.names[0], np.uint64), (a.names[1], b.names[1], np.uint8), (a.status, b.status, np.uint8)):
            same(x, y, dt)
        assert a.n_reads == b.n_reads
    with pytest.raises(ValueError, match="record 0 carries different names"):
        glue(TT, [one, two], True, strip=False, wrap=tensor)
    with pytest.raises(ValueError, match="record 1 of text 1 is malformed"):
        glue(TT, [FC.CASES["missing_at"].text], True, wrap=tensor)
