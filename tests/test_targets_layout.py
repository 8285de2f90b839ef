"""CPU: kmerhash_amd.Targets, the contig table of a reference of several sequences: the layout arithmetic, from_sequences and
from_fasta (wrapped lines, lower case, a contig of one base, exactly `spacer` bytes of N between contigs), locate on every boundary
byte, and every refusal."""
import numpy as np
import pytest

import kmerhash_amd as kh


def test_layout_arithmetic():
    T = kh.Targets(["a", "b", "c", "d"], [10, 1, 300, 7], spacer=40)
    assert T.starts.dtype == np.uint32 and T.ends.dtype == np.uint32 and T.text is None and T.spacer == 40 and len(T) == 4
    assert T.names == ["a", "b", "c", "d"] and T.lengths.tolist() == [10, 1, 300, 7]
    assert T.starts[0] == 0
    for t in range(4):
        assert T.ends[t] == T.starts[t] + T.lengths[t]
        if t:
            assert T.starts[t] == T.ends[t - 1] + 40
    assert T.starts.tolist() == [0, 50, 91, 431] and T.ends.tolist() == [10, 51, 391, 438]
    assert kh.Targets(["x"], [5]).spacer == 64
    one = kh.Targets([b"only"], [2 ** 31])                          # the whole coordinate space
    assert one.names == ["only"] and one.ends.tolist() == [2 ** 31]


def test_from_sequences_round_trip():
    seqs = [b"ACGTacgtNN", b"g", np.frombuffer(b"TTTTTTTTTT" * 30, dtype=np.uint8), "GATTACA"]
    T = kh.Targets.from_sequences(["a", "b", "c", "d"], seqs, spacer=40)
    assert T.text.dtype == np.uint8 and len(T.text) == T.ends[-1] == 438
    raw = T.text.tobytes()
    for t, s in enumerate([b"ACGTacgtNN", b"g", b"TTTTTTTTTT" * 30, b"GATTACA"]):
        assert raw[int(T.starts[t]):int(T.ends[t])] == s            # lower case and N stay as they are
        if t:
            assert raw[int(T.ends[t - 1]):int(T.starts[t])] == b"N" * 40
    assert kh.Targets.from_sequences(["x"], [b"ACGT"]).text.tobytes() == b"ACGT"


@pytest.mark.parametrize("spacer", [32, 64])
def test_from_fasta_round_trip(spacer):
    fasta = (b"junk before the first header\n>chr1 first contig, wrapped\nACGTAC\nGTAC\n\nGT\n>one\tbase\na\n>lower case\nacgtn\r\nACG T\n>last no newline at the end\nGGG\nCC")
    T = kh.Targets.from_fasta(fasta, spacer=spacer)
    assert T.names == ["chr1", "one", "lower", "last"] and T.lengths.tolist() == [12, 1, 9, 5] and T.spacer == spacer
    S = kh.Targets.from_sequences(T.names, [b"ACGTACGTACGT", b"a", b"acgtnACGT", b"GGGCC"], spacer=spacer)
    assert T.text.tobytes() == S.text.tobytes() and T.starts.tolist() == S.starts.tolist() and T.ends.tolist() == S.ends.tolist()
    raw = T.text.tobytes()
    assert raw == (b"N" * spacer).join([b"ACGTACGTACGT", b"a", b"acgtnACGT", b"GGGCC"])
    assert kh.Targets.from_fasta(np.frombuffer(fasta, dtype=np.uint8), spacer=spacer).text.tobytes() == raw      # an array will do
    assert kh.Targets.from_fasta(b">x\nAC\n>y\nG\n").text.tobytes() == b"AC" + b"N" * 64 + b"G"


def test_from_fasta_refusals():
    for bad in (b"", b"ACGT\n", b">a\nAC\n>b\n\n", b">a\nAC\n>a\nGG\n", b">\nAC\n", b">a\n"):
        with pytest.raises(ValueError):
            kh.Targets.from_fasta(bad)


def test_locate_on_every_boundary_byte():
    T = kh.Targets(["a", "b", "c"], [10, 1, 300], spacer=32)       # [0, 10), [42, 43), [75, 375)
    pos = [0, 9, 10, 41, 42, 43, 74, 75, 374, 375, 376, 2 ** 31, 2 ** 32 - 1]
    tgt = [0, 0, -1, -1, 1, -1, -1, 2, 2, -1, -1, -1, -1]
    loc = [0, 9, 0, 0, 0, 0, 0, 0, 299, 0, 0, 0, 0]
    for dt in (np.int64, np.uint32, np.uint64):
        t, l = T.locate(np.array(pos, dtype=dt))
        assert t.dtype == np.int64 and l.dtype == np.int64 and t.tolist() == tgt and l.tolist() == loc
    t, l = T.locate(np.array(pos, dtype=np.uint32).view(np.int32))      # uint32 bits in an int32 container, as the device arrays hold them
    assert t.tolist() == tgt and l.tolist() == loc
    # every byte of the layout, against the definition
    every = np.arange(0, 400)
    t, l = T.locate(every)
    for p in every:
        hit = [i for i in range(3) if T.starts[i] <= p < T.ends[i]]
        assert (t[p], l[p]) == ((hit[0], p - T.starts[hit[0]]) if hit else (-1, 0)), p
    t, l = T.locate(np.zeros(0, dtype=np.uint32))
    assert len(t) == 0 and len(l) == 0


def test_refusals():
    ok = dict(names=["a", "b"], lengths=[5, 6])
    kh.Targets(**ok, spacer=32)
    for kw in (dict(spacer=31), dict(spacer=0), dict(spacer=-1), dict(names=[], lengths=[]), dict(lengths=[5, 0]), dict(lengths=[0, 6]), dict(lengths=[5, -1]),
               dict(names=["a", "a"]), dict(names=["a", b"a"]), dict(lengths=[5]), dict(names=["a"]), dict(lengths=[2 ** 31, 1]), dict(lengths=[2 ** 31 - 64 - 5, 6])):
        with pytest.raises(ValueError):
            kh.Targets(**dict(ok, **kw))
    assert kh.Targets(["a", "b"], [2 ** 31 - 64 - 6, 6]).ends[-1] == 2 ** 31      # ends[-1] == 2^31 is the last that fits
    with pytest.raises(ValueError):
        kh.Targets.from_sequences(["a", "b"], [b"ACGT", b""])
    with pytest.raises(ValueError):
        kh.Targets.from_sequences(["a"], [b"ACGT"], spacer=8)
