"""CPU: sam_lines(pairs=) on a hand-made Mapping and PairSelect, every line written out by hand: a representative that is a secondary of
select (its parent is then printed 0x100 and the representative carries SEQ, the pair's quality and TLEN), a second primary of a read
(0x800), a read whose mate is unmapped (0x8, and the mate placed at its position), a pair without any row; pairs=None gives the lines the
function gives without the keyword."""
import collections

import numpy as np

import kmerhash_amd as kh
from kmerhash_amd.index import ChainTable

Rec = collections.namedtuple("Rec", "valid rs re nm")

#        seg rev cnt score | flag mapq sub parent | rs    re   nm  cigar     seq
ROWS = [(0, 0, 5, 90, 3, 0, 88, 0, 100, 200, 0, "100=", "AAAA"),
        (0, 0, 5, 88, 2, 0, 0, 0, 5100, 5200, 1, "100=", "AAAA"),
        (1, 1, 6, 95, 3, 50, 0, 2, 5400, 5500, 0, "100=", "CCCC"),
        (2, 0, 7, 99, 3, 60, 0, 3, 200, 260, 0, "60=40S", "GGGG"),
        (2, 1, 3, 40, 3, 20, 0, 4, 9000, 9040, 2, "60S40=", "TTTT")]
N_READS = 6
READS = ["aaaa", "cccc", "gggg", "tttt", "acac", "gtgt"]      # as given (what an unmapped read prints)


def csr(strings):
    offs = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.uint64)
    return offs, np.frombuffer("".join(strings).encode(), dtype=np.uint8)


def mapping():
    col = lambda i, dt: np.array([r[i] for r in ROWS], dtype=dt)      # noqa: E731
    n = len(ROWS)
    table = ChainTable(col(0, np.uint32), col(1, np.uint8), None, None, None, None, col(2, np.uint32), col(3, np.int32), None, None)
    select = kh.ChainSelect(col(7, np.int32), np.zeros(n, dtype=np.uint32), col(5, np.uint8), col(4, np.uint8), col(6, np.int32), np.zeros(n, dtype=np.uint32),
                            np.array([0, 2, 3, -1, -1, -1], dtype=np.int32))
    return kh.Mapping(table, None, None, None, select, Rec(np.ones(n, dtype=np.uint8), col(8, np.uint32), col(9, np.uint32), col(10, np.uint32)))


PAIRS = kh.PairSelect(np.array([1, 2, 3, -1, -1, -1], dtype=np.int32), np.array([60, 60, 60, 0, 0, 0], dtype=np.uint8), np.array([400, -400, 0, 0, 0, 0], dtype=np.int32),
                      np.array([7, 0, 0], dtype=np.uint8), np.array([183, 0, 0], dtype=np.int32), np.array([1, 0, 0], dtype=np.uint32))

EXPECT = [
    "r0 353 ref 101 0 100= = 5401 0 * * NM:i:0 tp:A:S cm:i:5 s1:i:90",
    "r0 99 ref 5101 60 100= = 5401 400 AAAA * NM:i:1 tp:A:P cm:i:5 s1:i:88 s2:i:0",
    "r1 147 ref 5401 60 100= = 5101 -400 CCCC * NM:i:0 tp:A:P cm:i:6 s1:i:95 s2:i:0",
    "r2 73 ref 201 60 60=40S = 201 0 GGGG * NM:i:0 tp:A:P cm:i:7 s1:i:99 s2:i:0",
    "r2 2137 ref 9001 20 60S40= = 201 0 TTTT * NM:i:2 tp:A:P cm:i:3 s1:i:40 s2:i:0",
    "r3 133 ref 201 0 * = 201 0 tttt *",
    "r4 77 * 0 0 * * 0 0 acac *",
    "r5 141 * 0 0 * * 0 0 gtgt *",
]


def lines(**kw):
    toff, text = csr([r[11] for r in ROWS])
    seq_rows = csr([r[12] for r in ROWS] + READS)
    return kh.sam_lines(mapping(), toff, text, seq_rows, ["r%d" % i for i in range(N_READS)], ref_name="ref", ref_len=20000, header=False, **kw)


def test_every_line_of_the_paired_output():
    got, skipped, n_unmapped = lines(pairs=PAIRS)
    assert [l.replace("\t", " ") for l in got] == EXPECT
    assert (skipped, n_unmapped) == (0, 3)


def test_unmapped_false_drops_the_reads_without_a_representative():
    got, skipped, n_unmapped = lines(pairs=PAIRS, unmapped=False)
    assert [l.replace("\t", " ") for l in got] == EXPECT[:5] and n_unmapped == 3


def test_a_row_of_another_read_is_no_representative():
    p = PAIRS._replace(row=np.array([2, 2, 3, -1, -1, -1], dtype=np.int32))      # row 2 belongs to read 1
    got, skipped, n_unmapped = lines(pairs=p)
    assert got[0].split("\t")[:4] == ["r0", str(0x1 | 0x40 | 0x4 | 0x20), "ref", "5401"] and (skipped, n_unmapped) == (2, 4)


def test_with_targets_rnext_names_the_other_target():
    T = kh.Targets(["ctgA", "ctgB"], [6000, 6000], spacer=64)      # ctgB starts at 6064
    toff, text = csr([r[11] for r in ROWS])
    seq_rows = csr([r[12] for r in ROWS] + READS)
    p = PAIRS._replace(row=np.array([0, 2, 3, -1, -1, -1], dtype=np.int32), flag=np.array([2, 0, 0], dtype=np.uint8), tlen=np.zeros(6, dtype=np.int32))
    got, _, _ = kh.sam_lines(mapping(), toff, text, seq_rows, ["r%d" % i for i in range(N_READS)], targets=T, header=False, pairs=p)
    f = [l.split("\t") for l in got]
    assert f[0][:9] == ["r0", str(0x1 | 0x40 | 0x20), "ctgA", "101", "60", "100=", "=", "5401", "0"]      # rows 0 and 2 on ctgA
    assert f[4][:9] == ["r2", str(0x1 | 0x40 | 0x8 | 0x10 | 0x800), "ctgB", str(9000 - 6064 + 1), "20", "60S40=", "ctgA", "201", "0"]


def test_pairs_none_is_the_output_without_the_keyword():
    assert lines(pairs=None) == lines()
    got, skipped, n_unmapped = lines()
    assert [l.split("\t")[1] for l in got] == ["0", "256", "16", "0", "2064", "4", "4", "4"] and all(l.split("\t")[6:9] == ["*", "0", "0"] for l in got)
