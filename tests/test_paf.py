"""CPU: the formatting half of write_paf (kmers.paf_lines) over a numpy Mapping with the text passed in: the twelve PAF columns, the
tags in their order, s2 on primaries only, kept_only, rows without a whole alignment skipped and counted, ref_start taken off.  (write_paf
itself calls cigar_text, which stages through a device in host memory: tests/test_gpu_records_index.py holds it.)"""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import records_model as RM  # noqa: E402
from kmerhash_amd import kmers  # noqa: E402

Table = collections.namedtuple("Table", "seg rev q_start q_end r_start r_end count score anchors chain")
u32 = lambda *x: np.array(x, dtype=np.uint32)      # noqa: E731
u8 = lambda *x: np.array(x, dtype=np.uint8)        # noqa: E731


def mapping():
    run = lambda o, n: (n << 4) | o                # noqa: E731
    rows = [[run(4, 3), run(7, 40), run(8, 1), run(7, 20)], [run(7, 50), run(2, 2), run(7, 14)], [], [run(7, 64)]]
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    ops = u32(*[v for r in rows for v in r])
    table = Table(u32(0, 0, 1, 1), u8(0, 1, 0, 1), None, None, None, None, u32(9, 5, 4, 7), np.array([120, 70, 44, 90], dtype=np.int32), None, None)
    select = kmers.ChainSelect(None, None, u8(37, 0, 60, 0), u8(3, 2, 3, 0), np.array([70, 0, 0, 0], dtype=np.int32), None, None)
    records = kmers.ChainRecords(u8(1, 1, 0, 1), u32(3, 0, 0, 0), u32(64, 64, 0, 64), u32(1100, 5000, 0, 7000), u32(1161, 5066, 0, 7064), u32(64, 64, 80, 64), u32(60, 64, 0, 64),
                                 u32(61, 66, 0, 64), u32(1, 2, 0, 0), offs, ops)
    return kmers.Mapping(table, None, None, None, select, records)


def test_lines_columns_tags_and_skips():
    mp = mapping()
    toff, text = RM.cigar_text(mp.records.offsets, mp.records.ops)
    toff, text = np.array(toff, dtype=np.uint64), np.frombuffer(text, dtype=np.uint8)
    lines, skipped = kmers.paf_lines(mp, toff, text, ["r0", "r1"], "chr", 9000, 15, ref_start=1000)
    assert skipped == 1
    assert lines == ["r0\t64\t3\t64\t+\tchr\t9000\t100\t161\t60\t61\t37\ttp:A:P\tcm:i:9\ts1:i:120\ts2:i:70\tNM:i:1\tcg:Z:3S40=1X20=",
                     "r0\t64\t0\t64\t-\tchr\t9000\t4000\t4066\t64\t66\t0\ttp:A:S\tcm:i:5\ts1:i:70\tNM:i:2\tcg:Z:50=2D14="]
    lines, skipped = kmers.paf_lines(mp, toff, text, ["r0", "r1"], "chr", 9000, 15, kept_only=False)
    assert skipped == 1 and len(lines) == 3
    assert lines[2] == "r1\t64\t0\t64\t-\tchr\t9000\t7000\t7064\t64\t64\t0\ttp:A:S\tcm:i:7\ts1:i:90\tNM:i:0\tcg:Z:64="
    assert all(len(ln.split("\t")) == (18 if "tp:A:P" in ln else 17) for ln in lines)
