"""CPU: kmers.paf_lines(..., targets=T) over a hand-made numpy Mapping whose rows lie on three targets: columns 6 to 9 are the row's
own target name, that target's length and the target-local interval; everything else is as without targets; ref_name / ref_len /
ref_start must stay unset; a row whose interval lies in no single target is skipped and counted."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import records_model as RM  # noqa: E402
import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import kmers  # noqa: E402

Table = collections.namedtuple("Table", "seg rev q_start q_end r_start r_end count score anchors chain")
u32 = lambda *x: np.array(x, dtype=np.uint32)      # noqa: E731
u8 = lambda *x: np.array(x, dtype=np.uint8)        # noqa: E731
T = kh.Targets(["chrA", "plasmid", "tx7"], [3000, 2000, 150], spacer=32)      # [0, 3000), [3032, 5032), [5064, 5214)


def mapping(rs, re_):
    run = lambda o, n: (n << 4) | o                # noqa: E731
    rows = [[run(4, 3), run(7, 40), run(8, 1), run(7, 20)], [run(7, 50), run(2, 2), run(7, 14)], [run(7, 150)], [run(7, 64)], [run(7, 64)]]
    offs = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    ops = u32(*[v for r in rows for v in r])
    table = Table(u32(0, 0, 1, 2, 2), u8(0, 1, 0, 1, 0), None, None, None, None, u32(9, 5, 12, 7, 6), np.array([120, 70, 150, 90, 80], dtype=np.int32), None, None)
    select = kmers.ChainSelect(None, None, u8(37, 0, 60, 11, 0), u8(3, 2, 3, 3, 2), np.array([70, 0, 0, 80, 0], dtype=np.int32), None, None)
    records = kmers.ChainRecords(u8(1, 1, 1, 1, 1), u32(3, 0, 0, 0, 0), u32(64, 64, 150, 64, 64), u32(*rs), u32(*re_), u32(64, 64, 150, 64, 64),
                                 u32(60, 64, 150, 64, 64), u32(61, 66, 150, 64, 64), u32(1, 2, 0, 0, 0), offs, ops)
    mp = kmers.Mapping(table, None, None, None, select, records)
    toff, text = RM.cigar_text(offs, ops)
    return mp, np.array(toff, dtype=np.uint64), np.frombuffer(text, dtype=np.uint8)


def test_rows_on_three_targets():
    # row 0 on chrA, row 1 on the plasmid up to its last base, row 2 IS tx7, rows 3 and 4: one read on chrA's first base and on the plasmid
    mp, toff, text = mapping([100, 4966, 5064, 0, 3032], [161, 5032, 5214, 64, 3096])
    lines, skipped = kmers.paf_lines(mp, toff, text, ["r0", "r1", "r2"], targets=T)
    assert skipped == 0
    assert lines == ["r0\t64\t3\t64\t+\tchrA\t3000\t100\t161\t60\t61\t37\ttp:A:P\tcm:i:9\ts1:i:120\ts2:i:70\tNM:i:1\tcg:Z:3S40=1X20=",
                     "r0\t64\t0\t64\t-\tplasmid\t2000\t1934\t2000\t64\t66\t0\ttp:A:S\tcm:i:5\ts1:i:70\tNM:i:2\tcg:Z:50=2D14=",
                     "r1\t150\t0\t150\t+\ttx7\t150\t0\t150\t150\t150\t60\ttp:A:P\tcm:i:12\ts1:i:150\ts2:i:0\tNM:i:0\tcg:Z:150=",
                     "r2\t64\t0\t64\t-\tchrA\t3000\t0\t64\t64\t64\t11\ttp:A:P\tcm:i:7\ts1:i:90\ts2:i:80\tNM:i:0\tcg:Z:64=",
                     "r2\t64\t0\t64\t+\tplasmid\t2000\t0\t64\t64\t64\t0\ttp:A:S\tcm:i:6\ts1:i:80\tNM:i:0\tcg:Z:64="]
    # without targets the same rows print one name and whole-text coordinates, as before
    plain, _ = kmers.paf_lines(mp, toff, text, ["r0", "r1", "r2"], "all", 5214, 15)
    assert [ln.split("\t")[5:9] for ln in plain] == [["all", "5214", "100", "161"], ["all", "5214", "4966", "5032"], ["all", "5214", "5064", "5214"],
                                                      ["all", "5214", "0", "64"], ["all", "5214", "3032", "3096"]]
    assert [ln.split("\t")[:5] + ln.split("\t")[9:] for ln in plain] == [ln.split("\t")[:5] + ln.split("\t")[9:] for ln in lines]


def test_a_row_outside_every_target_is_skipped():
    # row 1 runs one base into the spacer behind the plasmid, row 3 starts in the spacer before it, row 4 lies beyond the last target
    mp, toff, text = mapping([100, 4966, 5064, 3031, 5214], [161, 5033, 5214, 3095, 5278])
    lines, skipped = kmers.paf_lines(mp, toff, text, ["r0", "r1", "r2"], targets=T)
    assert skipped == 3 and [ln.split("\t")[5] for ln in lines] == ["chrA", "tx7"]


def test_one_name_and_targets_exclude_each_other():
    mp, toff, text = mapping([100, 4966, 5064, 0, 3032], [161, 5032, 5214, 64, 3096])
    for kw in (dict(ref_name="x"), dict(ref_len=9), dict(ref_start=5), dict(ref_name="x", ref_len=9)):
        with pytest.raises(ValueError, match="with targets"):
            kmers.paf_lines(mp, toff, text, ["r0", "r1", "r2"], targets=T, **kw)
    with pytest.raises(ValueError, match="without targets"):
        kmers.paf_lines(mp, toff, text, ["r0", "r1", "r2"])
