"""CPU: sam_line_columns, the array glue of the device SAM path, over numpy: its columns through the model of kh_sam_lines
(tests/samtext_model.py) must give the very bytes of sam_lines(), and the same triple -- on the hand-made Mapping of
test_sam_lines.py (a read with no rows, a read whose best row is not printable, kept_only=False, unmapped=False, targets, with and
without difference strings and QUAL), on a Mapping with a row that straddles a spacer, and on the hand-made Mapping and PairSelect of
test_sam_pairs_lines.py with PairSelects for two unmapped mates, a mapped mate with an unmapped partner, a pair on different targets
and a representative that is not select.best.  The torch-CPU namespace must give the same columns.  No GPU, no library call beyond
sam_header's version string."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _xp, sam  # noqa: E402
import samtext_model as SM  # noqa: E402
import test_sam_lines as U  # noqa: E402
import test_sam_pairs_lines as P  # noqa: E402

NP = _xp.NUMPY


def model_text(mapping, L, names, tnames, cigars, seq_rows, qual_rows, md, cs):
    h = lambda pair: None if pair is None else ([int(x) for x in pair[0]], bytes(np.asarray(pair[1])))      # noqa: E731
    cols = {k: [int(v) for v in getattr(L, k)] for k in SM.COLUMNS}
    return SM.sam_lines(h(sam.names_csr(names)), h(sam.names_csr(tnames)), h(cigars), h(seq_rows), h(qual_rows), h(md), h(cs), cols)[1]


def expect(lines):
    return ("\n".join(lines) + "\n").encode() if lines else b""


def check_unpaired(targets=None, ref_start=0, kept_only=True, unmapped=True, md=True, cs=True, qual=True, mapping=None):
    m = mapping or U.mapping()
    toff, text = U.csr(U.CIGARS)
    seq_rows, qual_rows = U.texts()
    dm, dc = (U.diffs("M") if md else None), (U.diffs("c") if cs else None)
    ref = dict(ref_name="chr", ref_len=5000) if targets is None else {}
    want, skipped, n_un = kh.sam_lines(m, toff, text, seq_rows, U.NAMES, qual_rows=qual_rows if qual else None, md=dm, cs=dc, ref_start=ref_start, targets=targets,
                                       kept_only=kept_only, unmapped=unmapped, header=False, **ref)
    L = kh.sam_line_columns(NP, m, targets, ref_start, kept_only, unmapped, md, cs, None, [d.ok for d in (dm, dc) if d is not None])
    got = model_text(m, L, U.NAMES, ["chr"] if targets is None else targets.names, (toff, text), seq_rows, qual_rows if qual else None,
                     None if dm is None else (dm.offsets, dm.text), None if dc is None else (dc.offsets, dc.text))
    assert got == expect(want)
    assert (L.lines, L.skipped, L.unmapped_reads) == (len(want) - (n_un if unmapped else 0), skipped, n_un)
    # the SEQ rows the lines print are the ones the columns ask oriented_rows for
    assert set(int(r) for r in L.seq if r >= 0) == set(np.flatnonzero(L.need)) | set(len(L.need) + np.flatnonzero(L.show))
    return L


def test_unpaired_lines_of_the_hand_made_mapping():
    L = check_unpaired()      # read 2 has no rows; the best row of read 3 is not valid; read 4's only row is not kept
    assert (L.lines, L.skipped, L.unmapped_reads) == (5, 2, 3)
    assert [dt for dt in (getattr(L, k).dtype for k in sam.LINE_COLUMNS)] == [np.dtype(d) for d in sam.LINE_DTYPES]


@pytest.mark.parametrize("kw", [dict(kept_only=False), dict(unmapped=False), dict(md=False), dict(cs=False), dict(md=False, cs=False, qual=False), dict(ref_start=30),
                                dict(kept_only=False, unmapped=False)], ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_unpaired_options(kw):
    check_unpaired(**kw)


def test_targets_and_a_row_that_straddles_a_spacer():
    T = kh.Targets(["a", "b"], [1000, 2000], spacer=64)      # b covers [1064, 3064)
    check_unpaired(targets=T)
    m = U.mapping()
    rs = m.records.rs.copy()
    rs[0] = 995                                              # row 0, the best of read 0, now runs from a into the spacer: not printable
    L = check_unpaired(targets=T, mapping=m._replace(records=m.records._replace(rs=rs, re=rs + 10)))
    assert (L.lines, L.unmapped_reads) == (3, 4)
    with pytest.raises(ValueError, match="ref_start must be 0"):
        kh.sam_line_columns(NP, U.mapping(), T, 5)


def test_refusals_of_the_glue():
    bad = U.diffs("M")
    bad.ok[1] = 0
    with pytest.raises(ValueError, match="row 1 does not walk the two texts.*ref_order=True"):
        kh.sam_line_columns(NP, U.mapping(), diff_ok=[U.diffs("c").ok, bad.ok])
    bad.ok[1], bad.ok[5] = 1, 0                              # row 5 is not printed: nobody asks whether it walks
    kh.sam_line_columns(NP, U.mapping(), diff_ok=[bad.ok])
    m = U.mapping()
    with pytest.raises(ValueError, match="names read 4, the Mapping holds 4 reads"):
        kh.sam_line_columns(NP, m._replace(select=m.select._replace(best=m.select.best[:4])))
    with pytest.raises(ValueError, match="ref_start lies beyond"):
        kh.sam_line_columns(NP, m, ref_start=150)


def pair_select(row, mapq=(60, 60, 60, 0, 0, 0), tlen=(400, -400, 0, 0, 0, 0), flag=(7, 0, 0)):
    return kh.PairSelect(np.array(row, dtype=np.int32), np.array(mapq, dtype=np.uint8), np.array(tlen, dtype=np.int32), np.array(flag, dtype=np.uint8), None, None)


PAIR_CASES = {
    "as_written": (P.PAIRS, None),                                                   # read 0's representative (row 1) is not select.best (row 0); read 3 unmapped beside read 2; pair 2 without rows
    "best_rows": (pair_select([0, 2, 4, -1, -1, -1]), None),
    "a_row_of_another_read": (pair_select([2, 2, 3, -1, -1, -1]), None),             # pairs.row[0] names a row of read 1: read 0 is unmapped
    "nobody": (pair_select([-1] * 6, flag=(0, 0, 0)), None),
    "targets": (P.PAIRS, kh.Targets(["a", "b"], [5300, 14000], spacer=64)),          # a = [0, 5300), b = [5364, 19364): the representatives of pair 0 lie on a (row 1) and on b (row 2)
    "different_targets": (pair_select([0, 2, 3, -1, -1, -1], flag=(2, 0, 0), tlen=(0, 0, 0, 0, 0, 0)), kh.Targets(["a", "b"], [5300, 14000], spacer=64)),
}


@pytest.mark.parametrize("case", sorted(PAIR_CASES))
@pytest.mark.parametrize("kw", [dict(), dict(unmapped=False), dict(kept_only=False)], ids=["default", "unmapped=False", "kept_only=False"])
def test_paired_lines(case, kw):
    pairs, targets = PAIR_CASES[case]
    m = P.mapping()
    toff, text = P.csr([r[11] for r in P.ROWS])
    seq_rows = P.csr([r[12] for r in P.ROWS] + P.READS)
    names = ["r%d" % i for i in range(P.N_READS)]
    ref = dict(ref_name="ref", ref_len=20000) if targets is None else dict(targets=targets)
    want, skipped, n_un = kh.sam_lines(m, toff, text, seq_rows, names, header=False, pairs=pairs, **ref, **kw)
    L = kh.sam_line_columns(NP, m, targets, 0, kw.get("kept_only", True), kw.get("unmapped", True), False, False, pairs)
    got = model_text(m, L, names, ["ref"] if targets is None else targets.names, (toff, text), seq_rows, None, None, None)
    assert got == expect(want)
    assert (L.lines, L.skipped, L.unmapped_reads) == (len(want) - (n_un if kw.get("unmapped", True) else 0), skipped, n_un)
    if case == "different_targets" and not kw:
        f = {x[0]: x for x in reversed([l.split("\t") for l in want])}      # the first line of every read
        assert (f["r0"][2], f["r0"][6], f["r1"][2], f["r1"][6]) == ("a", "b", "b", "a")
    if case == "as_written" and not kw:
        assert want == [e.replace(" ", "\t") for e in P.EXPECT]


def test_pairs_must_fit_the_mapping():
    with pytest.raises(ValueError, match="reads must come in pairs"):
        kh.sam_line_columns(NP, P.mapping(), pairs=pair_select([0, 2, 3, -1, -1], mapq=(0,) * 5, tlen=(0,) * 5))


def test_names_csr():
    offs, text = kh.names_csr(["r0", "", "read/1"])
    assert offs.dtype == np.uint64 and offs.tolist() == [0, 2, 2, 8] and text.dtype == np.uint8 and bytes(text) == b"r0read/1"
    offs, text = kh.names_csr([])
    assert offs.tolist() == [0] and len(text) == 0
    with pytest.raises(UnicodeEncodeError):
        kh.names_csr(["réad"])


def test_the_torch_namespace_gives_the_same_columns():
    torch = pytest.importorskip("torch")
    from test_array_namespace import same, tensor
    TT = _xp.Torch(torch.device("cpu"))
    tt = lambda nt: type(nt)(*(None if x is None else tensor(x) for x in nt))      # noqa: E731
    T = kh.Targets(["a", "b"], [5300, 14000], spacer=64)
    for m, pairs, targets in ((U.mapping(), None, None), (U.mapping(), None, kh.Targets(["a", "b"], [1000, 2000], spacer=64)), (P.mapping(), P.PAIRS, None),
                              (P.mapping(), PAIR_CASES["different_targets"][0], T)):
        mt = kh.Mapping(tt(m.table), None, None, None, tt(m.select), tt(m.records))
        for kw in (dict(), dict(unmapped=False, kept_only=False)):
            a = kh.sam_line_columns(NP, m, targets, pairs=pairs, **kw)
            b = kh.sam_line_columns(TT, mt, targets, pairs=None if pairs is None else tt(pairs), **kw)
            for k, dt in zip(sam.LINE_COLUMNS, sam.LINE_DTYPES):
                same(getattr(a, k), getattr(b, k), dt)
            same(a.need, b.need)
            same(a.show, b.show)
            assert (a.lines, a.skipped, a.unmapped_reads) == (b.lines, b.skipped, b.unmapped_reads)
    # checks of the caller ride along in the one read and come first
    for xp, one, m in ((NP, lambda v: np.int64(v), U.mapping()), (TT, lambda v: torch.tensor(v), kh.Mapping(tt(U.mapping().table), None, None, None, tt(U.mapping().select), tt(U.mapping().records)))):
        kh.sam_line_columns(xp, m, refuse=[(one(0), "never")])
        with pytest.raises(ValueError, match="the layout is wrong"):
            kh.sam_line_columns(xp, m, ref_start=150, refuse=[(one(0), "never"), (one(3), "the layout is wrong")])
