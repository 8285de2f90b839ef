"""The mapper's glue steps (kmerhash_amd/mapper.py) on the host, numpy against torch-on-CPU: every step is written once over an array
namespace, so the statement a device Mapping runs is run here on CPU tensors (the namespace is passed explicitly: picking it from a
column would send a CPU tensor through numpy) and must give the values and the documented dtypes of the numpy one.  The Mapping is the
hand-made one of test_capi_rescue.py::test_python_refusals_and_requests_need_no_device -- five pairs of 100-base reads, four rows --
alone and extended by a row whose re is exactly 2^31 (the sign bit of an int32), a row on no target and a row of a read beyond
n_reads; and an empty table.  Then the read layout: every refusal that can be reached without a device, and the default ends.
No GPU, no library call."""
import io

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _xp, mapper as M  # noqa: E402
from test_array_namespace import same, tensor  # noqa: E402

NP, TT = _xp.NUMPY, _xp.Torch(torch.device("cpu"))
z = lambda v, dt: np.array(v, dtype=dt)      # noqa: E731
STARTS = np.arange(10, dtype=np.int64) * 100
TOP = 2 ** 31


def targets(big):
    """a = [0, 5300) and b = [5364, 19364) as in test_capi_rescue; big: c = [19428, 2^31 - 50) behind them"""
    return kh.Targets(["a", "b", "c"], [5300, 14000, TOP - 50 - 19428], spacer=64) if big else kh.Targets(["a", "b"], [5300, 14000], spacer=64)


def make(kind):
    """-> (Mapping, PairSelect) of numpy columns.  base: rows 0..3 of reads 0, 3, 5, 6.  ext: also row 4 of read 8 at [2^31 - 100, 2^31),
    row 5 of read 9 inside the spacer behind target a and not kept, row 6 of read 12 (beyond the ten reads) and not valid"""
    n = {"empty": 0, "base": 4, "ext": 7}[kind]
    seg, rev = z([0, 3, 5, 6, 8, 9, 12][:n], np.uint32), z([0, 1, 0, 0, 0, 1, 0][:n], np.uint8)
    rs, re_ = z([5000, 9000, 300, 19950, TOP - 100, 5320, 40][:n], np.uint32), z([5100, 9100, 400, 20000, TOP, 5350, 140][:n], np.uint32)
    table = M.ChainTable(seg, rev, None, None, None, None, None, z([50, 60, 70, 80, 90, 55, 65][:n], np.int32), None, None)
    select = M.ChainSelect(None, None, z([60, 0, 30, 60, 7, 1, 2][:n], np.uint8), z([3, 3, 3, 3, 3, 1, 3][:n], np.uint8), None, None, None)
    rec = M.ChainRecords(z([1, 1, 1, 1, 1, 1, 0][:n], np.uint8), None, None, rs, re_, None, None, None, None, None, None)
    row = z([0, -1, -1, 1, -1, 2, 3, -1, 4 if n > 4 else -1, -1], np.int32)      # pair 4: nobody has a row (base), read 8 has one (ext)
    if n == 0:
        row[:] = -1
    return M.Mapping(table, None, None, None, select, rec), M.PairSelect(row, None, None, None, None, None)


def as_tensors(nt):
    """a namedtuple of numpy columns (nested ones too) as CPU tensors holding the same bits"""
    return type(nt)(*(None if x is None else as_tensors(x) if isinstance(x, tuple) else tensor(x) for x in nt))


def same_all(a, t, dtypes):
    assert len(a) == len(t) == len(dtypes)
    for x, y, dt in zip(a, t, dtypes):
        same(x, y, dt)


@pytest.mark.parametrize("q", [[0, 5, 99, 100, 100, 250, 999], [], [950]])
def test_segments_of_reads(q):
    q = z(q, np.uint32)
    lay = M.ReadLayout(STARTS, None, None)
    a, t = M.read_segments(NP, q, lay), M.read_segments(TT, tensor(q), lay)
    same(a, t, np.uint64)
    assert len(a) == 11 and a[0] == 0 and a[-1] == len(q) and (len(q) != 7 or a.tolist() == [0, 3, 5, 6, 6, 6, 6, 6, 6, 6, 7])
    assert M.read_segments(NP, q, M.ReadLayout(None, None, None)) is None and M.read_segments(TT, tensor(q), M.ReadLayout(None, None, None)) is None


@pytest.mark.parametrize("how", ["one read", "reads", "groups"])
@pytest.mark.parametrize("n_chains", [3, 0])
def test_chain_table_rows(how, n_chains):
    k = 15
    q, v = z([0, 5, 99, 100, 180, 250, 280], np.uint32), z([0, 0, 0, 1, 1, 0, 0], np.uint8)
    r = z([1000, 1010, 1100, 7000, 6900, TOP - 50, TOP - 16], np.uint32)      # r_end reaches 2^31 - 1; a reverse chain descends
    c = M.Chains(None, None, None, z([0, 3, 5][:n_chains], np.uint32), z([2, 4, 6][:n_chains], np.uint32), z([3, 2, 2][:n_chains], np.uint32), z([45, 30, 31][:n_chains], np.int32))
    seg = groups = None
    if how == "reads":
        seg = M.read_segments(NP, q, M.ReadLayout(STARTS, None, None))
    if how == "groups":      # (read, target) groups: anchors [0, 3) of read 0, [3, 5) of read 1, [5, 6) and [6, 7) of read 2 on two targets
        groups = M.AnchorGroups(q, r, v, None, None, z([0, 3, 5, 6, 7], np.uint64), z([0, 1, 2, 2], np.uint32), None)
        seg = groups.offsets
    a = M.chain_rows(NP, q, r, v, c, k, seg, groups)
    t = M.chain_rows(TT, tensor(q), tensor(r), tensor(v), as_tensors(c), k, None if seg is None else tensor(seg), None if groups is None else as_tensors(groups))
    same_all(a, t, [np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.int32])
    if n_chains:
        assert a[0].tolist() == {"one read": [0, 0, 0], "reads": [0, 1, 2], "groups": [0, 1, 2]}[how] and a[1].tolist() == [0, 1, 0]
        assert (a[2].tolist(), a[3].tolist(), a[4].tolist(), a[5].tolist()) == ([0, 100, 250], [114, 195, 295], [1000, 6900, TOP - 50], [1115, 7015, TOP - 1])


@pytest.mark.parametrize("kind", ["base", "ext", "empty"])
def test_read_intervals_and_the_offsets_csr(kind):
    mp, _ = make(kind)
    seg = mp.table.seg
    lay = M.ReadLayout(np.arange(13) * 100, np.arange(13) * 100 + 96, 1300)
    a, t = M.chain_read_intervals(NP, lay, seg), M.chain_read_intervals(TT, lay, tensor(seg))
    same_all(a, t, [np.uint32, np.uint32])
    assert a[0].tolist() == (seg.astype(np.int64) * 100).tolist() and a[1].tolist() == (seg.astype(np.int64) * 100 + 96).tolist()
    for n_reads in (10, 13, 14):
        a, t = M.seg_offsets(NP, seg, n_reads, checked=False), M.seg_offsets(TT, tensor(seg), n_reads, checked=False)
        same(a, t, np.uint64)
        assert len(a) == n_reads + 1 and all(a[g] == int((seg < g).sum()) for g in range(n_reads + 1))
        covers = not len(seg) or int(seg.max()) < n_reads
        for xp, s in ((NP, seg), (TT, tensor(seg))):
            if covers:
                M.seg_offsets(xp, s, n_reads, checked=True)
            else:
                with pytest.raises(ValueError, match="does not cover the reads of the table"):
                    M.seg_offsets(xp, s, n_reads, checked=True)


@pytest.mark.parametrize("with_targets", [False, True])
@pytest.mark.parametrize("kind", ["base", "ext", "empty"])
def test_printable_rows_and_pair_candidates(kind, with_targets):
    mp, _ = make(kind)
    T = targets(kind == "ext") if with_targets else None
    n = len(mp.table.seg)
    for kept_only in (True, False):
        a, t = M.printable(NP, mp, T, kept_only), M.printable(TT, as_tensors(mp), T, kept_only)
        assert a[0].dtype == a[1].dtype == bool and t[0].dtype == t[1].dtype == torch.bool
        assert a[0].tolist() == t[0].tolist() and a[1].tolist() == t[1].tolist() and (a[2] is None) == (t[2] is None) == (T is None)
        # by hand: row 3 lies behind b -- on no target, or inside c where there is one --, row 4 ends 50 bases beyond c (its re has the sign
        # bit), row 5 lies in a spacer and is not kept, row 6 is invalid
        want = [True, True, True, not with_targets or kind == "ext", not with_targets, not with_targets and not kept_only, False][:n]
        assert a[0].tolist() == want and a[1].tolist() == ([True] * n if not kept_only else [True, True, True, True, True, False, True][:n])
        if T is not None:
            same(a[2], t[2], np.int64)
            assert a[2].tolist() == [0, 1, 0, 2 if kind == "ext" else -1, 2, -1, 0][:n]
    a, t = M.pair_candidates(NP, mp, 14, T), M.pair_candidates(TT, as_tensors(mp), 14, T)
    same(a[0], t[0], np.uint64)
    same(a[1], t[1], np.uint8)
    assert (a[2] is None) == (t[2] is None) == (T is None)
    if T is not None:
        same(a[2], t[2], np.uint32)
        assert a[2].tolist() == [0, 1, 0, 2 if kind == "ext" else 0xFFFFFFFF, 2, 0xFFFFFFFF, 0][:n]
    assert a[1].tolist() == M.printable(NP, mp, T)[0].astype(int).tolist() and a[0][-1] == n
    if kind == "ext":      # ten reads do not cover read 12: the host Mapping is refused, the tensor Mapping leaves the row outside the CSR (no wait)
        with pytest.raises(ValueError, match="does not cover the reads of the table"):
            M.pair_candidates(NP, mp, 10, T)
        assert M.pair_candidates(TT, as_tensors(mp), 10, T)[0].tolist() == [0, 1, 1, 1, 2, 2, 3, 4, 4, 5, 6]


@pytest.mark.parametrize("with_targets", [False, True])
@pytest.mark.parametrize("kind", ["base", "ext", "empty"])
def test_rescue_windows(kind, with_targets):
    mp, pairs = make(kind)
    big = kind == "ext"
    where = dict(targets=targets(big)) if with_targets else dict(ref_len=TOP if big else 20000)
    lay = M.ReadLayout(STARTS, STARTS + 100, None)
    a = M.rescue_windows(NP, mp, pairs, lay, 200, 600, 31, **where)
    t = M.rescue_windows(TT, as_tensors(mp), as_tensors(pairs), lay, 200, 600, 31, **where)
    same_all(a, t, [np.uint32] * 4 + [np.uint8, np.uint32])
    for lay_t in (M.ReadLayout(tensor(STARTS), tensor(STARTS + 100), None), M.ReadLayout(STARTS.tolist(), (STARTS + 100).tolist(), None)):
        same_all(a, M.rescue_windows(TT, as_tensors(mp), as_tensors(pairs), lay_t, 200, 600, 31, **where), [np.uint32] * 4 + [np.uint8, np.uint32])
    if kind == "empty":
        assert all(len(x) == 0 for x in a)
        return
    # the numbers of test_capi_rescue.py: reads 1, 2, 4 and 7 ask; with targets a and b alone read 7's partner lies on none.  Read 7's partner
    # stands forward at [19950, 20000) -> [20019, 20550), clamped to the 20000 bases of the base text
    n = 3 if with_targets and not big else 4
    assert a.read.tolist()[:n] == [1, 2, 4, 7][:n] and a.q_lo.tolist()[:n] == [100, 200, 400, 700][:n] and a.q_hi.tolist()[:n] == [200, 300, 500, 800][:n]
    assert a.rev.tolist()[:n] == [1, 0, 1, 1][:n] and a.w_lo.tolist()[:n] == [5069, 8500, 369, 20019 if big else 20000][:n]
    assert a.w_hi.tolist()[:n] == ([5300, 9031, 900, 20550][:n] if with_targets else [5600, 9031, 900, 20550 if big else 20000])
    if not big:
        assert len(a.read) == n
        return
    # read 9: its partner stands forward at [2^31 - 100, 2^31) -> [2^31 - 31, 2^31 + 500), clamped to the text's end or to target c's
    assert a.read.tolist()[n:] == [9] and a.rev.tolist()[n:] == [1]
    assert (a.w_lo.tolist()[n:], a.w_hi.tolist()[n:]) == (([TOP - 50], [TOP - 50]) if with_targets else ([TOP - 31], [TOP]))


def test_the_public_calls_pick_numpy_for_cpu_tensors():
    mp, pairs = make("base")
    rq = kh.rescue_requests(as_tensors(mp), as_tensors(pairs), tensor(STARTS), tensor(STARTS + 100), min_ins=200, max_ins=600, ref_len=20000)
    assert all(isinstance(x, np.ndarray) for x in rq) and rq.w_lo.tolist() == [5069, 8500, 369, 20000] and rq.w_hi.tolist() == [5600, 9031, 900, 20000]
    assert [x.dtype for x in rq] == [np.uint32] * 4 + [np.uint8, np.uint32]


def test_read_layout_defaults_and_placing():
    lay = M.ReadLayout([0, 100, 250], None, 400)
    assert lay.n_reads == 3 and [x.tolist() for x in lay.host] == [[0, 100, 250], [100, 250, 400]] and all(x.dtype == np.int64 for x in lay.host)
    one = M.ReadLayout(None, None, 77)
    assert one.n_reads == 1 and [x.tolist() for x in one.host] == [[0], [77]]
    given = M.ReadLayout(tensor(z([0, 100], np.int64)), tensor(z([90, 190], np.int32)), 200)
    assert [x.tolist() for x in given.host] == [[0, 100], [90, 190]] and M.ReadLayout.of(b"ACGT", given) is given
    assert M.ReadLayout.of(b"ACGTAC", [0, 2]).host[1].tolist() == [2, 6]
    for lay_ in (lay, one, given):
        for xp, kind in ((NP, np.ndarray), (TT, torch.Tensor)):
            s, e = lay_.on(xp)
            assert isinstance(s, kind) and isinstance(e, kind) and s.tolist() == lay_.host[0].tolist() and e.tolist() == lay_.host[1].tolist()
            assert (s.dtype, e.dtype) == ((np.int64, np.int64) if xp is NP else (torch.int64, torch.int64))
    lay.ascending(), lay.bounded(False), lay.bounded(True), one.bounded(True), given.bounded(False), given.bounded(True)


def test_read_layout_refusals_of_every_entry_point():
    # the chaining calls (chains ... map_pairs_rescued, anchor_groups) check the starts where they make the segments
    for bad in ([], [5, 10], [0, 200, 100]):
        with pytest.raises(ValueError, match="read_starts must be ascending byte offsets of the reads in seq, the first one 0"):
            M.read_segments(NP, z([0, 7], np.uint32), M.ReadLayout(bad, None, None))
    # chain_ends and what is built on it check read_ends that are given: one per read, start <= end <= len(seq); starts below 0 are not theirs to refuse
    for ends in ([90], [90, 190, 200], [90, 99], [90, 201]):
        with pytest.raises(ValueError, match=r"^read_ends must hold one byte offset per read, read_starts\[s\] <= read_ends\[s\] <= len\(seq\)$"):
            M.ReadLayout([0, 100], ends, 200).bounded(False)
    M.ReadLayout([-5, 100], [90, 190], 200).bounded(False)
    M.ReadLayout([0, 300], None, 200).bounded(False)          # the default ends are not checked there
    # the SAM writers check the default ends and the starts too, before anything else
    mp, pairs = make("base")
    seq, names = b"A" * 1000, ["r%d" % i for i in range(10)]
    sam_msg = "read_starts and read_ends must hold one byte offset per read, 0 <= read_starts"
    for rs, re_ in (([-5, 100], [90, 190]), ([0, 100], [90]), ([0, 100], [90, 1001]), ([0, 100], [90, 99]), ([0, 1200], None)):      # (the last: default ends 1200, 1000)
        for call in (lambda **kw: kh.write_sam(io.StringIO(), mp, seq, seq, names, **kw), lambda **kw: kh.write_sam_pairs(io.StringIO(), mp, pairs, seq, seq, names, **kw),
                     lambda **kw: kh.write_sam_rescued(io.StringIO(), mp, pairs, "unused", seq, seq, names, **kw)):
            with pytest.raises(ValueError, match=sam_msg):
                call(read_starts=rs, read_ends=re_, ref_name="ref", ref_len=1000)
    with pytest.raises(TypeError):
        kh.write_sam(io.StringIO(), mp, seq, seq, names, None, ref_name="ref", ref_len=1000)
    # rescue_requests: one entry per read of pairs, both columns given; an even number of reads
    with pytest.raises(ValueError, match="one entry per read"):
        kh.rescue_requests(mp, pairs, STARTS[:8], STARTS[:8] + 100, ref_len=20000)
    with pytest.raises(ValueError, match="one entry per read"):
        kh.rescue_requests(mp, pairs, STARTS, STARTS[:8] + 100, ref_len=20000)
    with pytest.raises(ValueError, match="ref_len"):
        kh.rescue_requests(mp, pairs, STARTS, STARTS + 100)
    with pytest.raises(TypeError):
        kh.rescue_requests(mp, pairs, STARTS, None, ref_len=20000)
    with pytest.raises(ValueError, match="even number of reads"):
        kh.rescue_requests(mp, pairs._replace(row=pairs.row[:9]), STARTS[:9], STARTS[:9] + 100, ref_len=20000)
    with pytest.raises(ValueError, match="even number of reads"):
        kh.pair_mapping(mp, 9)
    with pytest.raises(ValueError, match="does not cover the reads of the table"):
        kh.pair_mapping(mp, 6)
    with pytest.raises(ValueError, match="n_reads"):
        kh.select_table(mp.table, 6)
    # every pipeline method of an index that is not stranded refuses first, by its own name (map_pairs_rescued: by map_pairs')
    ix = kh.KmerPositionIndex.__new__(kh.KmerPositionIndex)
    ix.stranded = False
    for meth, args in (("anchors", ()), ("chains", ()), ("chain_select", ()), ("chain_edits", (b"ACGT",)), ("chain_cigars", (b"ACGT",)), ("chain_ends", (b"ACGT",)),
                       ("map", (b"ACGT",)), ("map_pairs", (b"ACGT", [0, 2])), ("map_pairs_rescued", (b"ACGT", [0, 2]))):
        with pytest.raises(ValueError, match=r"%s\(\) needs an index made with stranded=True" % ("map_pairs" if meth == "map_pairs_rescued" else meth)):
            getattr(ix, meth)(b"ACGT", *args)
    with pytest.raises(ValueError, match=r"anchor_groups\(\) needs an index made with stranded=True"):
        ix.anchor_groups(b"ACGT", targets=targets(False))
    ix.stranded = True
    with pytest.raises(ValueError, match="even number of reads"):
        ix.map_pairs(b"ACGT", b"ACGT", [0, 1, 2])
    with pytest.raises(ValueError, match="even number of reads"):
        ix.map_pairs_rescued(b"ACGT", b"ACGT", None)
