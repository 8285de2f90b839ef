"""GPU: write_sam_bytes, the SAM file assembled on the device, against write_sam byte for byte, and the triples they return: the planted
reads of tests/test_gpu_records_index.py mapped by ix.map(ref_order=True) on both index classes, with and without Targets, on numpy
arrays and on CUDA tensors; md / cs / both / neither, with and without qual, kept_only=False, unmapped=False, header=False.  The same
with pairs= against write_sam_pairs on the planted pairs of tests/test_gpu_pair_index.py.  A Mapping made with ref_order=False, and a
reference text cut short, end as they end in write_sam: the same triple or the same ValueError, word for word (on the planted reads
write_sam itself accepts the ref_order=False Mapping -- its reverse-strand rows still consume both texts end to end -- and refuses the
short text).  read_names as a ready CSR gives the same file."""
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from stream_checks import to_dev  # noqa: E402
from test_gpu_pair_index import GAP, MATE, N_PAIRS, make_pairs  # noqa: E402
from test_gpu_records_index import N_READS, REF_LEN, make_reads  # noqa: E402

CUT = 9000      # with targets the reference is two contigs: [0, CUT) and [CUT, REF_LEN)
OPTIONS = [dict(md=True, cs=False), dict(md=False, cs=True), dict(md=True, cs=True), dict(md=False, cs=False), dict(qual=None), dict(kept_only=False),
           dict(unmapped=False), dict(header=False), dict(kept_only=False, unmapped=False, cs=True, qual=None)]


def both_files(mp, args, kw, pairs=None):
    """-> the file of the host writer, encoded, and its triple; the file of write_sam_bytes and its triple"""
    fh, bh = io.StringIO(), io.BytesIO()
    want = kh.write_sam(fh, mp, *args, **kw) if pairs is None else kh.write_sam_pairs(fh, mp, pairs, *args, **kw)
    got = kh.write_sam_bytes(bh, mp, *args, pairs=pairs, **kw)
    return fh.getvalue().encode(), tuple(want), bh.getvalue(), tuple(got)


def outcome(write, fh):
    """how a writer ends: the triple and the bytes of the file, or the text of its ValueError"""
    try:
        triple = tuple(write(fh))
        return "returned", triple, fh.getvalue() if isinstance(fh, io.BytesIO) else fh.getvalue().encode()
    except ValueError as e:
        return "ValueError", str(e)


@pytest.mark.parametrize("dev", [False, True], ids=["numpy", "tensors"])
@pytest.mark.parametrize("with_targets", [False, True], ids=["one_ref", "targets"])
@pytest.mark.parametrize("cls,k", [("KmerPositionIndex", 15), ("WideKmerPositionIndex", 35)])
def test_the_file_of_the_device_equals_the_file_of_the_host(cls, k, with_targets, dev):
    ref, seq, starts, ends_at = make_reads()
    T = kh.Targets.from_sequences(["ctgA", "ctgB"], [ref[:CUT], ref[CUT:]]) if with_targets else None
    mk = to_dev if dev else (lambda a: a)
    rt = mk(T.text.copy() if with_targets else np.frombuffer(ref, dtype=np.uint8).copy())
    qt = mk(np.frombuffer(seq, dtype=np.uint8).copy())
    qual = mk((33 + np.arange(len(seq)) % 41).astype(np.uint8))
    names = ["read%d" % i for i in range(N_READS)]
    where = dict(targets=T) if with_targets else dict(ref_name="ref", ref_len=REF_LEN)
    ix = getattr(kh, cls)(k=k, stranded=True, **({"s": 25} if cls == "WideKmerPositionIndex" else {}))
    try:
        ix.build_sequences(rt)
        mp = ix.map(qt, rt, read_starts=starts, read_ends=ends_at, min_score=20, min_count=2, pri_pct=50, targets=T, ref_order=True)
        plain = ix.map(qt, rt, read_starts=starts, read_ends=ends_at, min_score=20, min_count=2, pri_pct=50, targets=T, ref_order=False)
    finally:
        ix.close()
    args = (qt, rt, names, starts, ends_at)
    seen = set()
    for opt in OPTIONS:
        kw = dict(qual=qual, **where)
        kw.update(opt)
        want, t_want, got, t_got = both_files(mp, args, kw)
        assert got == want, opt
        assert t_got == t_want, opt
        seen |= {int(l.split(b"\t")[1]) for l in want.splitlines() if not l.startswith(b"@")}
    assert 0 in seen and all(any(f & bit for f in seen) for bit in (0x10, 0x100, 0x4)), seen      # forward, reverse, secondary and unmapped lines were compared
    st = kh.sam_text(mp, *args, qual=qual, **where)
    assert (st.text.is_cuda and st.offsets.is_cuda) if dev else (isinstance(st.text, np.ndarray) and st.text.dtype == np.uint8 and st.offsets.dtype == np.uint64)
    assert st.header == kh.sam_header(**where).encode() and len(st.offsets) == st.lines + (st.unmapped_reads) + 1
    # names as a ready CSR, living where the Mapping lives
    bh = io.BytesIO()
    kh.write_sam_bytes(bh, mp, qt, rt, tuple(mk(a) for a in kh.names_csr(names)), starts, ends_at, qual=qual, **where)
    fh = io.StringIO()
    kh.write_sam(fh, mp, *args, qual=qual, **where)
    assert bh.getvalue() == fh.getvalue().encode()
    if dev:      # the read layout as CUDA tensors: the same file, and its bounds check comes back with the glue's one read
        ds, de = to_dev(starts), to_dev(ends_at)
        bh = io.BytesIO()
        kh.write_sam_bytes(bh, mp, qt, rt, names, ds, de, qual=qual, **where)
        assert bh.getvalue() == fh.getvalue().encode()
        with pytest.raises(ValueError, match="read_starts and read_ends must hold one byte offset per read"):
            kh.write_sam_bytes(io.BytesIO(), mp, qt, rt, names, ds, de + len(seq), **where)
    # a row that does not walk the texts: the ValueError of write_sam, word for word.  kh_record_diffs calls a row ok when its runs consume
    # the read and the reference bases under it from end to end, and the runs of a reverse-strand row in read order consume as many as
    # in reference order: a Mapping made with ref_order=False is NOT refused by write_sam, whatever the reads (its strings are those
    # of the wrong order).  So the device writer must end as write_sam ends there, with the same triple and the same bytes; the
    # ValueError itself is pinned on a reference text cut short, which both refuse
    for m, text in ((plain, rt), (mp, rt[:100])):
        host = outcome(lambda fh: kh.write_sam(fh, m, qt, text, names, starts, ends_at, **where), io.StringIO())
        device = outcome(lambda fh: kh.write_sam_bytes(fh, m, qt, text, names, starts, ends_at, **where), io.BytesIO())
        assert device == host
        assert host[0] == ("returned" if m is plain else "ValueError")
    assert host[0] == "ValueError" and "ref_order=True" in host[1]


@pytest.mark.parametrize("with_targets", [False, True], ids=["one_ref", "targets"])
@pytest.mark.parametrize("cls,k", [("KmerPositionIndex", 15), ("WideKmerPositionIndex", 33)])
def test_paired_files(cls, k, with_targets):
    A, B, seq, plan = make_pairs()
    T = kh.Targets.from_sequences(["ctgA", "ctgB"], [A, B])
    dev = (cls == "WideKmerPositionIndex") != with_targets      # tensors in two of the four runs, numpy in the others
    mk = to_dev if dev else (lambda x: x)
    rt, qt = mk(T.text.copy()), mk(np.frombuffer(seq, dtype=np.uint8).copy())
    qual = mk((33 + np.arange(len(seq)) % 41).astype(np.uint8))
    n_reads = 2 * N_PAIRS
    starts = np.arange(n_reads, dtype=np.int64) * (MATE + GAP)
    ends_at = starts + MATE
    names = ["frag%d" % (s // 2) for s in range(n_reads)]
    where = dict(targets=T) if with_targets else dict(ref_name="ref", ref_len=len(T.text))
    ix = getattr(kh, cls)(k=k, stranded=True, **({"s": 25} if cls == "WideKmerPositionIndex" else {}))
    try:
        ix.build_sequences(rt)
        mp, pr = ix.map_pairs(qt, rt, starts, ends_at, min_score=20, min_count=2, targets=T if with_targets else None)
    finally:
        ix.close()
    args = (qt, rt, names, starts, ends_at)
    flags = set()
    for opt in (dict(), dict(md=False, cs=True, qual=None), dict(kept_only=False), dict(unmapped=False, header=False)):
        kw = dict(qual=qual, **where)
        kw.update(opt)
        want, t_want, got, t_got = both_files(mp, args, kw, pairs=pr)
        assert got == want, opt
        assert t_got == t_want, opt
        flags |= {int(l.split(b"\t")[1]) for l in want.splitlines() if not l.startswith(b"@")}
    assert any(f & 0x2 for f in flags) and any(f & 0x8 for f in flags) and any(f & 0x4 for f in flags) and any(f & 0x20 for f in flags), sorted(flags)
