"""CPU: kh_fastq_records and kh_pack_rows are declared after kh_sam_lines and before kh_release_cached_memory, bound with matching
argtypes and exported; every refusal the header lists comes back as KH_ERR_INVALID before a device is touched (this test runs without
one) and leaves the outputs alone; an empty host text is KH_OK without a device; the Python surface exists with its signatures."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC_ORDER = ["text", "n", "flags", "where", "name_lo", "name_hi", "seq_lo", "seq_hi", "qual_lo", "status", "cap", "n_records", "n_bad", "tail_lines", "device", "hip_stream"]
PACK_ORDER = ["text", "n", "lo", "hi", "dst", "n_rows", "sep", "where", "out", "out_n", "device", "hip_stream"]
COLS = ["name_lo", "name_hi", "seq_lo", "seq_hi", "qual_lo"]


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def test_symbols_declared_bound_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, order in (("kh_fastq_records", REC_ORDER), ("kh_pack_rows", PACK_ORDER)):
        m = re.search(r"kh_status\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, "%s is not declared" % name
        assert [re.sub(r"\s+", " ", p).strip().split(" ")[-1].lstrip("*") for p in m.group(1).split(",")] == order
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    assert txt.index("kh_sam_lines") < txt.index("kh_fastq_records") < txt.index("kh_pack_rows") < txt.index("kh_release_cached_memory")
    for name, value in (("KH_FASTQ_STRIP_MATE", "1u"), ("KH_FASTQ_NO_AT", "1u"), ("KH_FASTQ_NO_PLUS", "2u"), ("KH_FASTQ_LENGTHS", "4u"), ("KH_FASTQ_NO_NAME", "8u")):
        assert re.search(r"#define\s+%s\s+%s" % (name, value), txt), name
    for phrase in ("the number of '\\n' (10) before it", "One '\\r' (13) directly before the end of a line", "NON-EMPTY lines", "is KEPT", "the name \"/1\" itself stays",
                   "behind EVERY row", "Every store is clamped to out_n", "the call does not wait"):
        assert phrase in raw, phrase
    vp, u64, u32, i32, pu64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)
    f = capi.lib().kh_fastq_records
    assert list(f.argtypes) == [vp, u64, u32, i32, vp, vp, vp, vp, vp, vp, u64, pu64, pu64, C.POINTER(u32), i32, vp] and f.restype is C.c_int
    g = capi.lib().kh_pack_rows
    assert list(g.argtypes) == [vp, u64, vp, vp, vp, u64, i32, i32, vp, u64, i32, vp] and g.restype is C.c_int


def ptr(x):
    return x.ctypes.data if isinstance(x, np.ndarray) else x


def rec_args(**over):
    text = np.frombuffer(b"@a\nAC\n+\nII\n", dtype=np.uint8)
    a = dict(text=text, n=len(text), flags=0, where=0, status=np.full(4, 7, dtype=np.uint8), cap=4)
    a.update({c: np.full(4, 7, dtype=np.uint32) for c in COLS})
    a.update(over)
    return a


def rec_call(capi, a, with_n=True):
    n, bad, tail = C.c_uint64(77), C.c_uint64(77), C.c_uint32(77)
    st = capi.lib().kh_fastq_records(*(ptr(a[f]) for f in REC_ORDER[:11]), C.byref(n) if with_n else None, C.byref(bad), C.byref(tail), 0, None)
    return st, (n.value, bad.value, tail.value)


def untouched(a, names):
    return all((a[f] == 7).all() for f in names if isinstance(a.get(f), np.ndarray))


REC_REFUSALS = [dict(n=2 ** 32), dict(flags=2), dict(flags=0x80000001), dict(where=2), dict(where=-1), dict(text=None)] + \
               [{c: None} for c in COLS] + [dict(name_lo=None, name_hi=None), dict(seq_lo=None, seq_hi=None, qual_lo=None, name_hi=None)]


@pytest.mark.parametrize("over", REC_REFUSALS, ids=lambda o: "-".join("%s" % k for k in o))
def test_records_refuses_before_anything_is_touched(capi, over):
    a = rec_args(**over)
    st, counts = rec_call(capi, a)
    assert st == capi.KH_ERR_INVALID and counts == (77, 77, 77) and untouched(a, COLS + ["status"])


def test_records_a_null_count_is_refused(capi):
    a = rec_args()
    assert rec_call(capi, a, with_n=False)[0] == capi.KH_ERR_INVALID and untouched(a, COLS + ["status"])
    a = rec_args(**{c: None for c in COLS}, status=None, cap=0)      # ... in the count pass as well
    assert rec_call(capi, a, with_n=False)[0] == capi.KH_ERR_INVALID


def test_an_empty_host_text_needs_no_device(capi):
    for a in (rec_args(n=0), rec_args(n=0, text=None), rec_args(n=0, text=None, status=None, cap=0, **{c: None for c in COLS}), rec_args(n=0, flags=1)):
        assert rec_call(capi, a) == (capi.KH_OK, (0, 0, 0)) and untouched(a, COLS + ["status"])
    n = C.c_uint64(77)      # n_bad and tail_lines may be NULL
    assert capi.lib().kh_fastq_records(None, 0, 0, 0, None, None, None, None, None, None, 0, C.byref(n), None, None, 0, None) == capi.KH_OK and n.value == 0


def pack_args(**over):
    a = dict(text=np.arange(16, dtype=np.uint8), n=16, lo=np.array([0, 4], dtype=np.uint32), hi=np.array([4, 9], dtype=np.uint32), dst=np.array([0, 8], dtype=np.uint64),
             n_rows=2, sep=10, where=0, out=np.full(32, 7, dtype=np.uint8), out_n=32)
    a.update(over)
    return a


def pack_call(capi, a):
    return capi.lib().kh_pack_rows(*(ptr(a[f]) for f in PACK_ORDER[:10]), 0, None)


PACK_REFUSALS = [dict(n=2 ** 32), dict(out_n=2 ** 32), dict(n_rows=2 ** 31 + 1), dict(sep=-2), dict(sep=256), dict(where=2), dict(where=-1), dict(lo=None), dict(hi=None),
                 dict(dst=None), dict(text=None), dict(out=None)]


@pytest.mark.parametrize("over", PACK_REFUSALS, ids=lambda o: "-".join("%s" % k for k in o))
def test_pack_refuses_before_anything_is_touched(capi, over):
    a = pack_args(**over)
    assert pack_call(capi, a) == capi.KH_ERR_INVALID and untouched(a, ["out"])


def test_pack_without_rows_or_room_needs_no_device(capi):
    for a in (pack_args(n_rows=0), pack_args(n_rows=0, lo=None, hi=None, dst=None, text=None, n=0, out=None, out_n=0), pack_args(out_n=0, out=None)):
        assert pack_call(capi, a) == capi.KH_OK and untouched(a, ["out"])


def test_python_surface(capi):
    import kmerhash_amd as kh
    from kmerhash_amd import fastq, mapper
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]      # noqa: E731
    E = inspect.Parameter.empty
    assert sig(kh.fastq_records) == [("text", E), ("strip_mate", False), ("device", 0)]
    assert sig(kh.pack_rows) == [("text", E), ("lo", E), ("hi", E), ("dst", E), ("out_len", E), ("sep", None), ("out", None), ("device", 0)]
    assert sig(kh.read_fastq) == [("text", E), ("text2", None), ("strict", True), ("strip_mate", None), ("device", 0)]
    assert kh.FastqRecords._fields == ("name_lo", "name_hi", "seq_lo", "seq_hi", "qual_lo", "status", "n_bad", "tail_lines")
    assert kh.Reads._fields == ("seq", "qual", "read_starts", "read_ends", "names", "n_reads", "status")
    assert all(getattr(kh, n) is getattr(fastq, n) for n in ("fastq_records", "pack_rows", "read_fastq", "FastqRecords", "Reads"))
    assert (fastq.STRIP_MATE, fastq.NO_AT, fastq.NO_PLUS, fastq.LENGTHS, fastq.NO_NAME) == (1, 1, 2, 4, 8)
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        assert sig(cls.map_fastq)[:3] == [("self", E), ("text", E), ("ref_text", E)]
        assert sig(cls.map_fastq_pairs)[:5] == [("self", E), ("text", E), ("ref_text", E), ("text2", None), ("rescue", False)]
    assert sig(mapper.map_fastq)[:3] == [("ix", E), ("text", E), ("ref_text", E)] and sig(mapper.map_fastq_pairs)[3:5] == [("text2", None), ("rescue", False)]
    sys_path = os.path.join(ROOT, "benchmark")
    src = open(os.path.join(sys_path, "read_mapper.py")).read()
    assert "def main(argv" in src and "write_sam_bytes" in src and "Targets.from_fasta" in src
    # the refusals of the Python calls come before the library is asked
    with pytest.raises(ValueError, match="contiguous uint8"):
        kh.pack_rows(b"abc", [0], [1], [0], 4, out=np.zeros(8, dtype=np.uint8)[::2])
    with pytest.raises(ValueError, match="one entry per row"):
        kh.pack_rows(b"abc", [0, 1], [1], [0], 4)
    with pytest.raises(ValueError, match="byte value"):
        kh.pack_rows(b"abc", [0], [1], [0], 4, sep=256)
    out = np.full(4, 7, dtype=np.uint8)
    assert kh.pack_rows(b"abc", [], [], [], 4, out=out) is out and (out == 7).all()      # no rows: nothing is queued
    r = kh.fastq_records(b"")
    assert len(r.status) == 0 and r.seq_lo.dtype == np.uint32 and (r.n_bad, r.tail_lines) == (0, 0)
    e = kh.read_fastq(b"")
    assert e.n_reads == 0 and len(e.seq) == len(e.qual) == len(e.read_starts) == len(e.read_ends) == len(e.status) == 0
    assert e.names[0].tolist() == [0] and len(e.names[1]) == 0
