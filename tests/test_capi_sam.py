"""CPU: kh_record_diffs and kh_oriented_rows are declared, bound with matching argtypes and exported; every refusal the header lists
comes back as KH_ERR_INVALID before a device is touched (this test runs without one) and leaves the outputs alone; no rows in host
memory are KH_OK without a device; the Python surface exists with its signatures."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIFF_ORDER = ["qtext", "nq", "rtext", "nr", "ref_base", "offsets", "ops", "n_ops", "valid", "rev", "q_lo", "q_hi", "rs", "n_rows", "kind", "where", "out_ok", "out_offsets",
              "out_text", "cap_text", "n_text", "device", "hip_stream"]
ROWS_ORDER = ["text", "n", "lo", "hi", "rev", "n_rows", "complement", "where", "out_offsets", "out_text", "cap_text", "n_text", "device", "hip_stream"]


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def test_symbols_declared_bound_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, order in (("kh_record_diffs", DIFF_ORDER), ("kh_oriented_rows", ROWS_ORDER)):
        m = re.search(r"kh_status\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
        assert m, "%s is not declared" % name
        assert [re.sub(r"\s+", " ", p).strip().split(" ")[-1].lstrip("*") for p in m.group(1).split(",")] == order
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    assert txt.index("kh_anchor_targets") < txt.index("kh_record_diffs") < txt.index("kh_oriented_rows")
    assert re.search(r"#define\s+KH_DIFF_CS\s+0u", txt) and re.search(r"#define\s+KH_DIFF_MD\s+1u", txt)
    for phrase in ("ORIENTED READ", "spoils the\n *      row", "\"acgtn\"[R]", "\"ACGTN\"[R]", "[0-9]+(([A-Z]|\\^[A-Z]+)[0-9]+)*", "A<->T, C<->G"):
        assert phrase in raw, phrase
    vp, u64, u32, i32, pu64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)
    f, g = capi.lib().kh_record_diffs, capi.lib().kh_oriented_rows
    assert list(f.argtypes) == [vp, u64, vp, u64, u32, vp, vp, u64, vp, vp, vp, vp, vp, u64, u32, i32, vp, vp, vp, u64, pu64, i32, vp]
    assert list(g.argtypes) == [vp, u64, vp, vp, vp, u64, u32, i32, vp, vp, u64, pu64, i32, vp]
    assert f.restype is C.c_int and g.restype is C.c_int


def diff_args(**over):
    rows = 3
    a = dict(qtext=np.full(64, 65, dtype=np.uint8), nq=64, rtext=np.full(64, 65, dtype=np.uint8), nr=64, ref_base=0, offsets=np.arange(rows + 1, dtype=np.uint64),
             ops=np.full(rows, (8 << 4) | 7, dtype=np.uint32), n_ops=rows, valid=np.ones(rows, dtype=np.uint8), rev=np.zeros(rows, dtype=np.uint8),
             q_lo=np.zeros(rows, dtype=np.uint32), q_hi=np.full(rows, 8, dtype=np.uint32), rs=np.zeros(rows, dtype=np.uint32), n_rows=rows, kind=0, where=0,
             out_ok=np.full(rows, 7, dtype=np.uint8), out_offsets=np.full(rows + 1, 7, dtype=np.uint64), out_text=np.full(32, 7, dtype=np.uint8), cap_text=32)
    a.update(over)
    return a


def rows_args(**over):
    rows = 3
    a = dict(text=np.full(64, 65, dtype=np.uint8), n=64, lo=np.zeros(rows, dtype=np.uint32), hi=np.full(rows, 8, dtype=np.uint32), rev=np.zeros(rows, dtype=np.uint8),
             n_rows=rows, complement=1, where=0, out_offsets=np.full(rows + 1, 7, dtype=np.uint64), out_text=np.full(32, 7, dtype=np.uint8), cap_text=32)
    a.update(over)
    return a


def call(capi, name, order, a, with_n=True):
    n = C.c_uint64(77)
    vals = [a[f].ctypes.data if isinstance(a[f], np.ndarray) else a[f] for f in order[:-3]]
    st = getattr(capi.lib(), name)(*vals, C.byref(n) if with_n else None, 0, None)
    return st, n.value


def untouched(a):
    return all((a[f] == 7).all() for f in ("out_ok", "out_offsets", "out_text") if isinstance(a.get(f), np.ndarray))


DIFF_REFUSALS = [dict(kind=2), dict(kind=0xFFFFFFFF), dict(n_rows=2 ** 31 + 1), dict(n_ops=2 ** 31 + 1), dict(nq=2 ** 32 + 1), dict(nr=2 ** 32 + 1), dict(where=2), dict(where=-1),
                 dict(out_offsets=None), dict(offsets=None), dict(valid=None), dict(rev=None), dict(q_lo=None), dict(q_hi=None), dict(rs=None), dict(out_ok=None),
                 dict(ops=None), dict(qtext=None), dict(rtext=None)]
ROWS_REFUSALS = [dict(complement=2), dict(n_rows=2 ** 31 + 1), dict(n=2 ** 32 + 1), dict(where=2), dict(where=-1), dict(out_offsets=None), dict(lo=None), dict(hi=None),
                 dict(rev=None), dict(text=None)]


@pytest.mark.parametrize("over", DIFF_REFUSALS, ids=lambda o: "-".join("%s" % k for k in o))
def test_record_diffs_refuses_before_anything_is_touched(capi, over):
    a = diff_args(**over)
    st, n = call(capi, "kh_record_diffs", DIFF_ORDER, a)
    assert st == capi.KH_ERR_INVALID and n == 77 and untouched(a)


@pytest.mark.parametrize("over", ROWS_REFUSALS, ids=lambda o: "-".join("%s" % k for k in o))
def test_oriented_rows_refuses_before_anything_is_touched(capi, over):
    a = rows_args(**over)
    st, n = call(capi, "kh_oriented_rows", ROWS_ORDER, a)
    assert st == capi.KH_ERR_INVALID and n == 77 and untouched(a)


def test_a_null_count_is_refused(capi):
    for name, order, a in (("kh_record_diffs", DIFF_ORDER, diff_args()), ("kh_oriented_rows", ROWS_ORDER, rows_args())):
        assert call(capi, name, order, a, with_n=False)[0] == capi.KH_ERR_INVALID and untouched(a)


def test_no_rows_in_host_memory_need_no_device(capi):
    nothing = dict(offsets=None, ops=None, n_ops=0, valid=None, rev=None, q_lo=None, q_hi=None, rs=None, n_rows=0, out_ok=None, qtext=None, nq=0, rtext=None, nr=0)
    for kind in (0, 1):
        a = diff_args(kind=kind, **nothing)
        assert call(capi, "kh_record_diffs", DIFF_ORDER, a) == (capi.KH_OK, 0)
        assert a["out_offsets"][0] == 0 and (a["out_offsets"][1:] == 7).all() and (a["out_text"] == 7).all()
    a = rows_args(text=None, n=0, lo=None, hi=None, rev=None, n_rows=0)
    assert call(capi, "kh_oriented_rows", ROWS_ORDER, a) == (capi.KH_OK, 0)
    assert a["out_offsets"][0] == 0 and (a["out_offsets"][1:] == 7).all() and (a["out_text"] == 7).all()


def test_python_surface(capi):
    import kmerhash_amd as kh
    from kmerhash_amd import sam
    from collections import namedtuple
    assert kh.RecordDiffs._fields == ("ok", "offsets", "text")
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]      # noqa: E731
    E = inspect.Parameter.empty
    assert sig(kh.record_diffs) == [("qtext", E), ("rtext", E), ("records", E), ("rev", E), ("q_lo", E), ("q_hi", E), ("kind", "cs"), ("ref_base", 0), ("device", 0)]
    assert sig(kh.oriented_rows) == [("text", E), ("lo", E), ("hi", E), ("rev", E), ("complement", True), ("device", 0)]
    assert sig(kh.sam_header) == [("targets", None), ("ref_name", None), ("ref_len", None)]
    assert sig(kh.write_sam) == [("fh", E), ("mapping", E), ("seq", E), ("ref_text", E), ("read_names", E), ("read_starts", E), ("read_ends", None), ("qual", None),
                                 ("ref_name", None), ("ref_len", None), ("ref_start", 0), ("ref_base", 0), ("targets", None), ("kept_only", True), ("unmapped", True),
                                 ("header", True), ("md", True), ("cs", False), ("device", 0)]
    assert sig(kh.write_paf)[-1] == ("cs", None) and sig(kh.paf_lines)[-1] == ("cs", None)
    assert all(getattr(kh, n) is getattr(sam, n) for n in ("record_diffs", "oriented_rows", "sam_header", "sam_lines", "write_sam", "RecordDiffs"))
    # the refusals that need no call
    Rec = namedtuple("Rec", "valid rs offsets ops")
    z = lambda n, dt: np.zeros(n, dtype=dt)      # noqa: E731
    with pytest.raises(ValueError, match="'cs' or 'md'"):
        kh.record_diffs(b"", b"", Rec(z(0, np.uint8), z(0, np.uint32), z(1, np.uint64), z(0, np.uint32)), z(0, np.uint8), z(0, np.uint32), z(0, np.uint32), kind="MD")
    with pytest.raises(ValueError, match="one entry per row"):
        kh.record_diffs(b"", b"", Rec(z(2, np.uint8), z(2, np.uint32), z(3, np.uint64), z(0, np.uint32)), z(1, np.uint8), z(2, np.uint32), z(2, np.uint32))
    got = kh.record_diffs(b"", b"", Rec(z(0, np.uint8), z(0, np.uint32), z(1, np.uint64), z(0, np.uint32)), z(0, np.uint8), z(0, np.uint32), z(0, np.uint32), kind="md")
    assert [len(x) for x in got] == [0, 1, 0] and got.offsets[0] == 0
    offs, text = kh.oriented_rows(b"ACGT", z(0, np.uint32), z(0, np.uint32), z(0, np.uint8))
    assert list(offs) == [0] and len(text) == 0
