"""CPU: kh_sam_lines is declared after kh_mate_rescue and before kh_release_cached_memory, bound with matching argtypes and exported;
every refusal the header lists comes back as KH_ERR_INVALID before a device is touched (this test runs without one) and leaves the
outputs alone; no lines in host memory are KH_OK without a device; the Python surface exists with its signatures."""
import ctypes as C
import inspect
import io
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRS = ["names", "tnames", "cigar", "seq", "qual", "md", "cs"]
COLS = ["l_name", "l_flag", "l_rname", "l_pos", "l_mapq", "l_cigar", "l_rnext", "l_pnext", "l_tlen", "l_seq", "l_qual", "l_tags", "l_nm", "l_tp", "l_cm", "l_s1", "l_s2",
        "l_md", "l_cs"]
COL_DTYPES = [np.int32, np.uint32, np.int32, np.uint32, np.uint8, np.int32, np.int32, np.uint32, np.int32, np.int32, np.int32, np.uint8, np.uint32, np.uint8, np.uint32,
              np.int32, np.int32, np.int32, np.int32]
ORDER = [a for x in CSRS for a in (x + "_off", x + "_text", "n_" + x, x + "_bytes")] + COLS + ["n_lines", "where", "out_offsets", "out_text", "cap_text", "n_text", "device",
                                                                                                "hip_stream"]


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def test_symbol_declared_bound_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"kh_status\s+kh_sam_lines\s*\(([^)]*)\)\s*;", txt)
    assert m, "kh_sam_lines is not declared"
    assert [re.sub(r"\s+", " ", p).strip().split(" ")[-1].lstrip("*") for p in m.group(1).split(",")] == ORDER
    assert "kh_sam_lines" in capi.SYMBOLS and hasattr(capi.lib(), "kh_sam_lines")
    assert txt.index("kh_mate_rescue") < txt.index("kh_sam_lines") < txt.index("kh_release_cached_memory")
    for name, value in (("KH_SAMTAG_BASE", "1u"), ("KH_SAMTAG_S2", "2u"), ("KH_SAMTAG_MD", "4u"), ("KH_SAMTAG_CS", "8u"), ("KH_SAM_RNEXT_SAME", r"\(-2\)"),
                        ("KH_SAM_LINE_FIXED", "256u")):
        assert re.search(r"#define\s+%s\s+%s" % (name, value), txt), name
    for phrase in ("'*' where the row is outside OR empty", "exactly the 11 mandatory fields", "what \"%d\" prints", "names_bytes + 2 tnames_bytes"):
        assert phrase in raw, phrase
    vp, u64, i32, pu64 = C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)
    f = capi.lib().kh_sam_lines
    assert list(f.argtypes) == [vp, vp, u64, u64] * 7 + [vp] * 19 + [u64, i32, vp, vp, u64, pu64, i32, vp] and len(f.argtypes) == len(ORDER)
    assert f.restype is C.c_int


def args(**over):
    n = 3
    a = {}
    for x in CSRS:
        a.update({x + "_off": np.arange(n + 1, dtype=np.uint64), x + "_text": np.full(n, 65, dtype=np.uint8), "n_" + x: n, x + "_bytes": n})
    a.update({c: np.zeros(n, dtype=dt) for c, dt in zip(COLS, COL_DTYPES)})
    a.update(n_lines=n, where=0, out_offsets=np.full(n + 1, 7, dtype=np.uint64), out_text=np.full(256, 7, dtype=np.uint8), cap_text=256)
    a.update(over)
    return a


def call(capi, a, with_n=True):
    n = C.c_uint64(77)
    vals = [a[f].ctypes.data if isinstance(a[f], np.ndarray) else a[f] for f in ORDER[:-3]]
    st = capi.lib().kh_sam_lines(*vals, C.byref(n) if with_n else None, 0, None)
    return st, n.value


def untouched(a):
    return all((a[f] == 7).all() for f in ("out_offsets", "out_text") if isinstance(a.get(f), np.ndarray))


REFUSALS = ([dict(n_lines=2 ** 31 + 1), dict(where=2), dict(where=-1), dict(out_offsets=None)] +
            [{"n_" + x: 2 ** 31 + 1} for x in CSRS] + [{x + "_bytes": 2 ** 32 + 1} for x in CSRS] + [{x + "_off": None} for x in CSRS] + [{x + "_text": None} for x in CSRS] +
            [{c: None} for c in COLS] +
            # a line could reach 2^32 bytes: the sum of the text sizes (a target name can print twice) and the fixed part of a line
            [dict(seq_bytes=2 ** 32 - 256 - 3 * 7), dict(tnames_bytes=2 ** 31 - 128 - 3 * 3 + 1), dict(seq_bytes=2 ** 31, qual_bytes=2 ** 31)])


@pytest.mark.parametrize("over", REFUSALS, ids=lambda o: "-".join("%s" % k for k in o))
def test_refuses_before_anything_is_touched(capi, over):
    a = args(**over)
    st, n = call(capi, a)
    assert st == capi.KH_ERR_INVALID and n == 77 and untouched(a)


def test_a_null_count_is_refused(capi):
    a = args()
    assert call(capi, a, with_n=False)[0] == capi.KH_ERR_INVALID and untouched(a)


def test_no_lines_in_host_memory_need_no_device(capi):
    nothing = {c: None for c in COLS}
    for x in CSRS:
        nothing.update({x + "_off": None, x + "_text": None, "n_" + x: 0, x + "_bytes": 0})
    a = args(n_lines=0, **nothing)
    assert call(capi, a) == (capi.KH_OK, 0)
    assert a["out_offsets"][0] == 0 and (a["out_offsets"][1:] == 7).all() and (a["out_text"] == 7).all()
    a = args(n_lines=0)      # ... nor with CSRs that hold rows
    assert call(capi, a) == (capi.KH_OK, 0) and a["out_offsets"][0] == 0


def test_python_surface(capi):
    import kmerhash_amd as kh
    from kmerhash_amd import sam
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]      # noqa: E731
    E = inspect.Parameter.empty
    common = [("mapping", E), ("seq", E), ("ref_text", E), ("read_names", E), ("read_starts", E), ("read_ends", None), ("qual", None), ("ref_name", None), ("ref_len", None),
              ("ref_start", 0), ("ref_base", 0), ("targets", None), ("kept_only", True), ("unmapped", True)]
    assert sig(kh.sam_text) == common + [("md", True), ("cs", False), ("pairs", None), ("device", 0)]
    assert sig(kh.write_sam_bytes) == [("fh", E)] + common + [("header", True), ("md", True), ("cs", False), ("pairs", None), ("device", 0)]
    assert sig(kh.names_csr) == [("names", E)]
    assert sig(kh.sam_line_columns)[:2] == [("xp", E), ("mapping", E)] and sig(kh.sam_line_columns)[-3:] == [("pairs", None), ("diff_ok", ()), ("refuse", ())]
    assert kh.SamText._fields == ("header", "offsets", "text", "lines", "skipped", "unmapped_reads")
    assert kh.LineColumns._fields[:19] == sam.LINE_COLUMNS == tuple(c[2:] for c in COLS) and [np.dtype(d) for d in sam.LINE_DTYPES] == [np.dtype(d) for d in COL_DTYPES]
    assert all(getattr(kh, n) is getattr(sam, n) for n in ("names_csr", "sam_line_columns", "sam_lines_text", "sam_text", "write_sam_bytes", "SamText", "LineColumns"))
    assert (sam.TAG_BASE, sam.TAG_S2, sam.TAG_MD, sam.TAG_CS, sam.RNEXT_SAME) == (1, 2, 4, 8, -2)
    for f in (kh.sam_text, kh.write_sam_bytes):
        assert "MateRescue is not taken" in f.__doc__ and "write_sam_rescued() keeps the" in f.__doc__
    # no lines: nothing is queued, the zeroed offset is the answer
    offs, text = kh.sam_lines_text(None, None, None, None, None, None, None, [np.zeros(0, dtype=dt) for dt in COL_DTYPES])
    assert offs.tolist() == [0] and len(text) == 0
    with pytest.raises(ValueError, match="same memory and have one entry per line"):
        kh.sam_lines_text(None, None, None, None, None, None, None, [np.zeros(int(i == 3), dtype=dt) for i, dt in enumerate(COL_DTYPES)])
