"""CPU: kh_mate_rescue is declared with the documented parameter list, bound with matching argtypes and exported; the header stays C and
holds the definition in full; every refusal the header lists comes back as KH_ERR_INVALID before a device is touched (this test runs
without one) and leaves the outputs alone; no requests in host memory is KH_OK with offsets[0] = 0; the Python names exist with their
signatures, and the refusals and the request arithmetic of the Python layer need no device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def test_symbol_declared_bound_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"kh_status\s+kh_mate_rescue\s*\(([^)]*)\)\s*;", txt)
    assert m, "kh_mate_rescue is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert params == ["const void* qtext", "uint64_t nq", "const void* rtext", "uint64_t nr", "uint32_t ref_base", "const uint32_t* q_lo", "const uint32_t* q_hi",
                      "const uint32_t* w_lo", "const uint32_t* w_hi", "const uint8_t* rev", "uint64_t n", "uint32_t max_edits", "kh_mem where", "int32_t* out_edits",
                      "uint32_t* out_rs", "uint32_t* out_re", "uint32_t* out_span", "uint64_t* out_offsets", "uint32_t* out_ops", "uint64_t cap_ops", "uint64_t* n_ops",
                      "int device", "void* hip_stream"]
    assert txt.index("kh_pair_chains") < txt.index("kh_mate_rescue")
    for name, value in (("KH_RESCUE_NONE", "(-1)"), ("KH_RESCUE_OVER", "(-2)"), ("KH_RESCUE_MAX_READ", "512u"), ("KH_RESCUE_MAX_WINDOW", "65536u")):
        assert re.search(r"#define\s+%s\s+%s\s" % (name, re.escape(value)), txt), name
    # the definition stands in the header in full
    for phrase in ("Which requests are looked at", "D[0][c] = 0 for every c", "the smallest c attaining d*", "for a HEAD", "never stops early", "EQUALS d* BY CONSTRUCTION",
                   "the smaller |d| wins, then d < 0", "out_span <= out_edits", "reference order"):
        assert phrase in raw, phrase
    assert "kh_mate_rescue" in capi.SYMBOLS
    f = capi.lib().kh_mate_rescue                               # AttributeError: not exported
    vp, u64, u32, i32, pu64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)
    assert list(f.argtypes) == [vp, u64, vp, u64, u32, vp, vp, vp, vp, vp, u64, u32, i32, vp, vp, vp, vp, vp, vp, u64, pu64, i32, vp]
    assert f.restype is C.c_int


def test_the_header_stays_c(capi, tmp_path):
    src = tmp_path / "use_rescue.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  uint64_t n = 7, offs[1] = {7};\n'
                   '  kh_status a = kh_mate_rescue(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 32, KH_MEM_HOST, 0, 0, 0, 0, offs, 0, 0, &n, 0, 0);\n'      # max_edits = 32
                   '  kh_status b = kh_mate_rescue(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 31, KH_MEM_HOST, 0, 0, 0, 0, offs, 0, 0, &n, 0, 0);\n'      # nothing to do
                   '  printf("%d %d %d %d %d %d\\n", (int)a, (int)b, (int)n, (int)offs[0], KH_RESCUE_NONE, KH_RESCUE_OVER);\n  return 0;\n}\n')
    exe = tmp_path / "use_rescue"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["1", "0", "0", "0", "-1", "-2"], r.stdout


def test_refusals_need_no_device(capi):
    f = capi.lib().kh_mate_rescue
    nreq = 2
    qt, rt = np.frombuffer(b"ACGT" * 16, dtype=np.uint8).copy(), np.frombuffer(b"ACGT" * 16, dtype=np.uint8).copy()
    lo, hi = np.zeros(nreq, dtype=np.uint32), np.full(nreq, 20, dtype=np.uint32)
    wl, wh, rv = np.zeros(nreq, dtype=np.uint32), np.full(nreq, 64, dtype=np.uint32), np.zeros(nreq, dtype=np.uint8)
    ed = np.full(nreq, 7, dtype=np.int32)
    nums = [np.full(nreq, 7, dtype=np.uint32) for _ in range(3)]
    offs, ops = np.full(nreq + 1, 7, dtype=np.uint64), np.full(64, 7, dtype=np.uint32)
    n = C.c_uint64(7)
    P = lambda a: a.ctypes.data          # noqa: E731

    def call(qt=P(qt), nq=len(qt), rt=P(rt), nr=len(rt), base=0, lo=P(lo), hi=P(hi), wl=P(wl), wh=P(wh), rv=P(rv), nreq=nreq, me=31, where=capi.KH_MEM_HOST,
             ed=P(ed), rs=P(nums[0]), re_=P(nums[1]), sp=P(nums[2]), offs=P(offs), ops=P(ops), cap=64, n=C.byref(n)):
        return f(qt, nq, rt, nr, base, lo, hi, wl, wh, rv, nreq, me, where, ed, rs, re_, sp, offs, ops, cap, n, 0, None)

    bad = [dict(me=32), dict(me=1 << 31), dict(nreq=(1 << 24) + 1), dict(nreq=1 << 40), dict(nq=1 << 31), dict(nq=1 << 40), dict(nr=(1 << 31) + 1),
           dict(base=1, nr=1 << 31), dict(base=0xFFFFFFFF, nr=2), dict(base=(1 << 31) - 63), dict(where=7), dict(where=-1), dict(offs=None), dict(n=None),
           dict(lo=None), dict(hi=None), dict(wl=None), dict(wh=None), dict(rv=None), dict(ed=None), dict(rs=None), dict(re_=None), dict(sp=None),
           dict(qt=None), dict(rt=None)]
    for where in (capi.KH_MEM_HOST, capi.KH_MEM_DEVICE):
        for kw in bad:
            assert call(**dict(dict(where=where), **kw)) == capi.KH_ERR_INVALID, kw
        # the parameters are checked for an empty request list too
        for kw in (dict(me=32), dict(nq=1 << 31), dict(base=1, nr=1 << 31), dict(where=7), dict(offs=None), dict(n=None)):
            assert call(**dict(dict(nreq=0, where=where), **kw)) == capi.KH_ERR_INVALID, kw
    for a in nums + [ed, offs, ops]:
        assert (a == 7).all()                                    # refused before anything is written
    assert n.value == 7
    # host memory, no requests: offsets[0] = 0 and no runs are the whole effect of the call; every array may be null then
    assert call(nreq=0, qt=None, nq=0, rt=None, nr=0, lo=None, hi=None, wl=None, wh=None, rv=None, ed=None, rs=None, re_=None, sp=None, ops=None, cap=0) == capi.KH_OK
    assert n.value == 0 and offs[0] == 0 and (offs[1:] == 7).all() and (ops == 7).all() and (ed == 7).all() and all((a == 7).all() for a in nums)


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import kmers, sam
    for name in ("rescue_mates", "rescue_requests", "MateRescue", "RESCUE_NONE", "RESCUE_OVER"):
        assert getattr(kh, name) is getattr(kmers, name) and name in kh.__all__
    assert kh.write_sam_rescued is sam.write_sam_rescued and "write_sam_rescued" in kh.__all__
    assert (kh.RESCUE_NONE, kh.RESCUE_OVER) == (-1, -2)
    assert kh.MateRescue._fields == ("read", "edits", "rs", "re", "rev", "span", "offsets", "ops")
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]      # noqa: E731
    E = inspect.Parameter.empty
    assert sig(kh.rescue_mates) == [("qtext", E), ("rtext", E), ("q_lo", E), ("q_hi", E), ("w_lo", E), ("w_hi", E), ("rev", E), ("ref_base", 0), ("max_edits", 31),
                                    ("device", 0)]
    assert sig(kh.rescue_requests)[:9] == [("mapping", E), ("pairs", E), ("read_starts", E), ("read_ends", E), ("min_ins", 0), ("max_ins", 1000), ("max_edits", 31),
                                           ("targets", None), ("ref_len", None)]
    wp, wr = sig(kh.write_sam_pairs), sig(kh.write_sam_rescued)
    assert wr[:4] == [("fh", E), ("mapping", E), ("pairs", E), ("rescue", E)] and wr[:3] + wr[4:] == wp      # write_sam_pairs' arguments, the MateRescue fourth
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        assert sig(cls.map_pairs_rescued) == sig(cls.map_pairs)
    assert kh.WideKmerPositionIndex.map_pairs_rescued is kh.KmerPositionIndex.map_pairs_rescued


def test_python_refusals_and_requests_need_no_device():
    import kmerhash_amd as kh
    from kmerhash_amd import kmers
    t = b"ACGT" * 8
    one = lambda v, dt=np.uint32: np.array([v], dtype=dt)      # noqa: E731
    for kw in (dict(max_edits=32), dict(max_edits=-1), dict(ref_base=-1), dict(ref_base=2 ** 31)):
        with pytest.raises(ValueError):
            kh.rescue_mates(t, t, one(0), one(8), one(0), one(32), one(0, np.uint8), **kw)
    with pytest.raises(ValueError, match="one entry per request"):
        kh.rescue_mates(t, t, one(0), one(8), one(0), np.zeros(0, dtype=np.uint32), one(0, np.uint8))
    # no requests: no device needed, outputs of the documented types
    e = np.zeros(0, dtype=np.uint32)
    r = kh.rescue_mates(t, t, e, e, e, e, np.zeros(0, dtype=np.uint8))
    assert r.offsets.tolist() == [0] and all(len(x) == 0 for x in (r.read, r.edits, r.rs, r.re, r.rev, r.span, r.ops))
    assert [x.dtype for x in r] == [np.uint32, np.int32, np.uint32, np.uint32, np.uint8, np.uint32, np.uint64, np.uint32]
    # the requests: 4 pairs of 100-base reads; a Mapping of four rows, each the row of one read
    z = lambda v, dt: np.array(v, dtype=dt)      # noqa: E731
    table = kh.index.ChainTable(None, z([0, 1, 0, 0], np.uint8), None, None, None, None, None, None, None, None)
    rec = kmers.ChainRecords(None, None, None, z([5000, 9000, 300, 19950], np.uint32), z([5100, 9100, 400, 20000], np.uint32), None, None, None, None, None, None)
    mapping = kmers.Mapping(table, None, None, None, None, rec)
    row = z([0, -1, -1, 1, -1, 2, 3, -1, -1, -1], np.int32)      # pair 4: nobody has a row
    pairs = kmers.PairSelect(row, None, None, None, None, None)
    starts = np.arange(10) * 100
    rq = kh.rescue_requests(mapping, pairs, starts, starts + 100, min_ins=200, max_ins=600, max_edits=31, ref_len=20000)
    assert rq.read.tolist() == [1, 2, 4, 7] and rq.q_lo.tolist() == [100, 200, 400, 700] and rq.q_hi.tolist() == [200, 300, 500, 800]
    # read 1: partner forward at [5000, 5100) -> reverse in [max(5000, 5000 + 200 - 100 - 31), 5600)
    # read 2: partner reverse at [9000, 9100) -> forward in [9100 - 600, min(9100, 9100 - 200 + 100 + 31))
    # read 4: partner forward at [300, 400) -> [369, 900); read 7: partner forward at [19950, 20000) -> clamped to the text's end
    assert rq.rev.tolist() == [1, 0, 1, 1] and rq.w_lo.tolist() == [5069, 8500, 369, 20000] and rq.w_hi.tolist() == [5600, 9031, 900, 20000]
    assert [x.dtype for x in rq] == [np.uint32] * 4 + [np.uint8, np.uint32]
    # targets a = [0, 5300) and b = [5364, 19364): the window stops at the partner's target, and a partner on no target asks for nothing
    T = kh.Targets(["a", "b"], [5300, 14000], spacer=64)
    rq = kh.rescue_requests(mapping, pairs, starts, starts + 100, min_ins=200, max_ins=600, max_edits=31, targets=T)
    assert rq.read.tolist() == [1, 2, 4] and rq.w_lo.tolist() == [5069, 8500, 369] and rq.w_hi.tolist() == [5300, 9031, 900]
    with pytest.raises(ValueError, match="ref_len"):
        kh.rescue_requests(mapping, pairs, starts, starts + 100)
    with pytest.raises(ValueError, match="one entry per read"):
        kh.rescue_requests(mapping, pairs, starts[:8], starts[:8] + 100, ref_len=20000)
    ix = kh.KmerPositionIndex.__new__(kh.KmerPositionIndex)
    ix.stranded = False
    with pytest.raises(ValueError, match="stranded=True"):
        ix.map_pairs_rescued(b"ACGT", b"ACGT", [0, 2])
