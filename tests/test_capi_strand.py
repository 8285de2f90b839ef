"""CPU: the strand entry points (kh_stamp_strand, kh_index_set_stranded, kh_wide_index_set_stranded, kh_anchors_from_csr) are declared,
bound and exported; every refusal the header lists for the two handle-free calls comes back as KH_ERR_INVALID before a device is touched
(this test runs without one) and leaves the output buffers alone; the Python surface exists and refuses what it must before the library
is asked for anything."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kh_stamp_strand", "kh_index_set_stranded", "kh_wide_index_set_stranded", "kh_anchors_from_csr"]


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def test_symbols_declared_bound_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = capi.lib()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared" % s
        assert s in capi.SYMBOLS
        f = getattr(L, s)                                   # AttributeError: not exported
        assert f.argtypes, s
        assert f.restype is C.c_int
    assert len(L.kh_stamp_strand.argtypes) == 11 and len(L.kh_anchors_from_csr.argtypes) == 11
    assert list(L.kh_index_set_stranded.argtypes) == list(L.kh_wide_index_set_stranded.argtypes) == [C.c_void_p, C.c_int]
    assert re.search(r"#define\s+KH_POS_INVALID\s+0xFFFFFFFFu", txt)


def test_stamp_refusals_need_no_device(capi):
    f = capi.lib().kh_stamp_strand
    text = np.frombuffer(b"ACGT" * 20, dtype=np.uint8).copy()
    pos, out = np.arange(16, dtype=np.uint32), np.full(16, 9, dtype=np.uint32)
    INV = capi.KH_ERR_INVALID

    def call(n=len(text), k=9, m=16, pos_base=0, tptr=text.ctypes.data, pptr=pos.ctypes.data, optr=out.ctypes.data, count=True, where=capi.KH_MEM_HOST):
        bad = C.c_uint64(123)
        st = f(tptr, n, k, pptr, m, pos_base, where, optr, C.byref(bad) if count else None, 0, None)
        return st, bad.value

    for where in (capi.KH_MEM_HOST, capi.KH_MEM_DEVICE):
        for kw in (dict(k=0), dict(k=65), dict(n=1 << 31), dict(n=(1 << 31) + 7), dict(n=1 << 32), dict(pos_base=(1 << 31) - len(text) + 1),
                   dict(pos_base=0xFFFFFFFF), dict(tptr=None), dict(pptr=None), dict(optr=None)):
            assert call(where=where, **kw) == (INV, 0), kw
            assert call(where=where, count=False, **kw)[0] == INV, kw
            assert call(where=where, m=1, **kw)[0] == INV, kw
        # nothing to stamp: KH_OK, still without a device
        assert call(where=where, m=0) == (capi.KH_OK, 0)
        assert call(where=where, m=0, tptr=None, pptr=None, optr=None, n=0) == (capi.KH_OK, 0)
        assert call(where=where, m=0, pos_base=(1 << 31) - len(text)) == (capi.KH_OK, 0)
    assert (out == 9).all() and np.array_equal(pos, np.arange(16, dtype=np.uint32))


def test_anchor_refusals_need_no_device(capi):
    f = capi.lib().kh_anchors_from_csr
    qpos, offs, pos = np.arange(4, dtype=np.uint32), np.array([0, 2, 2, 5, 6], dtype=np.uint64), np.arange(6, dtype=np.uint32)
    oq, orp, orv = np.full(6, 7, dtype=np.uint32), np.full(6, 7, dtype=np.uint32), np.full(6, 7, dtype=np.uint8)
    INV = capi.KH_ERR_INVALID

    def call(n=4, total=6, q=qpos.ctypes.data, o=offs.ctypes.data, p=pos.ctypes.data, a=oq.ctypes.data, b=orp.ctypes.data, c=orv.ctypes.data,
             where=capi.KH_MEM_HOST):
        return f(q, o, n, p, total, where, a, b, c, 0, None)

    for where in (capi.KH_MEM_HOST, capi.KH_MEM_DEVICE):
        for kw in (dict(total=1 << 32), dict(total=(1 << 32) + 1, n=0), dict(q=None), dict(o=None), dict(p=None), dict(a=None), dict(b=None), dict(c=None)):
            assert call(where=where, **kw) == INV, kw
        assert call(where=where, n=0) == capi.KH_OK and call(where=where, total=0) == capi.KH_OK
        assert call(where=where, n=0, total=0, q=None, o=None, p=None, a=None, b=None, c=None) == capi.KH_OK
    assert (oq == 7).all() and (orp == 7).all() and (orv == 7).all()


def test_set_stranded_refuses_a_null_handle(capi):
    L = capi.lib()
    for on in (0, 1):
        assert L.kh_index_set_stranded(None, on) == capi.KH_ERR_INVALID
        assert L.kh_wide_index_set_stranded(None, on) == capi.KH_ERR_INVALID


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import kmers
    assert kh.stamp_strand is kmers.stamp_strand and kh.unstamp is kmers.unstamp
    for name in ("stamp_strand", "unstamp", "anchors_from_csr"):
        assert name in kh.__all__
    p = inspect.signature(kh.stamp_strand).parameters
    assert list(p) == ["text", "pos", "k", "pos_base", "device", "count_invalid"]
    assert (p["pos_base"].default, p["device"].default, p["count_invalid"].default) == (0, 0, False)
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex, kh.IndexGpuBackend, kh.WideIndexGpuBackend):
        assert inspect.signature(cls.__init__).parameters["stranded"].default is False
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        assert callable(cls.anchors)
        with pytest.raises(ValueError, match="canonical"):     # (before the library is asked for anything)
            cls(k=15, canonical=False, stranded=True)
    v = np.array([0, 1, 2, 7, (12345 << 1) | 1, 0xFFFFFFFE], dtype=np.uint32)
    pos, rc = kh.unstamp(v)
    assert pos.tolist() == [0, 0, 1, 3, 12345, 0x7FFFFFFF] and rc.tolist() == [0, 1, 0, 1, 1, 0]
    text, pp = np.frombuffer(b"ACGT" * 8, dtype=np.uint8), np.arange(4, dtype=np.uint32)
    for kw in (dict(k=0), dict(k=65), dict(k=9, pos_base=-1), dict(k=9, pos_base=2 ** 31 - 31)):
        with pytest.raises(ValueError):
            kh.stamp_strand(text, pp, **kw)
