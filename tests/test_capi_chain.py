"""CPU: kh_chain_anchors is declared, bound with the documented signature and exported; every refusal the header lists comes back as
KH_ERR_INVALID before a device is touched (this test runs without one) and leaves every output alone, *n_chains included; the Python
surface exists and refuses what it must before the library is asked for anything."""
import ctypes as C
import inspect
import os
import re

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
    m = re.search(r"kh_status\s+kh_chain_anchors\s*\(([^)]*)\)\s*;", txt)
    assert m, "kh_chain_anchors is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert len(params) == 24
    assert params[:6] == ["const uint32_t* qpos", "const uint32_t* rpos", "const uint8_t* rev", "uint64_t m", "const uint64_t* seg_offsets", "uint64_t n_seg"]
    assert params[6:13] == ["uint32_t k", "uint32_t lookback", "uint32_t max_gap", "uint32_t band", "int32_t min_score", "uint32_t min_count", "kh_mem where"]
    assert params[13:] == ["int32_t* out_score", "int32_t* out_pred", "int32_t* out_chain", "uint32_t* c_first", "uint32_t* c_last", "uint32_t* c_count",
                           "int32_t* c_score", "uint64_t cap_chains", "uint64_t* n_chains", "int device", "void* hip_stream"]
    assert txt.index("kh_anchors_from_csr") < txt.index("kh_chain_anchors")
    assert "kh_chain_anchors" in capi.SYMBOLS
    f = capi.lib().kh_chain_anchors                          # AttributeError: not exported
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    assert list(f.argtypes) == [vp, vp, vp, u64, vp, u64, u32, u32, u32, u32, i32, u32, i32, vp, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64), i32, vp]
    assert f.restype is C.c_int


def test_refusals_need_no_device(capi):
    f = capi.lib().kh_chain_anchors
    m = 8
    q, r, v = np.arange(m, dtype=np.uint32), np.arange(m, dtype=np.uint32), np.zeros(m, dtype=np.uint8)
    seg = np.array([0, 3, 8], dtype=np.uint64)
    outs = [np.full(m, 7, dtype=np.int32) for _ in range(3)]
    tabs = [np.full(m, 7, dtype=np.uint32) for _ in range(3)] + [np.full(m, 7, dtype=np.int32)]
    INV = capi.KH_ERR_INVALID
    P = lambda a: a.ctypes.data

    def call(m=m, q=P(q), r=P(r), v=P(v), seg=P(seg), n_seg=2, k=15, h=64, G=5000, B=500, o=(P(outs[0]), P(outs[1]), P(outs[2])),
             t=tuple(P(a) for a in tabs), cap=m, where=capi.KH_MEM_HOST):
        n = C.c_uint64(123)
        return f(q, r, v, m, seg, n_seg, k, h, G, B, 40, 3, where, *o, *t, cap, C.byref(n), 0, None), n.value

    o3 = (P(outs[0]), P(outs[1]), P(outs[2]))
    bad = [dict(k=0), dict(k=65), dict(h=0), dict(h=65), dict(G=0), dict(G=1 << 31), dict(G=0xFFFFFFFF), dict(B=1 << 31), dict(B=0xFFFFFFFF),
           dict(m=(1 << 24) + 1), dict(m=1 << 32), dict(q=None), dict(r=None), dict(v=None), dict(o=(None,) + o3[1:]), dict(o=(o3[0], None, o3[2])),
           dict(o=o3[:2] + (None,)), dict(n_seg=m + (1 << 24) + 1), dict(n_seg=0), dict(t=(None,) + tuple(P(a) for a in tabs[1:])),
           dict(t=tuple(P(a) for a in tabs[:3]) + (None,)), dict(where=7)]
    for where in (capi.KH_MEM_HOST, capi.KH_MEM_DEVICE):
        for kw in bad:
            kw = dict(dict(where=where), **kw)
            assert call(**kw) == (INV, 123), kw                 # (refused before anything is written, the count included)
        for kw in (dict(k=0), dict(h=65), dict(G=0), dict(B=1 << 31), dict(where=7)):   # the parameters are checked for an empty list too
            assert call(**dict(dict(m=0, where=where), **kw)) == (INV, 123), kw
        # nothing to chain: KH_OK and no chains, still without a device
        assert call(m=0, where=where) == (capi.KH_OK, 0)
        assert call(m=0, where=where, q=None, r=None, v=None, seg=None, n_seg=0, o=(None,) * 3, t=(None,) * 4, cap=0) == (capi.KH_OK, 0)
    for a in outs + tabs:
        assert (a == 7).all()
    # the count is optional
    assert f(None, None, None, 0, None, 0, 15, 64, 5000, 500, 40, 3, capi.KH_MEM_HOST, *(None,) * 7, 0, None, 0, None) == capi.KH_OK


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import kmers
    assert kh.chain_anchors is kmers.chain_anchors and "chain_anchors" in kh.__all__
    p = inspect.signature(kh.chain_anchors).parameters
    assert list(p) == ["qpos", "rpos", "rev", "k", "seg_offsets", "lookback", "max_gap", "band", "min_score", "min_count", "device"]
    assert [p[n].default for n in list(p)[4:]] == [None, 64, 5000, 500, 40, 3, 0]
    assert kmers.Chains._fields == ("score", "pred", "chain", "first", "last", "count", "cscore")
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        assert list(inspect.signature(cls.chains).parameters)[:3] == ["self", "seq", "read_starts"]
    assert kh.WideKmerPositionIndex.chains is kh.KmerPositionIndex.chains
    assert "Chaining is the caller's" not in (kh.KmerPositionIndex.anchors.__doc__ or "")


def test_python_refusals_need_no_device():
    import kmerhash_amd as kh
    q, r, v = np.arange(8, dtype=np.uint32), np.arange(8, dtype=np.uint32), np.zeros(8, dtype=np.uint8)
    for kw in (dict(k=0), dict(k=65), dict(k=15, lookback=0), dict(k=15, lookback=65), dict(k=15, max_gap=0), dict(k=15, max_gap=2 ** 31),
               dict(k=15, band=-1), dict(k=15, band=2 ** 31), dict(k=15, min_score=2 ** 31), dict(k=15, min_count=-1),
               dict(k=15, seg_offsets=np.zeros(0, dtype=np.uint64)), dict(k=15, seg_offsets=np.zeros(1, dtype=np.uint64))):
        with pytest.raises(ValueError):
            kh.chain_anchors(q, r, v, **kw)
    with pytest.raises(ValueError, match="one entry per anchor"):
        kh.chain_anchors(q, r[:7], v, 15)
    with pytest.raises(ValueError, match="2\\^24"):
        big = np.zeros(2 ** 24 + 1, dtype=np.uint32)
        kh.chain_anchors(big, big, np.zeros(2 ** 24 + 1, dtype=np.uint8), 15)
    # no anchors: no device needed, empty outputs of the documented types
    e = np.zeros(0, dtype=np.uint32)
    c = kh.chain_anchors(e, e, np.zeros(0, dtype=np.uint8), 15)
    assert [len(x) for x in c] == [0] * 7 and c.score.dtype == np.int32 and c.first.dtype == np.uint32 and c.cscore.dtype == np.int32
    c = kh.chain_anchors(e, e, np.zeros(0, dtype=np.uint8), 15, seg_offsets=np.zeros(4, dtype=np.uint64))
    assert [len(x) for x in c] == [0] * 7
    # chains() asks for a stranded index before anything else
    ix = kh.KmerPositionIndex.__new__(kh.KmerPositionIndex)
    ix.stranded = False
    with pytest.raises(ValueError, match="stranded=True"):
        ix.chains(b"ACGT")
