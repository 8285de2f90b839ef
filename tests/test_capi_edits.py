"""CPU: kh_chain_edits is declared with the documented parameter list, bound with matching argtypes and exported; every refusal the
header lists comes back as KH_ERR_INVALID before a device is touched (this test runs without one) and leaves the outputs alone; no
anchors is KH_OK; the Python surface exists and refuses what it must before the library is asked for anything."""
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
    m = re.search(r"kh_status\s+kh_chain_edits\s*\(([^)]*)\)\s*;", txt)
    assert m, "kh_chain_edits is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert params == ["const void* qtext", "uint64_t nq", "const void* rtext", "uint64_t nr", "uint32_t ref_base", "const uint32_t* qpos",
                      "const uint32_t* rpos", "const uint8_t* rev", "const int32_t* pred", "const int32_t* chain", "uint64_t m", "uint64_t n_chains",
                      "uint32_t k", "uint32_t max_edits", "kh_mem where", "int32_t* out_link", "uint32_t* c_edits", "uint32_t* c_over", "int device",
                      "void* hip_stream"]
    assert txt.index("kh_chain_anchors") < txt.index("kh_chain_edits")
    assert re.search(r"#define\s+KH_EDITS_NOLINK\s+\(-1\)", txt) and re.search(r"#define\s+KH_EDITS_OVER\s+\(-2\)", txt)
    assert "kh_chain_edits" in capi.SYMBOLS
    f = capi.lib().kh_chain_edits                              # AttributeError: not exported
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    assert list(f.argtypes) == [vp, u64, vp, u64, u32, vp, vp, vp, vp, vp, u64, u64, u32, u32, i32, vp, vp, vp, i32, vp]
    assert f.restype is C.c_int


def test_refusals_need_no_device(capi):
    f = capi.lib().kh_chain_edits
    m, nc = 8, 2
    qt, rt = np.frombuffer(b"ACGT" * 16, dtype=np.uint8).copy(), np.frombuffer(b"ACGT" * 16, dtype=np.uint8).copy()
    q, r, v = np.arange(m, dtype=np.uint32), np.arange(m, dtype=np.uint32), np.zeros(m, dtype=np.uint8)
    pred, chain = np.arange(-1, m - 1, dtype=np.int32), np.zeros(m, dtype=np.int32)
    link, ce, co = np.full(m, 7, dtype=np.int32), np.full(nc, 7, dtype=np.uint32), np.full(nc, 7, dtype=np.uint32)
    P = lambda a: a.ctypes.data

    def call(qt=P(qt), nq=len(qt), rt=P(rt), nr=len(rt), base=0, q=P(q), r=P(r), v=P(v), pred=P(pred), chain=P(chain), m=m, nc=nc, k=4, me=31,
             where=capi.KH_MEM_HOST, link=P(link), ce=P(ce), co=P(co)):
        return f(qt, nq, rt, nr, base, q, r, v, pred, chain, m, nc, k, me, where, link, ce, co, 0, None)

    bad = [dict(k=0), dict(k=65), dict(me=32), dict(me=0xFFFFFFFF), dict(m=(1 << 24) + 1), dict(m=1 << 32), dict(nq=1 << 31), dict(nq=1 << 40),
           dict(nr=(1 << 31) + 1), dict(base=1, nr=1 << 31), dict(base=0xFFFFFFFF, nr=2), dict(base=(1 << 31) - 63), dict(where=7), dict(where=-1),
           dict(ce=None), dict(co=None), dict(qt=None), dict(rt=None), dict(q=None), dict(r=None), dict(v=None), dict(pred=None), dict(chain=None),
           dict(link=None)]
    for where in (capi.KH_MEM_HOST, capi.KH_MEM_DEVICE):
        for kw in bad:
            kw = dict(dict(where=where), **kw)
            assert call(**kw) == capi.KH_ERR_INVALID, kw
        # the parameters and the chain arrays are checked for an empty anchor list too
        for kw in (dict(k=0), dict(k=65), dict(me=32), dict(nq=1 << 31), dict(base=1, nr=1 << 31), dict(where=7), dict(ce=None), dict(co=None)):
            assert call(**dict(dict(m=0, where=where), **kw)) == capi.KH_ERR_INVALID, kw
        # nothing to verify and no chain rows: KH_OK, still without a device; the arrays may be null then
        assert call(m=0, nc=0, where=where) == capi.KH_OK
        assert call(m=0, nc=0, where=where, qt=None, nq=0, rt=None, nr=0, q=None, r=None, v=None, pred=None, chain=None, link=None, ce=None, co=None) == capi.KH_OK
    for a in (link, ce, co):
        assert (a == 7).all()                                    # refused before anything is written
    # host memory, no anchors: the chain rows are zeroed (the whole effect of the call)
    assert call(m=0) == capi.KH_OK
    assert (ce == 0).all() and (co == 0).all() and (link == 7).all()
    # a text of length 0 may be null
    assert call(m=0, nc=0, qt=None, nq=0, rt=None, nr=0) == capi.KH_OK


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import kmers
    assert kh.chain_edits is kmers.chain_edits and "chain_edits" in kh.__all__
    p = inspect.signature(kh.chain_edits).parameters
    assert list(p) == ["qtext", "rtext", "qpos", "rpos", "rev", "pred", "chain", "n_chains", "k", "ref_base", "max_edits", "device"]
    assert [p[n].default for n in list(p)[9:]] == [0, 31, 0]
    assert kmers.ChainEdits._fields == ("link", "edits", "over")
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        p = inspect.signature(cls.chain_edits).parameters
        assert list(p)[:6] == ["self", "seq", "ref_text", "read_starts", "ref_base", "max_edits"]
        assert [p[n].default for n in ("read_starts", "ref_base", "max_edits")] == [None, 0, 31]
        assert list(inspect.signature(cls.chains).parameters)[:3] == ["self", "seq", "read_starts"]
    assert kh.WideKmerPositionIndex.chain_edits is kh.KmerPositionIndex.chain_edits


def test_python_refusals_need_no_device():
    import kmerhash_amd as kh
    t = b"ACGT" * 8
    q, r, v = np.arange(8, dtype=np.uint32), np.arange(8, dtype=np.uint32), np.zeros(8, dtype=np.uint8)
    pred, chain = np.arange(-1, 7, dtype=np.int32), np.zeros(8, dtype=np.int32)
    for kw in (dict(k=0), dict(k=65), dict(k=4, max_edits=-1), dict(k=4, max_edits=32), dict(k=4, n_chains=-1), dict(k=4, ref_base=-1),
               dict(k=4, ref_base=2 ** 31)):
        with pytest.raises(ValueError):
            kh.chain_edits(t, t, q, r, v, pred, chain, **dict(dict(n_chains=1), **kw))
    with pytest.raises(ValueError, match="one entry per anchor"):
        kh.chain_edits(t, t, q, r[:7], v, pred, chain, 1, 4)
    with pytest.raises(ValueError, match="one entry per anchor"):
        kh.chain_edits(t, t, q, r, v, pred[:7], chain, 1, 4)
    with pytest.raises(ValueError, match="2\\^24"):
        big = np.zeros(2 ** 24 + 1, dtype=np.uint32)
        b8, bi = np.zeros(2 ** 24 + 1, dtype=np.uint8), np.zeros(2 ** 24 + 1, dtype=np.int32)
        kh.chain_edits(t, t, big, big, b8, bi, bi, 1, 4)
    # no anchors: no device needed, outputs of the documented types, the chain rows zero
    e, e8, ei = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int32)
    c = kh.chain_edits(t, t, e, e, e8, ei, ei, 0, 4)
    assert [len(x) for x in c] == [0, 0, 0] and c.link.dtype == np.int32 and c.edits.dtype == np.uint32 and c.over.dtype == np.uint32
    c = kh.chain_edits(b"", b"", e, e, e8, ei, ei, 3, 4)
    assert len(c.link) == 0 and c.edits.tolist() == [0, 0, 0] and c.over.tolist() == [0, 0, 0]
    # chain_edits() asks for a stranded index before anything else
    ix = kh.KmerPositionIndex.__new__(kh.KmerPositionIndex)
    ix.stranded = False
    with pytest.raises(ValueError, match="stranded=True"):
        ix.chain_edits(b"ACGT", b"ACGT")
