"""CPU: kh_chain_cigars is declared with the documented parameter list, bound with matching argtypes and exported; the header stays C;
every refusal the header lists comes back as KH_ERR_INVALID before a device is touched (this test runs without one) and leaves the
outputs alone; no anchors in host memory is KH_OK with offsets[0] = 0 and zeroed chain rows; the Python surface exists."""
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
    m = re.search(r"kh_status\s+kh_chain_cigars\s*\(([^)]*)\)\s*;", txt)
    assert m, "kh_chain_cigars is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert params == ["const void* qtext", "uint64_t nq", "const void* rtext", "uint64_t nr", "uint32_t ref_base", "const uint32_t* qpos",
                      "const uint32_t* rpos", "const uint8_t* rev", "const int32_t* pred", "const int32_t* chain", "uint64_t m", "uint64_t n_chains",
                      "uint32_t k", "const int32_t* link", "kh_mem where", "uint64_t* out_offsets", "uint32_t* out_ops", "uint64_t cap_ops", "uint64_t* n_ops",
                      "uint32_t* c_ins", "uint32_t* c_del", "int device", "void* hip_stream"]
    assert txt.index("kh_chain_edits") < txt.index("kh_chain_cigars")
    # the definition of a non-empty row and of the canonical alignment stand in the header in full
    for phrase in ("Which rows are non-empty", "Canonical alignment", "dropped,", "the first of X, I, D", "dq < 2^28"):
        assert phrase in raw, phrase
    assert "kh_chain_cigars" in capi.SYMBOLS
    f = capi.lib().kh_chain_cigars                             # AttributeError: not exported
    vp, u64, u32, i32, pu64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)
    assert list(f.argtypes) == [vp, u64, vp, u64, u32, vp, vp, vp, vp, vp, u64, u64, u32, vp, i32, vp, vp, u64, pu64, vp, vp, i32, vp]
    assert f.restype is C.c_int


def test_the_header_stays_c(capi, tmp_path):
    src = tmp_path / "use_cigars.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  uint64_t n = 7, offs[1] = {7};\n'
                   '  kh_status a = kh_chain_cigars(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, KH_MEM_HOST, offs, 0, 0, &n, 0, 0, 0, 0);\n'      # k = 0
                   '  kh_status b = kh_chain_cigars(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 15, 0, KH_MEM_HOST, offs, 0, 0, &n, 0, 0, 0, 0);\n'     # nothing to do
                   '  printf("%d %d %d %d\\n", (int)a, (int)b, (int)n, (int)offs[0]);\n  return 0;\n}\n')
    exe = tmp_path / "use_cigars"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["1", "0", "0", "0"], r.stdout


def test_refusals_need_no_device(capi):
    f = capi.lib().kh_chain_cigars
    m, nc = 8, 2
    qt, rt = np.frombuffer(b"ACGT" * 16, dtype=np.uint8).copy(), np.frombuffer(b"ACGT" * 16, dtype=np.uint8).copy()
    q, r, v = np.arange(m, dtype=np.uint32), np.arange(m, dtype=np.uint32), np.zeros(m, dtype=np.uint8)
    pred, chain, link = np.arange(-1, m - 1, dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
    offs, ops = np.full(m + 1, 7, dtype=np.uint64), np.full(64, 7, dtype=np.uint32)
    ci, cd = np.full(nc, 7, dtype=np.uint32), np.full(nc, 7, dtype=np.uint32)
    n = C.c_uint64(7)
    P = lambda a: a.ctypes.data          # noqa: E731

    def call(qt=P(qt), nq=len(qt), rt=P(rt), nr=len(rt), base=0, q=P(q), r=P(r), v=P(v), pred=P(pred), chain=P(chain), m=m, nc=nc, k=4, link=P(link),
             where=capi.KH_MEM_HOST, offs=P(offs), ops=P(ops), cap=64, n=C.byref(n), ci=P(ci), cd=P(cd)):
        return f(qt, nq, rt, nr, base, q, r, v, pred, chain, m, nc, k, link, where, offs, ops, cap, n, ci, cd, 0, None)

    bad = [dict(k=0), dict(k=65), dict(m=(1 << 24) + 1), dict(m=1 << 32), dict(nq=1 << 31), dict(nq=1 << 40), dict(nr=(1 << 31) + 1), dict(base=1, nr=1 << 31),
           dict(base=0xFFFFFFFF, nr=2), dict(base=(1 << 31) - 63), dict(where=7), dict(where=-1), dict(ci=None), dict(cd=None), dict(offs=None), dict(n=None),
           dict(qt=None), dict(rt=None), dict(q=None), dict(r=None), dict(v=None), dict(pred=None), dict(chain=None), dict(link=None)]
    for where in (capi.KH_MEM_HOST, capi.KH_MEM_DEVICE):
        for kw in bad:
            assert call(**dict(dict(where=where), **kw)) == capi.KH_ERR_INVALID, kw
        # the parameters and the chain arrays are checked for an empty anchor list too
        for kw in (dict(k=0), dict(k=65), dict(nq=1 << 31), dict(base=1, nr=1 << 31), dict(where=7), dict(ci=None), dict(cd=None), dict(offs=None), dict(n=None)):
            assert call(**dict(dict(m=0, where=where), **kw)) == capi.KH_ERR_INVALID, kw
    for a in (offs, ops, ci, cd):
        assert (a == 7).all()                                    # refused before anything is written
    assert n.value == 7
    # host memory, no anchors: offsets[0] = 0, no runs, the chain rows zeroed (the whole effect of the call); the arrays may be null then
    assert call(m=0, qt=None, nq=0, rt=None, nr=0, q=None, r=None, v=None, pred=None, chain=None, link=None, ops=None, cap=0) == capi.KH_OK
    assert n.value == 0 and offs[0] == 0 and (offs[1:] == 7).all() and (ci == 0).all() and (cd == 0).all() and (ops == 7).all()
    assert call(m=0, nc=0, ci=None, cd=None) == capi.KH_OK


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import kmers
    assert kh.chain_cigars is kmers.chain_cigars and kh.cigar_string is kmers.cigar_string and {"chain_cigars", "cigar_string"} <= set(kh.__all__)
    p = inspect.signature(kh.chain_cigars).parameters
    assert list(p) == ["qtext", "rtext", "qpos", "rpos", "rev", "pred", "chain", "n_chains", "k", "link", "ref_base", "device"]
    assert [p[n].default for n in list(p)[10:]] == [0, 0]
    assert kmers.ChainCigars._fields == ("offsets", "ops", "ins", "dels")
    assert list(inspect.signature(kh.cigar_string).parameters) == ["cigars", "table", "row", "k"]
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        p = inspect.signature(cls.chain_cigars).parameters
        assert list(p)[:6] == ["self", "seq", "ref_text", "read_starts", "ref_base", "max_edits"]
        assert [p[n].default for n in ("read_starts", "ref_base", "max_edits")] == [None, 0, 31]
    assert kh.WideKmerPositionIndex.chain_cigars is kh.KmerPositionIndex.chain_cigars


def test_python_refusals_and_cigar_string_need_no_device():
    import kmerhash_amd as kh
    from kmerhash_amd.index import ChainTable
    t = b"ACGT" * 8
    q, r, v = np.arange(8, dtype=np.uint32), np.arange(8, dtype=np.uint32), np.zeros(8, dtype=np.uint8)
    pred, chain, link = np.arange(-1, 7, dtype=np.int32), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
    for kw in (dict(k=0), dict(k=65), dict(k=4, n_chains=-1), dict(k=4, ref_base=-1), dict(k=4, ref_base=2 ** 31)):
        with pytest.raises(ValueError):
            kh.chain_cigars(t, t, q, r, v, pred, chain, link=link, **dict(dict(n_chains=1), **kw))
    with pytest.raises(ValueError, match="one entry per anchor"):
        kh.chain_cigars(t, t, q, r, v, pred, chain, 1, 4, link[:7])
    # no anchors: no device needed, outputs of the documented types
    e, e8, ei = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.int32)
    c = kh.chain_cigars(b"", b"", e, e, e8, ei, ei, 3, 4, ei)
    assert c.offsets.tolist() == [0] and len(c.ops) == 0 and c.ins.tolist() == [0, 0, 0] and c.dels.tolist() == [0, 0, 0]
    assert [x.dtype for x in c] == [np.uint64, np.uint32, np.uint32, np.uint32]
    # chain_cigars() asks for a stranded index before anything else
    ix = kh.KmerPositionIndex.__new__(kh.KmerPositionIndex)
    ix.stranded = False
    with pytest.raises(ValueError, match="stranded=True"):
        ix.chain_cigars(b"ACGT", b"ACGT")
    # cigar_string: rows in ascending anchor order, k '=' for the last seed, equal neighbours merged; None over an empty link row
    run = lambda n, op: (n << 4) | op          # noqa: E731
    cig = kh.kmers.ChainCigars(np.array([0, 0, 2, 2, 3, 6, 6], dtype=np.uint64),
                               np.array([run(3, 7), run(1, 8), run(9, 7), run(2, 1), run(1, 2), run(4, 7)], dtype=np.uint32), None, None)
    table = ChainTable(*[None] * 9, np.array([0, 0, 1, 1, 0, -1], dtype=np.int32))
    assert kh.cigar_string(cig, table, 0, 5) == "3=1X2I1D9="          # anchors 0, 1, 4: 3=1X, then 2I1D4=, then 5=
    assert kh.cigar_string(cig, table, 1, 5) == "14="                 # anchors 2, 3: 9=, then 5=
    cig2 = cig._replace(offsets=np.array([0, 0, 2, 2, 3, 3, 3], dtype=np.uint64))
    assert kh.cigar_string(cig2, table, 0, 5) is None
    with pytest.raises(ValueError):
        kh.cigar_string(cig, table, 2, 5)
