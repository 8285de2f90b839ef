"""CPU: kh_chain_select is declared with the documented parameter list, bound with matching argtypes and exported; the header holds the
definition and stays C; every refusal the header lists comes back as KH_ERR_INVALID before a device is touched (this test runs without
one) and leaves the outputs alone; no chains in host memory is KH_OK with best = -1; the Python surface exists with its defaults;
select_table derives the groups of a hand-made ChainTable."""
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
    m = re.search(r"kh_status\s+kh_chain_select\s*\(([^)]*)\)\s*;", txt)
    assert m, "kh_chain_select is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert params == ["const uint32_t* q_start", "const uint32_t* q_end", "const int32_t* score", "const uint32_t* count", "uint64_t n_chains",
                      "const uint64_t* offsets", "uint64_t n_grp", "uint32_t mask_pct", "uint32_t pri_pct", "uint32_t best_n", "kh_mem where",
                      "int32_t* out_parent", "uint32_t* out_rank", "uint8_t* out_mapq", "uint8_t* out_flag", "int32_t* out_sub", "uint32_t* out_nsub",
                      "int32_t* out_best", "int device", "void* hip_stream"]
    assert txt.index("kh_chain_ends") < txt.index("kh_chain_select")
    # the definition stands in the header in full
    for phrase in ("score descending, ties to the smaller chain number", "p COVERS c iff 100 * ov(c, p) >= mask_pct * min(len_c, len_p)",
                   "A secondary never covers", "min(60, floor(60 * (s_p - sub_p) * min(cnt_p, 10) * min(s_p, 100) / (1000 * s_p)))",
                   "100 * s_c >= pri_pct * s_p", "fewer than best_n secondaries of p precede c", "-1 for an empty group",
                   "mm_set_parent / mm_set_mapq", "not comparable number for number", "WITHOUT waiting for the stream",
                   "every group is clamped to [0, n_chains)", "the status is KH_OK", "no floating point"):
        assert phrase in raw, phrase
    assert "kh_chain_select" in capi.SYMBOLS
    f = capi.lib().kh_chain_select                             # AttributeError: not exported
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    assert list(f.argtypes) == [vp, vp, vp, vp, u64, vp, u64, u32, u32, u32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    assert f.restype is C.c_int


def test_the_header_stays_c(capi, tmp_path):
    src = tmp_path / "use_select.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  int32_t best[2] = {7, 7}; uint64_t offs[3] = {0, 0, 0};\n'
                   '  kh_status a = kh_chain_select(0, 0, 0, 0, 0, offs, 2, 101, 80, 5, KH_MEM_HOST, 0, 0, 0, 0, 0, 0, best, 0, 0);\n'      # mask_pct = 101
                   '  kh_status b = kh_chain_select(0, 0, 0, 0, 0, offs, 2, 50, 80, 5, KH_MEM_HOST, 0, 0, 0, 0, 0, 0, best, 0, 0);\n'       # two unmapped reads
                   '  printf("%d %d %d %d\\n", (int)a, (int)b, (int)best[0], (int)best[1]);\n  return 0;\n}\n')
    exe = tmp_path / "use_select"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["1", "0", "-1", "-1"], r.stdout


def test_refusals_need_no_device(capi):
    f = capi.lib().kh_chain_select
    n, ng = 6, 3
    qs, qe = np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32) + 50
    sc, cn = np.arange(n, dtype=np.int32), np.full(n, 4, dtype=np.uint32)
    offs = np.array([0, 2, 2, 6], dtype=np.uint64)
    outs = [np.full(n, 7, dtype=dt) for dt in (np.int32, np.uint32, np.uint8, np.uint8, np.int32, np.uint32)]
    best = np.full(ng, 7, dtype=np.int32)
    P = lambda a: a.ctypes.data          # noqa: E731

    def call(qs=P(qs), qe=P(qe), sc=P(sc), cn=P(cn), n=n, offs=P(offs), ng=ng, mask=50, pri=80, bn=5, where=capi.KH_MEM_HOST, o0=P(outs[0]), o1=P(outs[1]),
             o2=P(outs[2]), o3=P(outs[3]), o4=P(outs[4]), o5=P(outs[5]), best=P(best)):
        return f(qs, qe, sc, cn, n, offs, ng, mask, pri, bn, where, o0, o1, o2, o3, o4, o5, best, 0, None)

    bad = [dict(mask=101), dict(mask=0xFFFFFFFF), dict(pri=101), dict(pri=1 << 31), dict(n=(1 << 23) + 1), dict(n=1 << 40), dict(ng=n + (1 << 24) + 1),
           dict(ng=1 << 50), dict(ng=0), dict(where=7), dict(where=-1), dict(qs=None), dict(qe=None), dict(sc=None), dict(cn=None),
           dict(o0=None), dict(o1=None), dict(o2=None), dict(o3=None), dict(o4=None), dict(o5=None)]
    for where in (capi.KH_MEM_HOST, capi.KH_MEM_DEVICE):
        for kw in bad:
            assert call(**dict(dict(where=where), **kw)) == capi.KH_ERR_INVALID, (where, kw)
        # the parameters are checked for an empty chain list too
        for kw in (dict(mask=101), dict(pri=101), dict(ng=(1 << 24) + 1), dict(ng=0), dict(where=7)):
            assert call(**dict(dict(n=0, where=where), **kw)) == capi.KH_ERR_INVALID, (where, kw)
    # host memory: offsets that do not ascend from 0 to n_chains are refused on the host
    for o in ([1, 2, 2, 6], [0, 2, 2, 5], [0, 2, 2, 7], [0, 3, 2, 6], [0, 7, 7, 6]):
        assert call(offs=P(np.array(o, dtype=np.uint64))) == capi.KH_ERR_INVALID, o
    assert call(n=0, offs=P(np.array([0, 0, 1, 0], dtype=np.uint64))) == capi.KH_ERR_INVALID
    for a in outs + [best]:
        assert (a == 7).all()                                    # refused before anything is written
    # host memory, no chains: best = -1 per group is the whole effect of the call; every other array may be null then
    nul = dict(qs=None, qe=None, sc=None, cn=None, n=0, o0=None, o1=None, o2=None, o3=None, o4=None, o5=None)
    assert call(offs=P(np.zeros(4, dtype=np.uint64)), **nul) == capi.KH_OK
    assert (best == -1).all() and all((a == 7).all() for a in outs)
    best[:] = 7
    assert call(offs=None, ng=0, **nul) == capi.KH_OK            # one group [0, 0)
    assert best.tolist() == [-1, 7, 7]
    assert call(offs=None, ng=0, best=None, **nul) == capi.KH_OK


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import kmers
    for name in ("select_chains", "select_table", "ChainSelect"):
        assert getattr(kh, name) is getattr(kmers, name) and name in kh.__all__
    p = inspect.signature(kh.select_chains).parameters
    assert list(p) == ["q_start", "q_end", "score", "count", "read_offsets", "mask_pct", "pri_pct", "best_n", "device"]
    assert [p[n].default for n in list(p)[4:]] == [None, 50, 80, 5, 0]
    assert kmers.ChainSelect._fields == ("parent", "rank", "mapq", "flag", "sub", "nsub", "best")
    p = inspect.signature(kh.select_table).parameters
    assert list(p) == ["table", "n_reads", "params"] and p["n_reads"].default is None and p["params"].kind is inspect.Parameter.VAR_KEYWORD
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        p = inspect.signature(cls.chain_select).parameters
        assert list(p) == ["self", "seq", "read_starts", "mask_pct", "pri_pct", "best_n", "params"]
        assert [p[n].default for n in ("read_starts", "mask_pct", "pri_pct", "best_n")] == [None, 50, 80, 5]
    assert kh.WideKmerPositionIndex.chain_select is kh.KmerPositionIndex.chain_select


def test_python_refusals_and_no_chains_need_no_device():
    import kmerhash_amd as kh
    a = np.arange(4, dtype=np.uint32)
    for kw in (dict(mask_pct=101), dict(mask_pct=-1), dict(pri_pct=101), dict(pri_pct=-1), dict(best_n=-1), dict(best_n=2 ** 32)):
        with pytest.raises(ValueError):
            kh.select_chains(a, a, a, a, **kw)
    with pytest.raises(ValueError, match="one entry per chain"):
        kh.select_chains(a, a, a[:3], a)
    with pytest.raises(ValueError, match="read_offsets"):
        kh.select_chains(a, a, a, a, np.zeros(1, dtype=np.uint64))
    with pytest.raises(kh.KhError):                              # host offsets that do not end at the number of chains
        kh.select_chains(a, a, a, a, np.array([0, 3], dtype=np.uint64))
    e = np.zeros(0, dtype=np.uint32)
    c = kh.select_chains(e, e, e, e)
    assert c.best.tolist() == [-1] and all(len(x) == 0 for x in c[:6])
    assert [x.dtype for x in c] == [np.int32, np.uint32, np.uint8, np.uint8, np.int32, np.uint32, np.int32]
    c = kh.select_chains(e, e, e, e, np.zeros(4, dtype=np.uint64))
    assert c.best.tolist() == [-1, -1, -1]
    ix = kh.KmerPositionIndex.__new__(kh.KmerPositionIndex)
    ix.stranded = False
    with pytest.raises(ValueError, match=r"chain_select\(\) needs an index made with stranded=True"):
        ix.chain_select(b"ACGT")


def test_select_table_derives_the_groups(monkeypatch):
    import kmerhash_amd as kh
    from kmerhash_amd import kmers
    from kmerhash_amd.index import ChainTable
    seen = {}

    def fake(q_start, q_end, score, count, read_offsets=None, **params):
        seen.update(offs=np.asarray(read_offsets), params=params, cols=(q_start, q_end, score, count))
        return "result"

    monkeypatch.setattr(kmers, "select_chains", fake)
    cols = [np.arange(5, dtype=np.uint32) + 10 * i for i in range(4)]
    table = ChainTable(np.array([1, 1, 3, 3, 3], dtype=np.uint32), None, cols[0], cols[1], None, None, cols[3], cols[2].astype(np.int32), None, None)
    assert kh.select_table(table) == "result"                   # n_reads = the last seg + 1
    assert seen["offs"].tolist() == [0, 0, 2, 2, 5] and seen["offs"].dtype == np.uint64 and seen["params"] == {}
    assert all(x is y or np.array_equal(x, y) for x, y in zip(seen["cols"], (cols[0], cols[1], cols[2], cols[3])))
    assert kh.select_table(table, 7, mask_pct=30, best_n=2) == "result"      # reads beyond the last seg: empty groups
    assert seen["offs"].tolist() == [0, 0, 2, 2, 5, 5, 5, 5] and seen["params"] == dict(mask_pct=30, best_n=2)
    with pytest.raises(ValueError, match="n_reads"):
        kh.select_table(table, 3)
    monkeypatch.undo()
    empty = ChainTable(*([np.zeros(0, dtype=np.uint32)] * 6), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int32), None, None)
    c = kh.select_table(empty)                                  # no rows, no reads: nothing at all, and no device
    assert all(len(x) == 0 for x in c)
    c = kh.select_table(empty, 3)                               # three reads without chains
    assert c.best.tolist() == [-1, -1, -1] and all(len(x) == 0 for x in c[:6])
