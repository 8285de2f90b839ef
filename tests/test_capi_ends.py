"""CPU: kh_chain_ends is declared with the documented parameter list, bound with matching argtypes and exported; the header stays C;
every refusal the header lists comes back as KH_ERR_INVALID before a device is touched (this test runs without one) and leaves the
outputs alone; no chains in host memory is KH_OK with offsets[0] = 0; the Python surface exists with its defaults, and read_cigar and
extended_intervals put the ends onto a table."""
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
    m = re.search(r"kh_status\s+kh_chain_ends\s*\(([^)]*)\)\s*;", txt)
    assert m, "kh_chain_ends is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert params == ["const void* qtext", "uint64_t nq", "const void* rtext", "uint64_t nr", "uint32_t ref_base", "const uint32_t* qpos",
                      "const uint32_t* rpos", "const uint8_t* rev", "uint64_t m", "const uint32_t* c_first", "const uint32_t* c_last",
                      "const uint32_t* q_lo", "const uint32_t* q_hi", "uint64_t n_chains", "uint32_t k", "uint32_t max_edits", "uint32_t clip_cost",
                      "kh_mem where", "uint32_t* e_q", "uint32_t* e_r", "uint32_t* e_edits", "uint32_t* e_clip", "uint64_t* out_offsets",
                      "uint32_t* out_ops", "uint64_t cap_ops", "uint64_t* n_ops", "int device", "void* hip_stream"]
    assert txt.index("kh_chain_cigars") < txt.index("kh_chain_ends")
    # the definition stands in the header in full
    for phrase in ("row 2c is its HEAD", "read DOWNWARDS", "Which rows are looked at", "S(e, d) = F_e[d] - clip_cost * e", "then to d < 0", "READ order"):
        assert phrase in raw, phrase
    assert "kh_chain_ends" in capi.SYMBOLS
    f = capi.lib().kh_chain_ends                               # AttributeError: not exported
    vp, u64, u32, i32, pu64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)
    assert list(f.argtypes) == [vp, u64, vp, u64, u32, vp, vp, vp, u64, vp, vp, vp, vp, u64, u32, u32, u32, i32, vp, vp, vp, vp, vp, vp, u64, pu64, i32, vp]
    assert f.restype is C.c_int


def test_the_header_stays_c(capi, tmp_path):
    src = tmp_path / "use_ends.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  uint64_t n = 7, offs[1] = {7};\n'
                   '  kh_status a = kh_chain_ends(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 15, 31, 0, KH_MEM_HOST, 0, 0, 0, 0, offs, 0, 0, &n, 0, 0);\n'      # clip_cost = 0
                   '  kh_status b = kh_chain_ends(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 15, 31, 4, KH_MEM_HOST, 0, 0, 0, 0, offs, 0, 0, &n, 0, 0);\n'      # nothing to do
                   '  printf("%d %d %d %d\\n", (int)a, (int)b, (int)n, (int)offs[0]);\n  return 0;\n}\n')
    exe = tmp_path / "use_ends"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["1", "0", "0", "0"], r.stdout


def test_refusals_need_no_device(capi):
    f = capi.lib().kh_chain_ends
    m, nc = 8, 2
    qt, rt = np.frombuffer(b"ACGT" * 16, dtype=np.uint8).copy(), np.frombuffer(b"ACGT" * 16, dtype=np.uint8).copy()
    q, r, v = np.arange(m, dtype=np.uint32), np.arange(m, dtype=np.uint32), np.zeros(m, dtype=np.uint8)
    cf, cl = np.array([0, 4], dtype=np.uint32), np.array([3, 7], dtype=np.uint32)
    lo, hi = np.zeros(nc, dtype=np.uint32), np.full(nc, 64, dtype=np.uint32)
    nums = [np.full(2 * nc, 7, dtype=np.uint32) for _ in range(4)]
    offs, ops = np.full(2 * nc + 1, 7, dtype=np.uint64), np.full(64, 7, dtype=np.uint32)
    n = C.c_uint64(7)
    P = lambda a: a.ctypes.data          # noqa: E731

    def call(qt=P(qt), nq=len(qt), rt=P(rt), nr=len(rt), base=0, q=P(q), r=P(r), v=P(v), m=m, cf=P(cf), cl=P(cl), lo=P(lo), hi=P(hi), nc=nc, k=4, me=31, cc=4,
             where=capi.KH_MEM_HOST, eq=P(nums[0]), er=P(nums[1]), ee=P(nums[2]), ec=P(nums[3]), offs=P(offs), ops=P(ops), cap=64, n=C.byref(n)):
        return f(qt, nq, rt, nr, base, q, r, v, m, cf, cl, lo, hi, nc, k, me, cc, where, eq, er, ee, ec, offs, ops, cap, n, 0, None)

    bad = [dict(k=0), dict(k=65), dict(me=32), dict(cc=0), dict(cc=256), dict(m=(1 << 24) + 1), dict(m=1 << 32), dict(nc=(1 << 23) + 1), dict(nc=1 << 40),
           dict(nq=1 << 31), dict(nq=1 << 40), dict(nr=(1 << 31) + 1), dict(base=1, nr=1 << 31), dict(base=0xFFFFFFFF, nr=2), dict(base=(1 << 31) - 63),
           dict(where=7), dict(where=-1), dict(offs=None), dict(n=None), dict(cf=None), dict(cl=None), dict(lo=None), dict(hi=None),
           dict(eq=None), dict(er=None), dict(ee=None), dict(ec=None), dict(qt=None), dict(rt=None), dict(q=None), dict(r=None), dict(v=None)]
    for where in (capi.KH_MEM_HOST, capi.KH_MEM_DEVICE):
        for kw in bad:
            assert call(**dict(dict(where=where), **kw)) == capi.KH_ERR_INVALID, kw
        # the parameters are checked for an empty chain list too
        for kw in (dict(k=0), dict(me=32), dict(cc=0), dict(cc=256), dict(nq=1 << 31), dict(base=1, nr=1 << 31), dict(where=7), dict(offs=None), dict(n=None)):
            assert call(**dict(dict(nc=0, where=where), **kw)) == capi.KH_ERR_INVALID, kw
    for a in nums + [offs, ops]:
        assert (a == 7).all()                                    # refused before anything is written
    assert n.value == 7
    # host memory, no chains: offsets[0] = 0 and no runs are the whole effect of the call; every array may be null then
    assert call(nc=0, qt=None, nq=0, rt=None, nr=0, q=None, r=None, v=None, m=0, cf=None, cl=None, lo=None, hi=None, eq=None, er=None, ee=None, ec=None,
                ops=None, cap=0) == capi.KH_OK
    assert n.value == 0 and offs[0] == 0 and (offs[1:] == 7).all() and (ops == 7).all() and all((a == 7).all() for a in nums)


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import kmers
    for name in ("chain_ends", "read_cigar", "extended_intervals"):
        assert getattr(kh, name) is getattr(kmers, name) and name in kh.__all__
    p = inspect.signature(kh.chain_ends).parameters
    assert list(p) == ["qtext", "rtext", "qpos", "rpos", "rev", "first", "last", "q_lo", "q_hi", "k", "ref_base", "max_edits", "clip_cost", "device"]
    assert [p[n].default for n in list(p)[10:]] == [0, 31, 4, 0]
    assert kmers.ChainEnds._fields == ("q", "r", "edits", "clip", "offsets", "ops")
    assert list(inspect.signature(kh.read_cigar).parameters) == ["cigars", "ends", "table", "row", "k"]
    assert list(inspect.signature(kh.extended_intervals).parameters) == ["table", "ends"]
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        p = inspect.signature(cls.chain_ends).parameters
        assert list(p)[:8] == ["self", "seq", "ref_text", "read_starts", "read_ends", "ref_base", "max_edits", "clip_cost"]
        assert [p[n].default for n in ("read_starts", "read_ends", "ref_base", "max_edits", "clip_cost")] == [None, None, 0, 31, 4]
    assert kh.WideKmerPositionIndex.chain_ends is kh.KmerPositionIndex.chain_ends


def test_python_refusals_and_the_host_helpers_need_no_device():
    import kmerhash_amd as kh
    from kmerhash_amd.index import ChainTable
    t = b"ACGT" * 8
    q, r, v = np.arange(8, dtype=np.uint32), np.arange(8, dtype=np.uint32), np.zeros(8, dtype=np.uint8)
    cf, cl, lo, hi = (np.array(x, dtype=np.uint32) for x in ([0], [7], [0], [32]))
    for kw in (dict(k=0), dict(k=65), dict(max_edits=32), dict(max_edits=-1), dict(clip_cost=0), dict(clip_cost=256), dict(ref_base=-1), dict(ref_base=2 ** 31)):
        with pytest.raises(ValueError):
            kh.chain_ends(t, t, q, r, v, cf, cl, lo, hi, **dict(dict(k=4), **kw))
    with pytest.raises(ValueError, match="one entry per chain"):
        kh.chain_ends(t, t, q, r, v, cf, cl, lo, hi[:0], 4)
    with pytest.raises(ValueError, match="one entry per anchor"):
        kh.chain_ends(t, t, q, r, v[:7], cf, cl, lo, hi, 4)
    # no chains: no device needed, outputs of the documented types
    e = np.zeros(0, dtype=np.uint32)
    c = kh.chain_ends(t, t, q, r, v, e, e, e, e, 4)
    assert c.offsets.tolist() == [0] and all(len(x) == 0 for x in (c.q, c.r, c.edits, c.clip, c.ops))
    assert [x.dtype for x in c] == [np.uint32] * 4 + [np.uint64, np.uint32]
    ix = kh.KmerPositionIndex.__new__(kh.KmerPositionIndex)
    ix.stranded = False
    with pytest.raises(ValueError, match="stranded=True"):
        ix.chain_ends(b"ACGT", b"ACGT")
    # read_cigar: S, head row, the chain's own CIGAR, tail row, S -- equal neighbours merged, zero clips dropped
    run = lambda n, op: (n << 4) | op          # noqa: E731
    cig = kh.kmers.ChainCigars(np.array([0, 0, 2, 2, 3], dtype=np.uint64), np.array([run(3, 7), run(1, 8), run(9, 7)], dtype=np.uint32), None, None)
    table = ChainTable(np.array([0, 0]), np.array([0, 1], dtype=np.uint8), np.array([10, 40], dtype=np.uint32), np.array([30, 60], dtype=np.uint32),
                       np.array([110, 240], dtype=np.uint32), np.array([130, 260], dtype=np.uint32), None, None, None, np.array([0, 0, 1, 1], dtype=np.int32))
    ends = kh.kmers.ChainEnds(np.array([5, 6, 0, 4], dtype=np.uint32), np.array([6, 6, 0, 3], dtype=np.uint32), np.array([1, 0, 0, 1], dtype=np.uint32),
                              np.array([2, 0, 7, 0], dtype=np.uint32), np.array([0, 2, 3, 3, 5], dtype=np.uint64),
                              np.array([run(1, 2), run(5, 7), run(6, 7), run(1, 1), run(3, 7)], dtype=np.uint32))
    assert kh.read_cigar(cig, ends, table, 0, 5) == "2S1D8=1X11="          # 2S | 1D5= | 3=1X + 5= | 6=
    assert kh.read_cigar(cig, ends, table, 1, 5) == "7S14=1I3="            # 7S | (empty) | 9= + 5= | 1I3=
    assert kh.read_cigar(cig._replace(offsets=np.array([0, 0, 0, 0, 0], dtype=np.uint64)), ends, table, 0, 5) is None
    # extended_intervals: forward, the head moves the starts and the tail the ends; reverse, the head extends r_end and the tail r_start
    q0, q1, r0, r1 = kh.extended_intervals(table, ends)
    assert (q0.tolist(), q1.tolist(), r0.tolist(), r1.tolist()) == ([5, 40], [36, 64], [104, 237], [136, 260])
