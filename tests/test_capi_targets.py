"""CPU: kh_anchor_targets is declared with the documented parameter list, bound with matching argtypes and exported; the header holds
the definition and stays C; every refusal the header lists comes back as KH_ERR_INVALID before a device is touched (this test runs
without one) and leaves the outputs alone; no anchors in host memory is KH_OK with one zero offset; the Python surface exists with its
defaults and refuses what it must without a device."""
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
    m = re.search(r"kh_status\s+kh_anchor_targets\s*\(([^)]*)\)\s*;", txt)
    assert m, "kh_anchor_targets is not declared"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    assert params == ["const uint32_t* qpos", "const uint32_t* rpos", "const uint8_t* rev", "uint64_t m", "const uint64_t* seg_offsets", "uint64_t n_seg",
                      "const uint32_t* t_start", "const uint32_t* t_end", "uint64_t n_t", "uint32_t k", "kh_mem where",
                      "uint32_t* out_q", "uint32_t* out_r", "uint8_t* out_v", "uint32_t* out_tid", "uint32_t* out_src",
                      "uint64_t* g_offsets", "uint32_t* g_seg", "uint32_t* g_tid", "uint64_t* n_grp", "int device", "void* hip_stream"]
    assert txt.index("kh_chain_records") < txt.index("kh_anchor_targets")
    assert re.search(r"#define\s+KH_TARGET_NONE\s+0xFFFFFFFFu", txt) and re.search(r"#define\s+KH_TARGETS_STAGED_MAX\s+8192u", txt)
    # the definition stands in the header in full
    for phrase in ("lo = 0; hi = n_t; while (lo < hi) { mid = (lo + hi) >> 1; if (t_start[mid] <= r) lo = mid + 1; else hi = mid; }",
                   "tid(i) = t iff t >= 0 and r < 2^31 and r + k <= t_end[t]", "The table\n *      is not validated", "never an access outside [0, n_t)",
                   "sorted by (segment, tid, input index)", "out_r[j] = KH_POS_INVALID where the id is KH_TARGET_NONE", "maximal runs of equal (segment, tid)",
                   "g_offsets[0] = 0 and g_offsets[*n_grp] = m", "A segment without anchors has no group", "KH_ERR_INVALID after the kernels have run",
                   "waits once, to\n *      learn *n_grp", "Integers only"):
        assert phrase in raw, phrase
    assert "kh_anchor_targets" in capi.SYMBOLS
    f = capi.lib().kh_anchor_targets                             # AttributeError: not exported
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    assert list(f.argtypes) == [vp, vp, vp, u64, vp, u64, vp, vp, u64, u32, i32] + [vp] * 8 + [C.POINTER(u64), i32, vp]
    assert f.restype is C.c_int


def test_the_header_stays_c(capi, tmp_path):
    src = tmp_path / "use_targets.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  uint64_t offs[1] = {7}, n = 7; uint32_t ts[1] = {0}, te[1] = {9};\n'
                   '  kh_status a = kh_anchor_targets(0, 0, 0, 0, 0, 0, ts, te, 1, 65, KH_MEM_HOST, 0, 0, 0, 0, 0, offs, 0, 0, &n, 0, 0);\n'      # k = 65
                   '  kh_status b = kh_anchor_targets(0, 0, 0, 0, 0, 0, ts, te, 1, 15, KH_MEM_HOST, 0, 0, 0, 0, 0, offs, 0, 0, &n, 0, 0);\n'      # no anchors
                   '  printf("%d %d %d %d %u %u\\n", (int)a, (int)b, (int)offs[0], (int)n, KH_TARGET_NONE == 0xFFFFFFFFu, KH_TARGETS_STAGED_MAX);\n  return 0;\n}\n')
    exe = tmp_path / "use_targets"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["1", "0", "0", "0", "1", "8192"], r.stdout


def test_refusals_need_no_device(capi):
    f = capi.lib().kh_anchor_targets
    m, nt, ns = 6, 2, 2
    q, r, v = np.arange(m, dtype=np.uint32), np.arange(m, dtype=np.uint32) * 10, np.zeros(m, dtype=np.uint8)
    seg = np.array([0, 2, 6], dtype=np.uint64)
    ts, te = np.array([0, 100], dtype=np.uint32), np.array([50, 150], dtype=np.uint32)
    outs = [np.full(m, 7, dtype=dt) for dt in (np.uint32, np.uint32, np.uint8, np.uint32, np.uint32)]
    goff, gseg, gtid = np.full(m + 1, 7, dtype=np.uint64), np.full(m, 7, dtype=np.uint32), np.full(m, 7, dtype=np.uint32)
    n = C.c_uint64(7)
    P = lambda a: a.ctypes.data          # noqa: E731

    def call(q=P(q), r=P(r), v=P(v), m=m, seg=P(seg), ns=ns, ts=P(ts), te=P(te), nt=nt, k=15, where=capi.KH_MEM_HOST, o0=P(outs[0]), o1=P(outs[1]), o2=P(outs[2]),
             o3=P(outs[3]), o4=P(outs[4]), goff=P(goff), gseg=P(gseg), gtid=P(gtid), n=C.byref(n)):
        return f(q, r, v, m, seg, ns, ts, te, nt, k, where, o0, o1, o2, o3, o4, goff, gseg, gtid, n, 0, None)

    bad = [dict(k=0), dict(k=65), dict(k=0xFFFFFFFF), dict(m=(1 << 24) + 1), dict(m=1 << 40), dict(nt=0), dict(nt=(1 << 24) + 1), dict(nt=1 << 50),
           dict(ns=m + (1 << 24) + 1), dict(ns=1 << 50), dict(ns=0), dict(where=7), dict(where=-1), dict(q=None), dict(r=None), dict(v=None), dict(ts=None),
           dict(te=None), dict(o0=None), dict(o1=None), dict(o2=None), dict(o3=None), dict(o4=None), dict(gseg=None), dict(gtid=None), dict(goff=None), dict(n=None)]
    for where in (capi.KH_MEM_HOST, capi.KH_MEM_DEVICE):
        for kw in bad:
            assert call(**dict(dict(where=where), **kw)) == capi.KH_ERR_INVALID, (where, kw)
        # the parameters are checked for an empty anchor list too
        for kw in (dict(k=0), dict(k=65), dict(nt=0), dict(nt=(1 << 24) + 1), dict(ns=(1 << 24) + 1), dict(where=7), dict(goff=None), dict(n=None)):
            assert call(**dict(dict(m=0, where=where), **kw)) == capi.KH_ERR_INVALID, (where, kw)
    for a in outs + [goff, gseg, gtid]:
        assert (a == 7).all()                                    # refused before anything is written
    assert n.value == 7
    # host memory, no anchors: one zero offset and no group are the whole effect of the call; every other array may be null then
    nul = dict(q=None, r=None, v=None, m=0, o0=None, o1=None, o2=None, o3=None, o4=None, gseg=None, gtid=None)
    assert call(**nul) == capi.KH_OK
    assert n.value == 0 and goff.tolist() == [0] + [7] * m
    n.value, goff[0] = 7, 7
    assert call(seg=None, ns=0, ts=None, te=None, **nul) == capi.KH_OK      # (n_t is still checked: 2)
    assert n.value == 0 and goff[0] == 0
    assert call(seg=P(np.zeros(1, dtype=np.uint64)), ns=0, **nul) == capi.KH_OK


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import kmers, targets
    for name in ("group_anchors", "AnchorGroups"):
        assert getattr(kh, name) is getattr(kmers, name) and name in kh.__all__
    assert kh.Targets is targets.Targets and "Targets" in kh.__all__ and kh.TARGET_NONE == 0xFFFFFFFF
    p = inspect.signature(kh.group_anchors).parameters
    assert list(p) == ["qpos", "rpos", "rev", "targets", "k", "seg_offsets", "device"] and [p[n].default for n in ("seg_offsets", "device")] == [None, 0]
    assert kmers.AnchorGroups._fields == ("qpos", "rpos", "rev", "tid", "src", "offsets", "seg", "target")
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        for meth in ("chains", "chain_edits", "chain_cigars", "chain_ends", "map"):
            p = inspect.signature(getattr(cls, meth)).parameters
            assert p["targets"].default is None and list(p)[-1] == "params", meth
        assert "targets=" in cls.chain_select.__doc__            # (its parameter list is pinned: the keyword travels with **params)
        p = inspect.signature(cls.anchor_groups).parameters
        assert list(p) == ["self", "seq", "read_starts", "targets"] and p["read_starts"].default is None
    assert kh.WideKmerPositionIndex.anchor_groups is kh.KmerPositionIndex.anchor_groups
    for fn in (kh.paf_lines, kh.write_paf):
        assert inspect.signature(fn).parameters["targets"].default is None


def test_python_refusals_and_no_anchors_need_no_device():
    import kmerhash_amd as kh
    a, v = np.arange(4, dtype=np.uint32), np.zeros(4, dtype=np.uint8)
    T = kh.Targets(["a", "b"], [100, 50])
    for k in (0, 65):
        with pytest.raises(ValueError, match="k must be 1..64"):
            kh.group_anchors(a, a, v, T, k)
    with pytest.raises(ValueError, match="one entry per anchor"):
        kh.group_anchors(a, a[:3], v, T, 15)
    with pytest.raises(ValueError, match="target table"):
        kh.group_anchors(a, a, v, (a[:0], a[:0]), 15)
    with pytest.raises(ValueError, match="target table"):
        kh.group_anchors(a, a, v, (a, a[:3]), 15)
    with pytest.raises(ValueError, match="seg_offsets"):
        kh.group_anchors(a, a, v, T, 15, np.zeros(1, dtype=np.uint64))
    e32, e8 = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
    g = kh.group_anchors(e32, e32, e8, T, 15, np.zeros(4, dtype=np.uint64))
    assert g.offsets.tolist() == [0] and [x.dtype for x in g] == [np.uint32, np.uint32, np.uint8, np.uint32, np.uint32, np.uint64, np.uint32, np.uint32]
    assert all(len(x) == 0 for x in g[:5] + g[6:])
    ix = kh.KmerPositionIndex.__new__(kh.KmerPositionIndex)
    ix.stranded = False
    with pytest.raises(ValueError, match=r"anchor_groups\(\) needs an index made with stranded=True"):
        ix.anchor_groups(b"ACGT", targets=T)
    # the text calls refuse a text that is not the targets', a reference base and a spacer an alignment could afford
    ix.stranded = True
    text = np.full(int(T.ends[-1]), ord("A"), dtype=np.uint8)
    for meth in ("chain_edits", "chain_cigars", "chain_ends", "map"):
        with pytest.raises(ValueError, match="ref_text must be the text the targets lay out"):
            getattr(ix, meth)(b"ACGT", text[:-1], targets=T)
        with pytest.raises(ValueError, match="ref_base must be 0"):
            getattr(ix, meth)(b"ACGT", text, ref_base=1, targets=T)
        with pytest.raises(ValueError, match="must exceed max_edits"):
            getattr(ix, meth)(b"ACGT", text, max_edits=64, targets=T)
        with pytest.raises(ValueError, match="must be a kmerhash_amd.Targets"):
            getattr(ix, meth)(b"ACGT", text, targets=(T.starts, T.ends))
