"""CPU: kh_chain_records and kh_cigar_text are declared, bound with matching argtypes and exported; the header holds the definition;
every refusal the header lists comes back as KH_ERR_INVALID before a device is touched (this test runs without one) and leaves the
outputs alone; no chains, and no rows or runs, in host memory are KH_OK without a device; the Python surface exists with its defaults."""
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


def test_symbols_declared_bound_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"kh_status\s+kh_chain_records\s*\(([^)]*)\)\s*;", txt)
    assert m, "kh_chain_records is not declared"
    names = [re.sub(r"\s+", " ", p).strip().split(" ")[-1] for p in m.group(1).split(",")]
    assert names == ["qpos", "rpos", "rev", "chain", "m", "lk_offsets", "lk_ops", "n_lk", "c_first", "c_last", "q_lo", "q_hi", "n_chains", "e_q", "e_r", "e_clip", "en_offsets",
                     "en_ops", "n_en", "k", "ref_order", "where", "out_valid", "out_qs", "out_qe", "out_rs", "out_re", "out_qlen", "out_match", "out_block", "out_nm",
                     "out_offsets", "out_ops", "cap_ops", "n_ops", "device", "hip_stream"]
    m = re.search(r"kh_status\s+kh_cigar_text\s*\(([^)]*)\)\s*;", txt)
    assert m and [re.sub(r"\s+", " ", p).strip().split(" ")[-1] for p in m.group(1).split(",")] == [
        "offsets", "n_rows", "ops", "n_ops", "where", "out_offsets", "out_text", "cap_text", "n_text", "device", "hip_stream"]
    assert txt.index("kh_chain_select") < txt.index("kh_chain_records") < txt.index("kh_cigar_text")
    for phrase in ("Members.", "Validity.", "a run of length 0 vanishes", "mod 2^28", "head and\n *      tail swap sides", "b - a > 63", "\"MIDNSHP=X\"", "base = o(0)"):
        assert phrase in raw, phrase
    vp, u64, u32, i32, pu64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)
    assert "kh_chain_records" in capi.SYMBOLS and "kh_cigar_text" in capi.SYMBOLS
    f, g = capi.lib().kh_chain_records, capi.lib().kh_cigar_text
    assert list(f.argtypes) == [vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, u32, u32, i32] + [vp] * 11 + [u64, pu64, i32, vp]
    assert list(g.argtypes) == [vp, u64, vp, u64, i32, vp, vp, u64, pu64, i32, vp]
    assert f.restype is C.c_int and g.restype is C.c_int


def records_args(**over):
    m, nc = 8, 2
    a = dict(qpos=np.arange(m, dtype=np.uint32), rpos=np.arange(m, dtype=np.uint32), rev=np.zeros(m, dtype=np.uint8), chain=np.zeros(m, dtype=np.int32), m=m,
             lk_offsets=np.zeros(m + 1, dtype=np.uint64), lk_ops=np.zeros(4, dtype=np.uint32), n_lk=4, c_first=np.zeros(nc, dtype=np.uint32),
             c_last=np.zeros(nc, dtype=np.uint32), q_lo=np.zeros(nc, dtype=np.uint32), q_hi=np.full(nc, 64, dtype=np.uint32), n_chains=nc,
             e_q=np.zeros(2 * nc, dtype=np.uint32), e_r=np.zeros(2 * nc, dtype=np.uint32), e_clip=np.zeros(2 * nc, dtype=np.uint32),
             en_offsets=np.zeros(2 * nc + 1, dtype=np.uint64), en_ops=np.zeros(4, dtype=np.uint32), n_en=4, k=15, ref_order=0, where=0,
             out_valid=np.full(nc, 7, dtype=np.uint8), **{"out_" + n: np.full(nc, 7, dtype=np.uint32) for n in "qs qe rs re qlen match block nm".split()},
             out_offsets=np.full(nc + 1, 7, dtype=np.uint64), out_ops=np.full(8, 7, dtype=np.uint32), cap_ops=8)
    a.update(over)
    return a


def call_records(capi, a):
    n = C.c_uint64(77)
    vals = [(v.ctypes.data if isinstance(v, np.ndarray) else v) for v in a.values()]
    st = capi.lib().kh_chain_records(*vals, C.byref(n) if a.get("_n", True) else None, 0, None)
    return st, n.value


REFUSALS = [dict(k=0), dict(k=65), dict(ref_order=2), dict(m=2 ** 24 + 1), dict(n_chains=2 ** 23 + 1), dict(n_lk=2 ** 31 + 1), dict(n_en=2 ** 31 + 1), dict(where=2), dict(where=-1),
            dict(out_offsets=None)] + [{f: None} for f in ("c_first", "c_last", "q_lo", "q_hi", "e_q", "e_r", "e_clip", "en_offsets", "en_ops", "out_valid", "out_qs", "out_qe",
                                                           "out_rs", "out_re", "out_qlen", "out_match", "out_block", "out_nm", "qpos", "rpos", "rev", "chain", "lk_offsets", "lk_ops")]


@pytest.mark.parametrize("over", REFUSALS, ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_records_refusals_need_no_device(capi, over):
    a = records_args(**over)
    st, n = call_records(capi, a)
    assert (st, n) == (capi.KH_ERR_INVALID, 77)                       # *n_ops is not touched either
    for key, v in a.items():
        if key.startswith("out_") and isinstance(v, np.ndarray):
            assert (v == 7).all(), key


def test_records_null_n_ops_and_no_chains(capi):
    a = records_args()
    vals = [(v.ctypes.data if isinstance(v, np.ndarray) else v) for v in a.values()]
    assert capi.lib().kh_chain_records(*vals, None, 0, None) == capi.KH_ERR_INVALID
    # no chains in host memory: nothing needs a device, null arrays are fine
    a = records_args(n_chains=0, **{f: None for f in ("c_first", "c_last", "q_lo", "q_hi", "e_q", "e_r", "e_clip", "en_offsets", "en_ops", "out_valid", "out_qs", "out_ops")}, n_en=0)
    st, n = call_records(capi, a)
    assert (st, n) == (capi.KH_OK, 0) and a["out_offsets"][0] == 0 and a["out_offsets"][1] == 7


def test_text_refusals_and_empty_inputs_need_no_device(capi):
    f = capi.lib().kh_cigar_text
    offs, ops = np.array([0, 2, 4], dtype=np.uint64), np.arange(4, dtype=np.uint32)
    out, text = np.full(3, 7, dtype=np.uint64), np.full(8, 7, dtype=np.uint8)
    n = C.c_uint64(77)
    p = lambda x: x.ctypes.data      # noqa: E731
    bad = [(p(offs), 2 ** 31 + 1, p(ops), 4, 0, p(out)), (p(offs), 2, p(ops), 2 ** 31 + 1, 0, p(out)), (p(offs), 2, p(ops), 4, 2, p(out)), (p(offs), 2, p(ops), 4, 0, None),
           (None, 2, p(ops), 4, 0, p(out)), (p(offs), 2, None, 4, 0, p(out))]
    for args in bad:
        assert f(*args, p(text), 8, C.byref(n), 0, None) == capi.KH_ERR_INVALID and n.value == 77
    assert f(p(offs), 2, p(ops), 4, 0, p(out), p(text), 8, None, 0, None) == capi.KH_ERR_INVALID
    assert (out == 7).all() and (text == 7).all()
    assert f(p(offs), 2, None, 0, 0, p(out), None, 0, C.byref(n), 0, None) == capi.KH_OK and n.value == 0 and (out == 0).all()      # no runs
    out[:] = 7
    assert f(None, 0, p(ops), 4, 0, p(out), None, 0, C.byref(n), 0, None) == capi.KH_OK and out[0] == 0 and out[1] == 7           # no rows


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import kmers
    sig = inspect.signature(kh.chain_records)
    assert list(sig.parameters) == ["qpos", "rpos", "rev", "chain", "cigars", "first", "last", "q_lo", "q_hi", "ends", "k", "ref_order", "device"]
    assert sig.parameters["ref_order"].default is False and sig.parameters["device"].default == 0
    assert list(inspect.signature(kh.cigar_text).parameters) == ["offsets", "ops", "device"]
    assert kh.ChainRecords._fields == ("valid", "qs", "qe", "rs", "re", "qlen", "n_match", "n_block", "nm", "offsets", "ops")
    assert kh.Mapping._fields == ("table", "edits", "cigars", "ends", "select", "records")
    wp = inspect.signature(kh.write_paf).parameters
    assert list(wp)[:8] == ["fh", "mapping", "read_names", "ref_name", "ref_len", "k", "ref_start", "kept_only"] and wp["ref_start"].default == 0 and wp["kept_only"].default is True
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        mp = inspect.signature(cls.map).parameters
        assert list(mp)[:12] == ["self", "seq", "ref_text", "read_starts", "read_ends", "ref_base", "max_edits", "clip_cost", "mask_pct", "pri_pct", "best_n", "ref_order"]
        assert (mp["max_edits"].default, mp["clip_cost"].default, mp["mask_pct"].default, mp["pri_pct"].default, mp["best_n"].default, mp["ref_order"].default) == (31, 4, 50, 80, 5, True)
    with pytest.raises(ValueError, match="k must be"):
        kmers.chain_records([], [], [], [], kmers.ChainCigars([0], [], [], []), [], [], [], [], kmers.ChainEnds([], [], [], [], [0], []), 0)
    # no chains, no rows: answered without the library's device path
    rec = kmers.chain_records([], [], [], [], kmers.ChainCigars([0], [], [], []), [], [], [], [], kmers.ChainEnds([], [], [], [], [0], []), 15)
    assert list(rec.offsets) == [0] and len(rec.ops) == 0 and len(rec.valid) == 0
    toff, text = kmers.cigar_text(np.zeros(3, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    assert list(toff) == [0, 0, 0] and len(text) == 0
