"""CPU: kh_pair_chains is declared, bound with matching argtypes and exported; every refusal the header lists comes back as
KH_ERR_INVALID before a device is touched (this test runs without one) and leaves the outputs alone; no chains in host memory are
answered without a device; the Python surface exists with its signatures."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ["rs", "re", "rev", "score", "tid", "use", "mapq_in", "n_chains", "offsets", "n_reads", "min_ins", "max_ins", "unpaired_pen", "where", "out_row", "out_mapq",
         "out_tlen", "out_flag", "out_score", "out_nconc", "device", "hip_stream"]
OUTS = ("out_row", "out_mapq", "out_tlen", "out_flag", "out_score", "out_nconc")


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def test_symbol_declared_bound_and_exported(capi):
    raw = open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"kh_status\s+kh_pair_chains\s*\(([^)]*)\)\s*;", txt)
    assert m, "kh_pair_chains is not declared"
    assert [re.sub(r"\s+", " ", p).strip().split(" ")[-1].lstrip("*") for p in m.group(1).split(",")] == ORDER
    assert "kh_pair_chains" in capi.SYMBOLS and hasattr(capi.lib(), "kh_pair_chains")
    assert txt.index("kh_oriented_rows") < txt.index("kh_pair_chains") < txt.index("kh_release_cached_memory")
    assert re.search(r"#define\s+KH_PAIR_CANDIDATES\s+64u", txt)
    for phrase in ("TAKES PART", "CANDIDATE ORDER", "CONCORDANT", "PROPER", "ps* + unpaired_pen >= s_a0 + s_b0", "equal rs: mate 1 gets +t", "Corners this text decides"):
        assert phrase in raw, phrase
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    f = capi.lib().kh_pair_chains
    assert list(f.argtypes) == [vp] * 7 + [u64, vp, u64, u32, u32, u32, i32] + [vp] * 6 + [i32, vp]
    assert f.restype is C.c_int


def args(**over):
    n, n_reads = 4, 4
    a = dict(rs=np.array([10, 300, 10, 300], dtype=np.uint32), re=np.array([110, 400, 110, 400], dtype=np.uint32), rev=np.array([0, 1, 0, 1], dtype=np.uint8),
             score=np.full(n, 50, dtype=np.int32), tid=np.zeros(n, dtype=np.uint32), use=np.ones(n, dtype=np.uint8), mapq_in=np.zeros(n, dtype=np.uint8), n_chains=n,
             offsets=np.arange(n_reads + 1, dtype=np.uint64), n_reads=n_reads, min_ins=0, max_ins=1000, unpaired_pen=17, where=0,
             out_row=np.full(n_reads, 7, dtype=np.int32), out_mapq=np.full(n_reads, 7, dtype=np.uint8), out_tlen=np.full(n_reads, 7, dtype=np.int32),
             out_flag=np.full(n_reads // 2, 7, dtype=np.uint8), out_score=np.full(n_reads // 2, 7, dtype=np.int32), out_nconc=np.full(n_reads // 2, 7, dtype=np.uint32))
    a.update(over)
    return a


def call(capi, a):
    vals = [a[f].ctypes.data if isinstance(a[f], np.ndarray) else a[f] for f in ORDER[:-2]]
    return capi.lib().kh_pair_chains(*vals, 0, None)


def untouched(a):
    return all((a[f] == 7).all() for f in OUTS if isinstance(a.get(f), np.ndarray))


REFUSALS = [dict(n_reads=3), dict(n_reads=1), dict(min_ins=1001), dict(min_ins=2, max_ins=1), dict(n_chains=2 ** 23 + 1), dict(n_reads=4 + 2 ** 24 + 2), dict(where=2),
            dict(where=-1), dict(offsets=None)] + [{f: None} for f in OUTS] + [dict(rs=None), dict(re=None), dict(rev=None), dict(score=None),
            dict(offsets=np.array([1, 1, 2, 3, 4], dtype=np.uint64)), dict(offsets=np.array([0, 1, 2, 3, 5], dtype=np.uint64)),
            dict(offsets=np.array([0, 2, 1, 3, 4], dtype=np.uint64)), dict(offsets=np.array([0, 1, 2, 3, 3], dtype=np.uint64))]


@pytest.mark.parametrize("over", REFUSALS, ids=lambda o: "-".join("%s" % k for k in o))
def test_refuses_before_anything_is_touched(capi, over):
    a = args(**over)
    assert call(capi, a) == capi.KH_ERR_INVALID and untouched(a)


def test_no_reads_and_no_chains_in_host_memory_need_no_device(capi):
    a = args(n_reads=0, n_chains=0, offsets=np.zeros(1, dtype=np.uint64), rs=None, re=None, rev=None, score=None, tid=None, use=None, mapq_in=None,
             **{f: None for f in OUTS})
    assert call(capi, a) == capi.KH_OK
    a = args(n_chains=0, offsets=np.zeros(5, dtype=np.uint64), rs=None, re=None, rev=None, score=None, tid=None, use=None, mapq_in=None)
    assert call(capi, a) == capi.KH_OK
    assert (a["out_row"] == -1).all() and all((a[f] == 0).all() for f in OUTS[1:])


def test_python_surface(capi):
    import kmerhash_amd as kh
    from kmerhash_amd import kmers, sam
    assert kh.PairSelect._fields == ("row", "mapq", "tlen", "flag", "score", "nconc") and kh.PairSelect is kmers.PairSelect
    assert kh.pair_chains is kmers.pair_chains and kh.pair_mapping is kmers.pair_mapping
    assert all(n in kh.__all__ for n in ("pair_chains", "pair_mapping", "PairSelect"))
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]      # noqa: E731
    E = inspect.Parameter.empty
    assert sig(kh.pair_chains) == [("rs", E), ("re", E), ("rev", E), ("score", E), ("read_offsets", E), ("tid", None), ("use", None), ("mapq", None), ("min_ins", 0),
                                   ("max_ins", 1000), ("unpaired_pen", 17), ("device", 0)]
    assert sig(kh.pair_mapping)[:3] == [("mapping", E), ("n_reads", E), ("targets", None)]
    assert sig(sam.sam_lines)[-1] == ("pairs", None) and kh.write_sam_pairs is sam.write_sam_pairs and "write_sam_pairs" in kh.__all__
    ws, wp = sig(kh.write_sam), sig(kh.write_sam_pairs)
    assert "pairs" not in dict(ws) and wp[:3] == [("fh", E), ("mapping", E), ("pairs", E)] and wp[:2] + wp[3:] == ws      # write_sam as it was, pairs third
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        s = dict(sig(cls.map_pairs))
        assert (s["min_ins"], s["max_ins"], s["unpaired_pen"], s["targets"], s["read_ends"]) == (0, 1000, 17, None, None) and s["read_starts"] is E
    z = lambda n, dt: np.zeros(n, dtype=dt)      # noqa: E731
    # the refusals that need no call
    with pytest.raises(ValueError, match="even number of reads"):
        kh.pair_chains(z(0, np.uint32), z(0, np.uint32), z(0, np.uint8), z(0, np.int32), z(2, np.uint64))
    with pytest.raises(ValueError, match="min_ins <= max_ins"):
        kh.pair_chains(z(0, np.uint32), z(0, np.uint32), z(0, np.uint8), z(0, np.int32), z(3, np.uint64), min_ins=5, max_ins=4)
    with pytest.raises(ValueError, match="one entry per chain"):
        kh.pair_chains(z(2, np.uint32), z(2, np.uint32), z(1, np.uint8), z(2, np.int32), np.array([0, 1, 2], dtype=np.uint64))
    # no chains: answered on the host
    got = kh.pair_chains(z(0, np.uint32), z(0, np.uint32), z(0, np.uint8), z(0, np.int32), z(5, np.uint64))
    assert list(got.row) == [-1] * 4 and not got.mapq.any() and not got.tlen.any() and list(got.flag) == [0, 0] and list(got.nconc) == [0, 0]
    assert [x.dtype for x in got] == [np.int32, np.uint8, np.int32, np.uint8, np.int32, np.uint32]
