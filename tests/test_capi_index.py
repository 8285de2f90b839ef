"""CPU: the k-mer position index (kh_index_*) and the position-keeping front end (kh_kmers_from_*_pos) are declared, bound and
exported; without a GPU the index fails loudly; arguments that cannot be served are refused before anything is touched; and the numpy
model the GPU tests compare against (tests/index_model.py) is right on an example small enough to check by hand."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from index_model import IndexModel, fastq_masked, np_kmers_fastq_pos, np_kmers_pos, pack_window  # noqa: E402

NEW = ["kh_kmers_from_sequence_pos", "kh_kmers_from_fastq_pos", "kh_index_create", "kh_index_destroy", "kh_index_set_stream",
       "kh_index_last_error", "kh_index_clear", "kh_index_build", "kh_index_build_from_sequence", "kh_index_build_from_fastq",
       "kh_index_size", "kh_index_total", "kh_index_capacity", "kh_index_export", "kh_index_count", "kh_index_find"]


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def test_index_symbols_declared_bound_and_exported(capi):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read(), flags=re.S)
    L = capi.lib()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared" % s
        assert s in capi.SYMBOLS
        f = getattr(L, s)                                   # AttributeError: not exported
        assert f.argtypes, s
    assert L.kh_index_last_error.restype is C.c_char_p
    assert L.kh_index_last_error(None) == b"null index"


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd.index import SORT_TILE
    assert SORT_TILE >= 1024 and SORT_TILE & (SORT_TILE - 1) == 0
    for m in ("build", "build_sequences", "build_fastq", "count", "find", "size", "total", "capacity", "export", "clear", "close"):
        assert callable(getattr(kh.KmerPositionIndex, m, None)), m
    with pytest.raises(ValueError):
        kh.KmerPositionIndex(k=33)
    # the tile the kernels sort is the tile the Python layer (and with it the tests' shapes) names
    src = open(os.path.join(ROOT, "kmerhash_amd", "csrc", "kh_kernels_index.h")).read()
    assert int(re.search(r"#define KI_SORT_TILE (\d+)", src).group(1)) == SORT_TILE


def test_no_index_without_gpu(capi):
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("GPU present")
    except ImportError:
        pass
    h = C.c_void_p(1)
    assert capi.lib().kh_index_create(C.byref(h), 3, 43, 0.35, 0.8, 0) == capi.KH_ERR_HIP and not h.value
    import kmerhash_amd as kh
    with pytest.raises(kh.KhError):
        kh.KmerPositionIndex()


def test_oversize_and_null_arguments_are_refused_before_anything_is_touched(capi):
    L = capi.lib()
    n_out = C.c_uint64(7)
    # 2^32 bytes of text / 2^32 pairs cannot be addressed by 32-bit positions: refused with null buffers, nothing is read
    for fn in (L.kh_kmers_from_sequence_pos, L.kh_kmers_from_fastq_pos):
        assert fn(None, 1 << 32, 21, 1, capi.KH_MEM_HOST, None, None, C.byref(n_out), 0, None) == capi.KH_ERR_INVALID
        assert n_out.value == 0
        n_out.value = 7
    # no handle can exist without a GPU: the null-handle form
    assert L.kh_index_build(None, None, None, 1 << 32, capi.KH_MEM_HOST) == capi.KH_ERR_INVALID
    assert L.kh_index_build_from_sequence(None, None, 1 << 32, 21, 1, capi.KH_MEM_HOST) == capi.KH_ERR_INVALID
    assert L.kh_index_find(None, None, 0, capi.KH_MEM_HOST, None, None, 0, C.byref(n_out)) == capi.KH_ERR_INVALID
    assert n_out.value == 0
    assert L.kh_index_count(None, None, 0, capi.KH_MEM_HOST, None) == capi.KH_ERR_INVALID
    assert L.kh_index_destroy(None) == capi.KH_OK


def test_model_on_a_hand_written_example():
    #        key:  7  3  7  9  3  7  3  7  9  7
    keys = np.array([7, 3, 7, 9, 3, 7, 3, 7, 9, 7], dtype=np.uint64)
    pos = np.array([50, 10, 20, 5, 10, 40, 2, 20, 1, 30], dtype=np.uint32)
    m = IndexModel(keys, pos)
    assert m.size() == 3 and m.total() == 10
    assert m.keys.tolist() == [3, 7, 9]
    assert m.offsets.tolist() == [0, 3, 8, 10]
    assert m.positions.tolist() == [2, 10, 10, 20, 20, 30, 40, 50, 1, 5]          # duplicates (3,10) and (7,20) kept
    assert m.count(np.array([9, 4, 7, 3, 9], dtype=np.uint64)).tolist() == [2, 0, 5, 3, 2]
    offs, p = m.find(np.array([9, 4, 7, 9], dtype=np.uint64))
    assert offs.tolist() == [0, 2, 2, 7, 9]
    assert p.tolist() == [1, 5, 20, 20, 30, 40, 50, 1, 5]
    offs, p = m.find(np.zeros(0, dtype=np.uint64))
    assert offs.tolist() == [0] and len(p) == 0
    # an export whose keys come in another (slot) order
    o, p = m.export_in_key_order(np.array([9, 3, 7], dtype=np.uint64))
    assert o.tolist() == [0, 2, 5, 10] and p.tolist() == [1, 5, 2, 10, 10, 20, 20, 30, 40, 50]
    # the same multiset in another order gives the same model
    sh = np.random.default_rng(1).permutation(10)
    m2 = IndexModel(keys[sh], pos[sh])
    assert np.array_equal(m2.offsets, m.offsets) and np.array_equal(m2.positions, m.positions)


def test_model_window_positions_by_hand():
    seq = np.frombuffer(b"ACGNTTa\nGC", dtype=np.uint8)
    km, pos = np_kmers_pos(seq, 2, False)
    assert pos.tolist() == [0, 1, 4, 5, 8]                       # AC CG | TT Ta | GC
    assert km.tolist() == [0b0001, 0b0110, 0b1111, 0b1100, 0b1001]
    for p, v in zip(pos, km):
        assert pack_window(seq, int(p), 2, False) == int(v)
    km, pos = np_kmers_pos(seq, 2, True)
    assert [pack_window(seq, int(p), 2, True) for p in pos] == km.tolist()
    fq = b"@AC\nACGT\n+\nACGT\n@r2\nGG\n+\nII\n"
    a = np.frombuffer(fq, dtype=np.uint8)
    assert bytes(fastq_masked(a)) == b"\n\n\n\nACGT\n\n\n\n\n\n\n\n\n\n\n\nGG\n\n\n\n\n\n"
    km, pos = np_kmers_fastq_pos(fq, 2, False)
    assert pos.tolist() == [4, 5, 6, 20] and km.tolist() == [0b0001, 0b0110, 0b1011, 0b1010]
