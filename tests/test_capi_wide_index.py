"""CPU: the position index over 16-byte k-mers (kh_wide_index_*) and its position-keeping front end (kh_kmers128_from_*_pos) are
declared, bound and exported; without a GPU the index fails loudly; arguments that cannot be served are refused before anything is
touched; and the numpy model the GPU tests compare against (tests/wide_index_model.py) is right on an example checked by hand."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from wide_index_model import WideIndexModel, kmers128_pos_model, pack_window128, split128  # noqa: E402

INDEX = ["create", "destroy", "set_stream", "last_error", "clear", "build", "build_from_sequence", "build_from_fastq", "size", "total",
         "capacity", "export", "count", "find", "profile_enable", "profile_dump"]
NEW = ["kh_kmers128_from_sequence_pos", "kh_kmers128_from_fastq_pos", "kh_wide_index_export_info"] + ["kh_wide_index_" + s for s in INDEX]


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def test_wide_index_symbols_declared_bound_and_exported(capi):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read(), flags=re.S)
    L = capi.lib()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared" % s
        assert s in capi.SYMBOLS
        f = getattr(L, s)                                   # AttributeError: not exported
        assert f.argtypes, s
    # one contract, two key widths: the argument lists are those of kh_index_*
    for s in INDEX:
        assert list(getattr(L, "kh_wide_index_" + s).argtypes) == list(getattr(L, "kh_index_" + s).argtypes), s
    assert list(L.kh_kmers128_from_sequence_pos.argtypes) == list(L.kh_kmers_from_sequence_pos.argtypes)
    assert list(L.kh_kmers128_from_fastq_pos.argtypes) == list(L.kh_kmers_from_fastq_pos.argtypes)
    assert L.kh_wide_index_last_error.restype is C.c_char_p
    assert L.kh_wide_index_last_error(None) == b"null index"


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import wide
    import inspect
    assert "WideKmerPositionIndex" in kh.__all__
    for m in ("build", "build_sequences", "build_fastq", "clear", "close", "size", "total", "capacity", "export", "count", "find",
              "profile_enable", "profile"):
        assert callable(getattr(kh.WideKmerPositionIndex, m, None)), m
    assert {"positions", "cap_out"} <= set(inspect.signature(kh.WideKmerPositionIndex.find).parameters)
    assert inspect.signature(kh.WideKmerPositionIndex.__init__).parameters["k"].default == 63
    for k in (0, 65):
        with pytest.raises(ValueError):
            kh.WideKmerPositionIndex(k=k)
    with pytest.raises(ValueError):
        kh.KmerPositionIndex(k=33)                          # the 64-bit index keeps its range
    for f in (wide.kmers128_from_sequence, wide.kmers128_from_fastq):
        assert inspect.signature(f).parameters["with_positions"].default is False


def test_no_wide_index_without_gpu(capi):
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("GPU present")
    except ImportError:
        pass
    h = C.c_void_p(1)
    assert capi.lib().kh_wide_index_create(C.byref(h), 3, 43, 0.35, 0.8, 0) == capi.KH_ERR_HIP and not h.value
    import kmerhash_amd as kh
    with pytest.raises(kh.KhError):
        kh.WideKmerPositionIndex()


def test_oversize_and_null_arguments_are_refused_before_anything_is_touched(capi):
    L = capi.lib()
    n_out = C.c_uint64(7)
    # 2^32 bytes of text cannot be addressed by 32-bit positions: refused with null buffers, nothing is read
    for fn in (L.kh_kmers128_from_sequence_pos, L.kh_kmers128_from_fastq_pos):
        assert fn(None, 1 << 32, 63, 1, capi.KH_MEM_HOST, None, None, C.byref(n_out), 0, None) == capi.KH_ERR_INVALID
        assert n_out.value == 0
        n_out.value = 7
    # no handle can exist without a GPU: the null-handle form
    assert L.kh_wide_index_build(None, None, None, 1 << 32, capi.KH_MEM_HOST) == capi.KH_ERR_INVALID
    assert L.kh_wide_index_build_from_sequence(None, None, 1 << 32, 63, 1, capi.KH_MEM_HOST) == capi.KH_ERR_INVALID
    assert L.kh_wide_index_build_from_fastq(None, None, 1 << 32, 63, 1, capi.KH_MEM_HOST) == capi.KH_ERR_INVALID
    assert L.kh_wide_index_find(None, None, 0, capi.KH_MEM_HOST, None, None, 0, C.byref(n_out)) == capi.KH_ERR_INVALID
    assert n_out.value == 0
    assert L.kh_wide_index_count(None, None, 0, capi.KH_MEM_HOST, None) == capi.KH_ERR_INVALID
    assert L.kh_wide_index_clear(None) == capi.KH_ERR_INVALID
    assert L.kh_wide_index_size(None, C.byref(n_out)) == capi.KH_ERR_INVALID
    assert L.kh_wide_index_profile_enable(None, 1) == capi.KH_ERR_INVALID
    assert L.kh_wide_index_export_info(None, None) == capi.KH_ERR_INVALID
    assert L.kh_wide_index_destroy(None) == capi.KH_OK


def test_model_on_a_hand_written_example():
    # keys A = (7, 0), B = (7, 1) differ in w1 only; C = (3, 1) is below B and above A as a 128-bit value; D = (9, 0)
    A, B, Cc, D = (7, 0), (7, 1), (3, 1), (9, 0)
    keys = np.array([B, A, B, D, A, Cc, B, A], dtype=np.uint64)
    pos = np.array([50, 10, 20, 5, 10, 8, 40, 2], dtype=np.uint32)
    m = WideIndexModel(keys, pos)
    assert m.size() == 4 and m.total() == 8
    assert m.keys.tolist() == [[7, 0], [9, 0], [3, 1], [7, 1]]                  # ascending by (w1, w0)
    assert m.offsets.tolist() == [0, 3, 4, 5, 8]
    assert m.positions.tolist() == [2, 10, 10, 5, 8, 20, 40, 50]               # the duplicate (A, 10) kept
    q = np.array([B, (7, 2), A, D, B], dtype=np.uint64)
    assert m.count(q).tolist() == [3, 0, 3, 1, 3]
    offs, p = m.find(q)
    assert offs.tolist() == [0, 3, 3, 6, 7, 10]
    assert p.tolist() == [20, 40, 50, 2, 10, 10, 5, 20, 40, 50]
    offs, p = m.find(np.zeros((0, 2), dtype=np.uint64))
    assert offs.tolist() == [0] and len(p) == 0
    o, p = m.export_in_key_order(np.array([D, B, A, Cc], dtype=np.uint64))
    assert o.tolist() == [0, 1, 4, 7, 8] and p.tolist() == [5, 20, 40, 50, 2, 10, 10, 8]
    sh = np.random.default_rng(1).permutation(8)
    m2 = WideIndexModel(keys[sh], pos[sh])
    assert np.array_equal(m2.keys, m.keys) and np.array_equal(m2.offsets, m.offsets) and np.array_equal(m2.positions, m.positions)


def test_model_window_of_k_40_packed_by_hand():
    # 40 bases: seven A and a C (the 16 bits above w0: 0b01), then 32 bases that fill w0
    text = np.frombuffer(b"NAAAAAAAC" + b"G" * 31 + b"T" + b"N", dtype=np.uint8)
    # forward: A x7 C | G x31 T  ->  V = (1 << 64) | w0 with w0 = GG..GT = 0b10 x31, 0b11
    w0 = int("10" * 31 + "11", 2)
    assert pack_window128(text, 1, 40, False) == (w0, 1)
    assert split128((1 << 64) | w0) == (w0, 1)
    # reverse complement: A C x31 G T x7 = 00 (01)x31 10 (11)x7 (80 bits); it starts with A as the forward does and then has C where the
    # forward has A, so the forward is the smaller: canonical = forward
    rc = int("00" + "01" * 31 + "10" + "11" * 7, 2)
    assert rc > ((1 << 64) | w0)
    assert pack_window128(text, 1, 40, True) == (w0, 1)
    km, pos = kmers128_pos_model(text, 40, True)
    assert pos.tolist() == [1] and km.tolist() == [[w0, 1]]
    # a window whose canonical form is the reverse complement: T x40 -> A x40 = 0
    t = np.frombuffer(b"T" * 41, dtype=np.uint8)
    km, pos = kmers128_pos_model(t, 40, True)
    assert pos.tolist() == [0, 1] and km.tolist() == [[0, 0], [0, 0]]
    km, _ = kmers128_pos_model(t, 40, False)
    assert km.tolist() == [[(1 << 64) - 1, (1 << 16) - 1]] * 2
