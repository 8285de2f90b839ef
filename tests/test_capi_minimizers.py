"""CPU: the minimizer entry points (kh_minimizers_from_sequence / _fastq, kh_index_build_from_minimizers / _append_from_minimizers) are
declared, bound and exported; every refusal the header lists comes back as KH_ERR_INVALID before a device is touched (this test runs
without one); the Python surface exists; and the header with the new section still compiles as C."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kh_minimizers_from_sequence", "kh_minimizers_from_fastq", "kh_index_build_from_minimizers", "kh_index_append_from_minimizers"]


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def test_symbols_declared_bound_and_exported(capi):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read(), flags=re.S)
    L = capi.lib()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, txt), "%s is not declared" % s
        assert s in capi.SYMBOLS
        f = getattr(L, s)                                   # AttributeError: not exported
        assert f.argtypes, s
        assert f.restype is C.c_int
    assert list(L.kh_minimizers_from_fastq.argtypes) == list(L.kh_minimizers_from_sequence.argtypes)
    assert len(L.kh_minimizers_from_sequence.argtypes) == 14
    assert list(L.kh_index_append_from_minimizers.argtypes) == list(L.kh_index_build_from_minimizers.argtypes) + [C.c_uint32]


@pytest.mark.parametrize("fn", NEW[:2])
def test_refusals_need_no_device(capi, fn):
    f = getattr(capi.lib(), fn)
    text = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT", dtype=np.uint8).copy()
    km, pos = np.full(64, 7, dtype=np.uint64), np.full(64, 9, dtype=np.uint32)
    H, INV = capi.KH_MEM_HOST, capi.KH_ERR_INVALID

    def call(n=len(text), k=5, w=4, hash_=2, ptr=text.ctypes.data, n_out=True):
        out = C.c_uint64(123)
        st = f(ptr, n, k, w, 1, hash_, 42, H, km.ctypes.data, pos.ctypes.data, 64, C.byref(out) if n_out else None, 0, None)
        return st, out.value

    for kw in (dict(k=0), dict(k=33), dict(w=0), dict(w=257), dict(n=1 << 32), dict(n=(1 << 32) + 5), dict(hash_=4), dict(hash_=-1),
               dict(ptr=None)):
        assert call(**kw) == (INV, 0), kw
    assert call(n_out=False)[0] == INV
    # count-only forms are refused in the same way
    out = C.c_uint64(5)
    assert f(text.ctypes.data, len(text), 5, 300, 1, 2, 42, H, None, None, 0, C.byref(out), 0, None) == INV and out.value == 0
    # nothing to sample: KH_OK and zero, still without a device
    assert call(n=0) == (capi.KH_OK, 0)
    assert call(n=0, ptr=None) == (capi.KH_OK, 0)
    assert call(n=7) == (capi.KH_OK, 0)                     # w + k - 1 = 8 bytes are the shortest text with a pick
    assert call(n=20, k=15, w=10) == (capi.KH_OK, 0)
    assert (km == 7).all() and (pos == 9).all()


def test_index_forms_refuse_a_null_handle(capi):
    L = capi.lib()
    for n in (0, 1, 1 << 32):
        for fastq in (0, 1):
            assert L.kh_index_build_from_minimizers(None, None, n, 15, 10, 1, 2, 42, capi.KH_MEM_HOST, fastq) == capi.KH_ERR_INVALID
            assert L.kh_index_append_from_minimizers(None, None, n, 15, 10, 1, 2, 42, capi.KH_MEM_HOST, fastq, 0xFFFFFFFF) == capi.KH_ERR_INVALID


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import kmers
    for fn in (kh.minimizers_from_sequence, kh.minimizers_from_fastq):
        p = inspect.signature(fn).parameters
        assert list(p)[:7] == [list(p)[0], "k", "w", "canonical", "order_hash", "order_seed", "device"]
        assert (p["k"].default, p["w"].default, p["canonical"].default, p["order_hash"].default, p["order_seed"].default) == (15, 10, True, "murmur", 42)
    assert kh.minimizers_from_sequence is kmers.minimizers_from_sequence
    p = inspect.signature(kh.KmerPositionIndex.__init__).parameters
    assert (p["w"].default, p["order_hash"].default, p["order_seed"].default) == (None, "murmur", 42)
    assert callable(kh.KmerPositionIndex.find_sequences)
    with pytest.raises(ValueError, match="16-byte"):
        kh.WideKmerPositionIndex(k=40, w=10)
    with pytest.raises(ValueError):
        kh.KmerPositionIndex(k=15, w=257)
    with pytest.raises(ValueError):
        kh.KmerPositionIndex(k=15, w=0)


def test_header_with_the_minimizer_section_compiles_as_c99(tmp_path):
    from kmerhash_amd.build import build_library
    build_library()
    src = tmp_path / "mz.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  uint64_t n = 9; uint64_t km[8]; uint32_t pos[8];\n'
                   '  kh_status a = kh_minimizers_from_sequence("ACGTACGT", 8, 3, 300, 1, KH_HASH_MURMUR3_X64_128_H0, 42, KH_MEM_HOST, km, pos, 8, &n, 0, 0);\n'
                   '  kh_status b = kh_minimizers_from_fastq("ACGT", 4, 3, 4, 0, KH_HASH_FARM64, 1, KH_MEM_HOST, 0, 0, 0, &n, 0, 0);\n'
                   '  kh_status c = kh_index_build_from_minimizers(0, "ACGT", 4, 3, 2, 1, KH_HASH_FARM64, 1, KH_MEM_HOST, 0);\n'
                   '  kh_status d = kh_index_append_from_minimizers(0, "ACGT", 4, 3, 2, 1, KH_HASH_FARM64, 1, KH_MEM_HOST, 1, 7);\n'
                   '  printf("%d %d %d %d %d\\n", (int)a, (int)b, (int)c, (int)d, (int)n);\n  return 0;\n}\n')
    exe = tmp_path / "mz"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["1", "0", "1", "1", "0"], r.stdout      # refused, too short, null handle twice
