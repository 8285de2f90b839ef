"""CPU: the closed-syncmer entry points (kh_syncmers[128]_from_sequence / _fastq, kh_[wide_]syncmer_mask, kh_[wide_]index_build_from_syncmers /
_append_from_syncmers) are declared, bound and exported; every refusal the header lists comes back as KH_ERR_INVALID before a device is
touched (this test runs without one); the Python surface exists; and the header with the new section still compiles as C."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = ["kh_syncmers_from_sequence", "kh_syncmers_from_fastq", "kh_syncmers128_from_sequence", "kh_syncmers128_from_fastq"]
MASK = ["kh_syncmer_mask", "kh_wide_syncmer_mask"]
INDEX = ["kh_index_build_from_syncmers", "kh_index_append_from_syncmers", "kh_wide_index_build_from_syncmers", "kh_wide_index_append_from_syncmers"]
NEW = FRONT + MASK + INDEX


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
    for s in FRONT:
        assert list(getattr(L, s).argtypes) == list(L.kh_minimizers_from_sequence.argtypes) and len(getattr(L, s).argtypes) == 14
    assert list(L.kh_wide_syncmer_mask.argtypes) == list(L.kh_syncmer_mask.argtypes) and len(L.kh_syncmer_mask.argtypes) == 11
    for pre in ("kh_index_", "kh_wide_index_"):
        b, a = getattr(L, pre + "build_from_syncmers"), getattr(L, pre + "append_from_syncmers")
        assert list(b.argtypes) == list(L.kh_index_build_from_minimizers.argtypes) and len(b.argtypes) == 10
        assert list(a.argtypes) == list(b.argtypes) + [C.c_uint32]


@pytest.mark.parametrize("fn", FRONT)
def test_refusals_need_no_device(capi, fn):
    f = getattr(capi.lib(), fn)
    wide = "128" in fn
    kmax = 64 if wide else 32
    text = np.frombuffer(b"ACGT" * 20, dtype=np.uint8).copy()
    km, pos = np.full(256, 7, dtype=np.uint64), np.full(128, 9, dtype=np.uint32)
    H, INV = capi.KH_MEM_HOST, capi.KH_ERR_INVALID

    def call(n=len(text), k=9, s=5, hash_=2, ptr=text.ctypes.data, n_out=True, count_only=False):
        out = C.c_uint64(123)
        bufs = (None, None, 0) if count_only else (km.ctypes.data, pos.ctypes.data, 128)
        st = f(ptr, n, k, s, 1, hash_, 42, H, *bufs, C.byref(out) if n_out else None, 0, None)
        return st, out.value

    bad = [dict(s=0), dict(k=9, s=10), dict(k=kmax, s=33), dict(k=0, s=1), dict(k=0, s=0), dict(k=kmax + 1, s=kmax // 2), dict(n=1 << 32),
           dict(n=(1 << 32) + 5), dict(hash_=4), dict(hash_=-1), dict(ptr=None)]
    if wide:
        bad += [dict(k=40, s=33), dict(k=64, s=64)]
    for kw in bad:
        assert call(**kw) == (INV, 0), kw
        assert call(count_only=True, **kw) == (INV, 0), kw
    assert call(n_out=False)[0] == INV
    # nothing to sample: KH_OK and zero, still without a device
    assert call(n=0) == (capi.KH_OK, 0)
    assert call(n=0, ptr=None) == (capi.KH_OK, 0)
    assert call(n=8) == (capi.KH_OK, 0)                      # k bytes are the shortest text with a window
    assert call(n=kmax - 1, k=kmax, s=kmax // 2) == (capi.KH_OK, 0)
    assert (km == 7).all() and (pos == 9).all()


@pytest.mark.parametrize("fn", MASK)
def test_mask_refusals_need_no_device(capi, fn):
    f = getattr(capi.lib(), fn)
    kmax = 64 if "wide" in fn else 32
    keys, out = np.arange(32, dtype=np.uint64), np.full(16, 5, dtype=np.uint8)
    H, INV = capi.KH_MEM_HOST, capi.KH_ERR_INVALID

    def call(n=16, k=9, s=5, hash_=2, ptr=keys.ctypes.data, optr=out.ctypes.data):
        return f(ptr, n, k, s, 1, hash_, 42, H, optr, 0, None)

    for kw in (dict(s=0), dict(k=9, s=10), dict(k=kmax, s=33), dict(k=0, s=1), dict(k=kmax + 1, s=5), dict(n=1 << 32), dict(hash_=4), dict(hash_=-1),
               dict(ptr=None)):
        assert call(**kw) == INV, kw
    assert call(n=0) == capi.KH_OK and call(n=0, ptr=None, optr=None) == capi.KH_OK
    assert (out == 5).all()


def test_index_forms_refuse_a_null_handle(capi):
    L = capi.lib()
    for pre in ("kh_index_", "kh_wide_index_"):
        for n in (0, 1, 1 << 32):
            for fastq in (0, 1):
                assert getattr(L, pre + "build_from_syncmers")(None, None, n, 15, 11, 1, 2, 42, capi.KH_MEM_HOST, fastq) == capi.KH_ERR_INVALID
                assert getattr(L, pre + "append_from_syncmers")(None, None, n, 15, 11, 1, 2, 42, capi.KH_MEM_HOST, fastq, 0xFFFFFFFF) == capi.KH_ERR_INVALID


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import kmers, wide
    for fn, k, s in ((kh.syncmers_from_sequence, 15, 11), (kh.syncmers_from_fastq, 15, 11), (kh.is_syncmer, 15, 11),
                     (kh.syncmers128_from_sequence, 63, 31), (kh.syncmers128_from_fastq, 63, 31), (kh.is_syncmer128, 63, 31)):
        p = inspect.signature(fn).parameters
        assert list(p)[:7] == [list(p)[0], "k", "s", "canonical", "order_hash", "order_seed", "device"]
        assert (p["k"].default, p["s"].default, p["canonical"].default, p["order_hash"].default, p["order_seed"].default) == (k, s, True, "murmur", 42)
    assert kh.syncmers_from_sequence is kmers.syncmers_from_sequence and kh.is_syncmer128 is wide.is_syncmer128
    for name in ("syncmers_from_sequence", "syncmers_from_fastq", "is_syncmer", "syncmers128_from_sequence", "syncmers128_from_fastq", "is_syncmer128"):
        assert name in kh.__all__
    for cls in (kh.KmerPositionIndex, kh.WideKmerPositionIndex):
        p = inspect.signature(cls.__init__).parameters
        assert (p["w"].default, p["s"].default, p["order_hash"].default, p["order_seed"].default) == (None, None, "murmur", 42)
        assert callable(cls.sampled) and callable(cls.find_sequences)
    for cls in (kh.IndexGpuBackend, kh.WideIndexGpuBackend):
        assert inspect.signature(cls.__init__).parameters["s"].default is None
    # refusals in Python, before the library is asked for anything
    with pytest.raises(ValueError, match="one of them"):
        kh.KmerPositionIndex(k=15, w=10, s=11)
    with pytest.raises(ValueError, match="16-byte"):
        kh.WideKmerPositionIndex(k=40, w=10)
    for cls, k, s in ((kh.KmerPositionIndex, 15, 0), (kh.KmerPositionIndex, 15, 16), (kh.WideKmerPositionIndex, 64, 33), (kh.WideKmerPositionIndex, 20, 21)):
        with pytest.raises(ValueError, match="s must be"):
            cls(k=k, s=s)


def test_wide_index_with_s_constructs_or_fails_loudly():
    import kmerhash_amd as kh
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        ix = kh.WideKmerPositionIndex(k=40, s=20)
        try:
            assert (ix.k, ix.s, ix.w) == (40, 20, None)
        finally:
            ix.close()
    else:
        with pytest.raises(kh.KhError):
            kh.WideKmerPositionIndex(k=40, s=20)


def test_header_with_the_syncmer_section_compiles_as_c99(tmp_path):
    from kmerhash_amd.build import build_library
    build_library()
    src = tmp_path / "sy.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  uint64_t n = 9; uint64_t km[16]; uint32_t pos[8]; uint8_t mask[8];\n'
                   '  kh_status a = kh_syncmers_from_sequence("ACGTACGT", 8, 3, 0, 1, KH_HASH_MURMUR3_X64_128_H0, 42, KH_MEM_HOST, km, pos, 8, &n, 0, 0);\n'
                   '  kh_status b = kh_syncmers_from_fastq("ACGT", 4, 5, 3, 0, KH_HASH_FARM64, 1, KH_MEM_HOST, 0, 0, 0, &n, 0, 0);\n'
                   '  kh_status c = kh_syncmers128_from_sequence("ACGTACGT", 8, 40, 33, 1, KH_HASH_FARM64, 1, KH_MEM_HOST, km, pos, 8, &n, 0, 0);\n'
                   '  kh_status d = kh_syncmers128_from_fastq("ACGT", 4, 40, 20, 1, KH_HASH_FARM64, 1, KH_MEM_HOST, 0, 0, 0, &n, 0, 0);\n'
                   '  kh_status e = kh_syncmer_mask(km, 8, 3, 4, 1, KH_HASH_FARM64, 1, KH_MEM_HOST, mask, 0, 0);\n'
                   '  kh_status f = kh_wide_syncmer_mask(km, 0, 64, 32, 1, KH_HASH_FARM64, 1, KH_MEM_HOST, mask, 0, 0);\n'
                   '  kh_status g = kh_index_build_from_syncmers(0, "ACGT", 4, 3, 2, 1, KH_HASH_FARM64, 1, KH_MEM_HOST, 0);\n'
                   '  kh_status h = kh_index_append_from_syncmers(0, "ACGT", 4, 3, 2, 1, KH_HASH_FARM64, 1, KH_MEM_HOST, 1, 7);\n'
                   '  kh_status i = kh_wide_index_build_from_syncmers(0, "ACGT", 4, 3, 2, 1, KH_HASH_FARM64, 1, KH_MEM_HOST, 0);\n'
                   '  kh_status j = kh_wide_index_append_from_syncmers(0, "ACGT", 4, 3, 2, 1, KH_HASH_FARM64, 1, KH_MEM_HOST, 1, 7);\n'
                   '  printf("%d %d %d %d %d %d %d %d %d %d %d\\n", (int)a, (int)b, (int)c, (int)d, (int)e, (int)f, (int)g, (int)h, (int)i, (int)j, (int)n);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sy"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    # s = 0, too short, s > 32, too short, s > k, n = 0, null handle four times
    assert r.returncode == 0 and r.stdout.split() == ["1", "0", "1", "0", "1", "0", "1", "1", "1", "1", "0"], r.stdout
