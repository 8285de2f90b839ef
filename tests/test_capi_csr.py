"""CPU: kh_csr_unpermute is declared, bound with the documented signature and exported; the refusals and the empty batch that need no
device behave as the header says; the Python surface of the sharded index exists; and the header still compiles as C."""
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
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read(), flags=re.S)
    m = re.search(r"kh_status\s+kh_csr_unpermute\s*\(([^)]*)\)\s*;", txt)
    assert m, "kh_csr_unpermute is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const uint32_t* counts_perm", "const uint32_t* pos_perm", "const uint32_t* origin", "uint64_t n", "uint32_t* out_counts",
                      "uint64_t* out_offsets", "uint32_t* out_pos", "uint64_t cap_out", "uint64_t* n_out", "int device", "void* hip_stream"]
    assert "kh_csr_unpermute" in capi.SYMBOLS
    f = capi.lib().kh_csr_unpermute                         # AttributeError: not exported
    vp, u64 = C.c_void_p, C.c_uint64
    assert list(f.argtypes) == [vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64), C.c_int, vp]
    assert f.restype is C.c_int


def test_refusals_and_the_empty_batch_need_no_device(capi):
    f = capi.lib().kh_csr_unpermute
    a = np.full(4, 7, dtype=np.uint32)
    out = C.c_uint64(123)
    for n in (1 << 32, (1 << 32) + 5, 1 << 40):             # refused before anything is touched, n_out included
        assert f(a.ctypes.data, a.ctypes.data, a.ctypes.data, n, a.ctypes.data, None, a.ctypes.data, 4, C.byref(out), 0, None) == capi.KH_ERR_INVALID
        assert out.value == 123 and (a == 7).all()
    assert f(None, None, a.ctypes.data, 3, None, None, None, 0, C.byref(out), 0, None) == capi.KH_ERR_INVALID
    assert f(a.ctypes.data, None, None, 3, None, None, None, 0, C.byref(out), 0, None) == capi.KH_ERR_INVALID
    out = C.c_uint64(123)
    assert f(None, None, None, 0, None, None, None, 0, C.byref(out), 0, None) == capi.KH_OK and out.value == 0
    assert f(None, None, None, 0, None, None, None, 0, None, 0, None) == capi.KH_OK


def test_python_surface():
    import kmerhash_amd as kh
    from kmerhash_amd import dist, dist_index
    assert kh.ShardedKmerPositionIndex is dist_index.ShardedKmerPositionIndex
    assert kh.IndexGpuBackend is dist_index.IndexGpuBackend and kh.WideIndexGpuBackend is dist_index.WideIndexGpuBackend
    S = kh.ShardedKmerPositionIndex
    assert issubclass(S, dist.ShardExchange) and not issubclass(S, dist.ShardedTable)      # a sibling of the table, not a table
    for name in ("append", "build", "append_sequences", "append_fastq", "build_sequences", "build_fastq", "count", "find", "find_sequences",
                 "erase", "erase_counts", "drop_above", "size", "total", "clear", "synchronize", "timings"):
        assert callable(getattr(S, name)), name
    assert isinstance(S.local, property)
    for name in ("append_sequences", "append_fastq", "build_sequences", "build_fastq"):
        assert inspect.signature(getattr(S, name)).parameters["pos_base"].default == 0
    p = inspect.signature(kh.IndexGpuBackend.__init__).parameters
    assert list(p)[1:9] == ["device", "k", "canonical", "hash", "seed", "w", "order_hash", "order_seed"]
    assert (p["seed"].default, p["w"].default) == (43, None)
    assert kh.WideIndexGpuBackend.key_words == 2 and "w" not in inspect.signature(kh.WideIndexGpuBackend.__init__).parameters
    assert kh.WideIndexGpuBackend.csr_unpermute is kh.IndexGpuBackend.csr_unpermute          # the unpermute never sees a key
    for b in (kh.IndexGpuBackend, kh.WideIndexGpuBackend):
        for name in ("shard", "empty", "text_pairs", "csr_unpermute"):
            assert callable(getattr(b, name)), (b, name)
        assert not hasattr(b, "shard_plan")
    assert "collectives" in dist_index.__doc__.lower()


def test_header_with_the_csr_call_compiles_as_c99(tmp_path):
    from kmerhash_amd.build import build_library
    build_library()
    src = tmp_path / "csr.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  uint64_t n = 9; uint32_t a[4] = {0, 0, 0, 0};\n'
                   '  kh_status x = kh_csr_unpermute(a, a, a, (uint64_t)1 << 32, a, 0, a, 4, &n, 0, 0);\n'
                   '  kh_status y = kh_csr_unpermute(0, 0, 0, 0, 0, 0, 0, 0, &n, 0, 0);\n'
                   '  printf("%d %d %d\\n", (int)x, (int)y, (int)n);\n  return 0;\n}\n')
    exe = tmp_path / "csr"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["1", "0", "0"], r.stdout      # refused, empty batch, *n_out = 0
