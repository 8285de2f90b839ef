"""CPU: the value-range operations (kh_value_histogram / kh_select_values / kh_erase_values and their kh_wide_ forms) are declared in
include/kmerhash_amd.h, bound with argument types in kmerhash_amd._capi, exported by the library, callable from C99, and surface as
members of the three table classes, of KmerCounter / ShardedKmerCounter and of dist.ShardedTable."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kh_value_histogram", "kh_select_values", "kh_erase_values", "kh_wide_value_histogram", "kh_wide_select_values", "kh_wide_erase_values"]


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def test_six_symbols_declared_bound_and_exported(capi):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read(), flags=re.S)
    L = capi.lib()
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    pu64 = C.POINTER(C.c_uint64)
    want = {"value_histogram": [vp, u32, vp], "select_values": [vp, u32, u32, i32, vp, vp, u64, pu64], "erase_values": [vp, u32, u32, pu64]}
    for s in NEW:
        assert re.search(r"\bkh_status\s+%s\s*\(" % s, txt), "%s is not declared" % s
        assert s in capi.SYMBOLS
        f = getattr(L, s)                                   # AttributeError: not exported
        assert list(f.argtypes) == want[s.replace("kh_wide_", "").replace("kh_", "")], (s, f.argtypes)
        assert f.restype is i32
    # the wide forms take the wide handle type
    for s in NEW[3:]:
        assert re.search(r"%s\s*\(\s*kh_wtable\s*\*" % s, txt), s
    for s in NEW[:3]:
        assert re.search(r"%s\s*\(\s*kh_table\s*\*" % s, txt), s


def test_header_with_a_call_to_each_compiles_as_c99(capi, tmp_path):
    src = tmp_path / "use_values.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  kh_table* t = 0; kh_wtable* w = 0; uint64_t n = 0, h[4], k[8]; uint32_t v[4];\n'
                   '  kh_status s = kh_create(&t, KH_KIND_ROBINHOOD, 8, 4, KH_HASH_MURMUR3_X86_128_LO64, 43, 128, 0.35f, 0.8f, 0);\n'
                   '  if (s == KH_OK) {\n'
                   '    kh_value_histogram(t, 4, h); kh_select_values(t, 0, UINT32_MAX, KH_MEM_HOST, k, v, 4, &n); kh_erase_values(t, 1, 2, &n);\n'
                   '    kh_destroy(t);\n  }\n'
                   '  if (kh_wide_create(&w, KH_KIND_ROBINHOOD, KH_HASH_IDENTITY, 43, 128, 0.4f, 0.9f, 0) == KH_OK) {\n'
                   '    kh_wide_value_histogram(w, 4, h); kh_wide_select_values(w, 2, 1, KH_MEM_HOST, k, v, 4, &n); kh_wide_erase_values(w, 0, 0, &n);\n'
                   '    kh_wide_destroy(w);\n  }\n'
                   '  printf("%s status=%d n=%d\\n", kh_version(), (int)s, (int)n);\n  return 0;\n}\n')
    exe = tmp_path / "use_values"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gfx950" in r.stdout


def test_null_table_is_refused(capi):
    L = capi.lib()
    n = C.c_uint64(7)
    out = (C.c_uint64 * 4)()
    for pre in ("kh_", "kh_wide_"):
        assert getattr(L, pre + "value_histogram")(None, 4, out) == capi.KH_ERR_INVALID
        assert getattr(L, pre + "select_values")(None, 0, 1, capi.KH_MEM_HOST, None, None, 0, C.byref(n)) == capi.KH_ERR_INVALID
        assert n.value == 0
        n.value = 7
        assert getattr(L, pre + "erase_values")(None, 0, 1, C.byref(n)) == capi.KH_ERR_INVALID
        assert n.value == 0
        n.value = 7


def test_table_classes_have_the_four_members():
    import kmerhash_amd as kh
    from kmerhash_amd.wide import hashmap_robinhood_doubling_wide, hashmap_robinhood_doubling_wide_stream
    for cls in (kh.hashmap_robinhood_doubling, kh.hashmap_linearprobe_doubling, hashmap_robinhood_doubling_wide, hashmap_robinhood_doubling_wide_stream):
        for m in ("value_histogram", "count_values", "select_values", "erase_values"):
            assert callable(getattr(cls, m, None)), (cls.__name__, m)


def test_counters_and_sharded_table_have_their_members():
    from kmerhash_amd.dist import ShardedTable
    from kmerhash_amd.kmers import KmerCounter, ShardedKmerCounter
    for m in ("spectrum", "drop_below", "counts"):
        assert callable(getattr(KmerCounter, m, None)), m
    for m in ("spectrum", "drop_below"):
        assert callable(getattr(ShardedKmerCounter, m, None)), m
    for m in ("value_histogram", "erase_values"):
        assert callable(getattr(ShardedTable, m, None)), m


def test_value_range_bounds_are_checked_before_the_library_sees_them():
    """a bound outside 0..2^32-1 must not be wrapped by ctypes into another range"""
    from kmerhash_amd.table import _TableCore
    assert _TableCore._value_range(0, 0xFFFFFFFF) == (0, 0xFFFFFFFF)
    for lo, hi in ((-1, 5), (0, 1 << 32), (1 << 40, 1 << 41)):
        with pytest.raises(ValueError):
            _TableCore._value_range(lo, hi)
