"""CPU: the C-ABI additions for reducer inserts beyond std::plus -- kh_insert_reduce, kh_wide_insert_reduce, the kh_reduce_op enum
and the KH_INS_REDUCE(op) flags of the streamed form -- are declared in include/kmerhash_amd.h, bound in kmerhash_amd._capi, exported
by the built library and usable from C99; and the Python wrappers refuse a bad operation before anything reaches the library."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"kh_insert_reduce": "kh_table", "kh_wide_insert_reduce": "kh_wtable"}


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def test_new_symbols_are_declared_bound_and_exported(capi):
    L = capi.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read(), flags=re.S)
    for s, handle in NEW.items():
        assert re.search(r"\bkh_status\s+%s\s*\(\s*%s\s*\*" % (s, handle), hdr), "%s(%s*, ...) is not declared in the header" % (s, handle)
        assert s in capi.SYMBOLS
        assert hasattr(L, s), "library does not export %s" % s
        assert len(getattr(L, s).argtypes) == 7
    assert re.search(r"KH_REDUCE_PLUS\s*=\s*0\s*,\s*KH_REDUCE_MIN\s*=\s*1\s*,\s*KH_REDUCE_MAX\s*=\s*2\s*,\s*KH_REDUCE_OR\s*=\s*3\s*}\s*kh_reduce_op", hdr)
    assert re.search(r"#define\s+KH_INS_REDUCE_PLUS\s+1u\b", hdr) and re.search(r"#define\s+KH_INS_REPEATABLE\s+2u\b", hdr)
    assert (capi.KH_REDUCE_PLUS, capi.KH_REDUCE_MIN, capi.KH_REDUCE_MAX, capi.KH_REDUCE_OR) == (0, 1, 2, 3)
    assert capi.REDUCE_OPS == {"plus": 0, "min": 1, "max": 2, "or": 3}


def test_header_compiles_as_c99_with_the_enum_and_the_flag_field(tmp_path):
    """the operation is a bit-field next to KH_INS_REDUCE_PLUS, which keeps its value; a NULL handle is refused without a GPU"""
    from kmerhash_amd.build import build_library
    build_library()
    src = tmp_path / "use_reduce.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  uint64_t n = 7, keys[2] = {1, 2}; uint32_t vals[2] = {3, 4}; kh_reduce_op op = KH_REDUCE_MAX;\n'
                   '  if (KH_INS_REDUCE_PLUS != 1u || KH_INS_REPEATABLE != 2u || KH_INS_REDUCE(KH_REDUCE_PLUS) != KH_INS_REDUCE_PLUS) return 2;\n'
                   '  if (KH_INS_REDUCE_MIN != 5u || KH_INS_REDUCE_MAX != 9u || KH_INS_REDUCE_OR != 13u || KH_INS_REDUCE(op) != KH_INS_REDUCE_MAX) return 3;\n'
                   '  if ((KH_INS_REDUCE_OR & KH_INS_REDUCE_OP_MASK) >> KH_INS_REDUCE_OP_SHIFT != KH_REDUCE_OR || (KH_INS_REDUCE_OP_MASK & 3u)) return 4;\n'
                   '  if (kh_insert_reduce(0, keys, vals, 2, KH_MEM_HOST, op, &n) != KH_ERR_INVALID) return 5;\n'
                   '  if (kh_wide_insert_reduce(0, keys, vals, 1, KH_MEM_HOST, KH_REDUCE_OR, &n) != KH_ERR_INVALID) return 6;\n'
                   '  if (kh_insert_begin_ex(0, 2, KH_INS_REDUCE_MIN | KH_INS_REPEATABLE) != KH_ERR_INVALID) return 7;\n'
                   '  printf("%s\\n", kh_version());\n  return 0;\n}\n')
    exe = tmp_path / "use_reduce"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gfx950" in r.stdout, (r.returncode, r.stdout)


def test_flags_of_the_streamed_form(capi):
    f = capi.ins_flags
    assert f() == 0 and f(reduce_plus=True) == 1 and f(repeatable=True) == 2 and f(True, True) == 3
    assert f(reduce="plus") == 1 and f(reduce_plus=True, reduce="plus") == 1
    assert f(reduce="min") == 5 and f(reduce="max", repeatable=True) == 11 and f(reduce="or") == 13
    with pytest.raises(ValueError):
        f(reduce="xor")
    with pytest.raises(ValueError):
        f(reduce_plus=True, reduce="max")


def test_python_wrappers_refuse_a_bad_operation_before_any_gpu_call():
    """no table is constructed (that needs a GPU): the members are called on a bare object and must raise before they touch it"""
    import kmerhash_amd as kh
    keys, vals = np.arange(4, dtype=np.uint64), np.arange(4, dtype=np.uint32)
    classes = [kh.hashmap_robinhood_doubling, kh.hashmap_linearprobe_doubling, kh.hashmap_robinhood_doubling_wide,
               kh.hashmap_robinhood_doubling_wide_stream]
    for cls in classes:
        bare = object.__new__(cls)
        kk = keys if cls in classes[:2] else keys.reshape(2, 2)
        for bad in ("xor", "replace", None, 2, "MAX"):
            with pytest.raises(ValueError):
                bare.insert_reduce(kk, vals[: len(kk)], bad)
            with pytest.raises(ValueError):
                bare.merge(bare, op=bad)
        for op in ("min", "max", "or"):
            with pytest.raises(ValueError):
                bare.insert_reduce(kk, None, op)
        if hasattr(cls, "insert_begin"):
            with pytest.raises(ValueError):
                bare.insert_begin(4, reduce="xor")
            with pytest.raises(ValueError):
                bare.insert_begin(4, reduce_plus=True, reduce="min")
    with pytest.raises(ValueError):       # tables of different key width (checked before the GPU is asked for anything)
        object.__new__(classes[0]).merge(object.__new__(classes[2]), op="max")
