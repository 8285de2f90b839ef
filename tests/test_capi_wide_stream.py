"""CPU: the C-ABI additions for wide keys across GPUs -- the streamed insert of the wide table (kh_wide_insert_begin_ex / feed / end /
abort) and kh_wide_shard_permute -- are declared in include/kmerhash_amd.h, exported by the built library, bound in _capi, and usable
from plain C; the Python members live on a subclass, hashmap_robinhood_doubling_wide itself keeps exactly its members."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kh_wide_insert_begin_ex", "kh_wide_insert_feed", "kh_wide_insert_end", "kh_wide_insert_abort", "kh_wide_shard_permute"]
STREAMED = ["insert_begin", "insert_feed", "insert_end", "insert_abort"]


@pytest.fixture(scope="module")
def capi():
    from kmerhash_amd.build import build_library
    build_library()
    from kmerhash_amd import _capi
    return _capi


def header_without_comments():
    txt = open(os.path.join(ROOT, "include", "kmerhash_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_new_symbols_are_declared_bound_and_exported(capi):
    L = capi.lib()
    hdr = header_without_comments()
    for s in NEW:
        assert re.search(r"\bkh_status\s+%s\s*\(" % s, hdr), "%s is not declared in the header" % s
        assert s in capi.SYMBOLS
        assert hasattr(L, s), "library does not export %s" % s
        assert getattr(L, s).argtypes is not None, "%s has no argtypes" % s
    # the first parameter of the streamed calls is the wide handle type: a kh_table* does not compile there
    for s in NEW[:4]:
        assert re.search(r"%s\s*\(\s*kh_wtable\s*\*" % s, hdr), s
    assert len(L.kh_wide_shard_permute.argtypes) == 11 and len(L.kh_wide_insert_feed.argtypes) == 5


def test_streamed_members_live_on_a_subclass():
    import kmerhash_amd as kh
    from kmerhash_amd.wide import hashmap_robinhood_doubling_wide as W, hashmap_robinhood_doubling_wide_stream as S
    assert kh.hashmap_robinhood_doubling_wide_stream is S and "hashmap_robinhood_doubling_wide_stream" in kh.__all__
    assert issubclass(S, W) and S is not W
    assert [m for m in STREAMED if hasattr(W, m)] == []
    assert [m for m in STREAMED if not callable(getattr(S, m, None))] == []
    assert S.PREFIX == "kh_wide_"
    # the subclass never reaches a 64-bit entry point: its own source names kh_wide_* calls only
    import inspect
    called = set(re.findall(r"_L\.(kh_[a-z0-9_]+)", inspect.getsource(S)))
    assert called == set(NEW[:4]), called


def test_sharding_layer_reads_the_key_width_from_the_backend():
    from kmerhash_amd import dist as D
    assert D.WideGpuBackend.key_words == 2 and not hasattr(D.WideGpuBackend, "shard_plan")
    assert not hasattr(D.GpuBackend, "key_words") and hasattr(D.GpuBackend, "shard_plan")


def test_header_with_the_new_calls_compiles_as_c99_and_links(tmp_path):
    from kmerhash_amd.build import build_library
    build_library()
    src = tmp_path / "use_wide.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  kh_wtable* t = 0; uint64_t n = 0, counts[4] = {9, 9, 9, 9}; kh_status s, p;\n'
                   '  s = kh_wide_create(&t, KH_KIND_ROBINHOOD, KH_HASH_MURMUR3_X86_128_LO64, 43, 128, 0.4f, 0.9f, 0);\n'
                   '  if (s == KH_OK) {\n'
                   '    if (kh_wide_insert_feed(t, 0, 0, 0, KH_MEM_HOST) != KH_ERR_INVALID) return 2;\n'
                   '    if (kh_wide_insert_end(t, &n) != KH_ERR_INVALID) return 3;\n'
                   '    if (kh_wide_insert_begin_ex(t, 0, KH_INS_REDUCE_PLUS | KH_INS_REPEATABLE) != KH_OK) return 4;\n'
                   '    if (kh_wide_insert_abort(t) != KH_OK) return 5;\n'
                   '    kh_wide_destroy(t);\n  }\n'
                   '  p = kh_wide_shard_permute(KH_HASH_FARM64, 1, 0, 0, 0, 0, 0, 0, counts, 0, 0);\n'
                   '  printf("%s status=%d permute=%d\\n", kh_version(), (int)s, (int)p);\n'
                   '  return p == KH_ERR_INVALID ? 0 : 6;\n}\n')
    exe = tmp_path / "use_wide"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gfx950" in r.stdout and "permute=1" in r.stdout, (r.returncode, r.stdout)


def test_sharded_kmer_counter_checks_the_key_width():
    """k and the sharded table's key width must agree; a wide counter has no HyperLogLog sizing (no GPU needed: refused up front)"""
    from kmerhash_amd import kmers as KM

    class B:
        pass

    class ST:
        def __init__(self, words):
            self.b = B()
            if words:
                self.b.key_words = words
            self.group = None

    KM.ShardedKmerCounter(ST(0), 31)
    KM.ShardedKmerCounter(ST(2), 63)
    KM.ShardedKmerCounter(ST(2), 33)
    for st, k in ((ST(0), 63), (ST(1), 33), (ST(2), 31), (ST(2), 32)):
        with pytest.raises(ValueError, match="byte keys"):
            KM.ShardedKmerCounter(st, k)
    with pytest.raises(ValueError, match="HyperLogLog"):
        KM.ShardedKmerCounter(ST(2), 63, reserve_from_estimate=True)
    with pytest.raises(ValueError):
        KM.ShardedKmerCounter(ST(2), 65)
