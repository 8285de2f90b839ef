"""CPU: the C-ABI additions for the HyperLogLog of every k-mer length -- kh_hll_update_wide, kh_hll_update_from_sequence and
kh_hll_update_from_fastq -- are declared in include/kmerhash_amd.h, bound with argument types in kmerhash_amd._capi, exported by the
built library and callable from C99; the Python layer has the members that use them; and the new kernels are in the compiler's
resource report without scratch or spills (tests/test_kernel_resources.py checks the whole report)."""
import inspect
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["kh_hll_update_wide", "kh_hll_update_from_sequence", "kh_hll_update_from_fastq"]


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
        assert re.search(r"\bkh_status\s+%s\s*\(\s*kh_hll\s*\*" % s, hdr), "%s(kh_hll*, ...) is not declared in the header" % s
        assert s in capi.SYMBOLS
        assert hasattr(L, s), "library does not export %s" % s
        assert getattr(L, s).argtypes is not None, "%s has no argtypes" % s
    assert len(L.kh_hll_update_wide.argtypes) == 4
    assert len(L.kh_hll_update_from_sequence.argtypes) == len(L.kh_hll_update_from_fastq.argtypes) == 7
    # appended: nothing that was declared before them moved behind them
    assert hdr.index("kh_hll_update_wide") > hdr.index("kh_kmers128_from_fastq") > hdr.index("kh_hll_estimate_registers")


def test_header_with_the_new_calls_compiles_as_c99_and_refuses_bad_arguments(tmp_path):
    """the argument checks come before any use of the GPU: a NULL handle is KH_ERR_INVALID on a machine without one"""
    from kmerhash_amd.build import build_library
    build_library()
    src = tmp_path / "use_hll.c"
    src.write_text('#include "kmerhash_amd.h"\n#include <stdio.h>\n'
                   'int main(void) {\n  uint64_t n = 7, keys[2] = {1, 2}; const char* seq = "ACGT";\n'
                   '  if (kh_hll_update_wide(0, keys, 1, KH_MEM_HOST) != KH_ERR_INVALID) return 2;\n'
                   '  if (kh_hll_update_from_sequence(0, seq, 4, 3, 1, KH_MEM_HOST, &n) != KH_ERR_INVALID || n != 0) return 3;\n'
                   '  if (kh_hll_update_from_fastq(0, seq, 4, 3, 1, KH_MEM_HOST, 0) != KH_ERR_INVALID) return 4;\n'
                   '  printf("%s\\n", kh_version());\n  return 0;\n}\n')
    exe = tmp_path / "use_hll"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src),
                        "-L" + os.path.join(ROOT, "kmerhash_amd"), "-lkmerhash_amd",
                        "-Wl,-rpath," + os.path.join(ROOT, "kmerhash_amd"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gfx950" in r.stdout, (r.returncode, r.stdout)


def test_python_members():
    from kmerhash_amd import kmers as KM
    from kmerhash_amd.hll import hyperloglog64 as H
    for m in ("update_wide", "update_from_sequence", "update_from_fastq", "text_grid"):
        assert callable(getattr(H, m, None)), m
    called = set(re.findall(r"kh_hll_update_[a-z_]+", inspect.getsource(H)))
    assert set(NEW) <= called, called
    sig = inspect.signature(KM.KmerCounter.__init__).parameters
    assert sig["reserve_from_estimate"].default is False
    assert callable(KM.KmerCounter.presize_sequences) and callable(KM.KmerCounter.presize_fastq)
    sig = inspect.signature(KM.ShardedKmerCounter.__init__).parameters
    assert sig["estimate_from_text"].default is False and sig["reserve_from_estimate"].default is False


def test_sharded_kmer_counter_estimator_checks():
    """refused up front, no GPU needed: a wide counter sized from an estimate needs an estimator with update_wide; an estimate from
    the text needs reserve_from_estimate and an estimator with update_from_fastq"""
    from kmerhash_amd import kmers as KM

    class B:
        pass

    class ST:
        def __init__(self, words):
            self.b = B()
            if words:
                self.b.key_words = words
            self.group = None

    class Narrow:
        def update(self, km):
            pass

    class Wide(Narrow):
        def update_wide(self, km):
            pass

    class Text(Wide):
        def update_from_fastq(self, text, k, canonical=True):
            return 0

    with pytest.raises(ValueError, match="HyperLogLog"):
        KM.ShardedKmerCounter(ST(2), 63, reserve_from_estimate=True)
    with pytest.raises(ValueError, match="HyperLogLog"):
        KM.ShardedKmerCounter(ST(2), 63, reserve_from_estimate=True, hll=Narrow())
    assert KM.ShardedKmerCounter(ST(2), 63, reserve_from_estimate=True, hll=Wide()).wide
    KM.ShardedKmerCounter(ST(0), 31, reserve_from_estimate=True, hll=Narrow())
    for k, st in ((31, ST(0)), (63, ST(2))):
        for kw in ({"estimate_from_text": True}, {"estimate_from_text": True, "hll": Text()},
                   {"estimate_from_text": True, "reserve_from_estimate": True, "hll": Wide()}):
            with pytest.raises(ValueError, match="estimate_from_text"):
                KM.ShardedKmerCounter(st, k, **kw)
        assert KM.ShardedKmerCounter(st, k, reserve_from_estimate=True, estimate_from_text=True, hll=Text()).estimate_from_text


def test_driver_flags_are_checked_before_any_gpu_work():
    import sys
    drv = [sys.executable, os.path.join(ROOT, "benchmark", "kmer_counter.py")]
    r = subprocess.run(drv + ["-k", "63", "--hll-reserve"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--hll-reserve" in r.stderr and "--estimate-reserve" in r.stderr and not r.stdout.strip()
    r = subprocess.run(drv + ["-k", "65", "--estimate-reserve"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and not r.stdout.strip()
    r = subprocess.run(drv + ["--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--estimate-reserve" in r.stdout


def test_new_kernels_in_the_resource_report(capi):
    from kmerhash_amd import build as B
    if not os.path.exists(B.RES):
        B.build_library(force=True)
    res = json.load(open(B.RES))
    wide = {n: r for n, r in res.items() if "k_hll_updateI" in n and "ELi2EE" in n}       # k_hll_update<HASH, 16-byte keys>
    text = {n: r for n, r in res.items() if "k_hll_from_textI" in n}
    assert len(wide) == 4 and len(text) == 16, (sorted(wide), sorted(text))          # 4 hashes; x 2 key widths x canonical or not
    for name, r in list(wide.items()) + list(text.items()):
        assert r.get("Scratch", 0) == 0 and r.get("VGPRSpill", 0) == 0 and r.get("SGPRSpill", 0) == 0, (name, r)
    for name, r in text.items():
        # four 256-lane workgroups per CU (4 waves per SIMD) is what the host's grid assumes: <= 128 VGPRs, and the static LDS next to
        # the 32 KB of registers at precision 13 stays under 160 KB / 4
        assert r["Occupancy"] >= 4 and r["VGPRs"] <= 128 and r["LDS"] + (4 << 13) <= (160 << 10) // 4, (name, r)
