"""Compiler report of the closed-syncmer kernels (CPU test over kmerhash_amd/kernel_resources.json): the count pass is in the library
once per ordering hash and strand rule (it never looks at a k-mer, so it has no key width), the emit pass and the keep test on packed
k-mers once more per key width; all keep their registers in registers; the two text passes hold the LDS layout and the occupancy their
header comment in csrc/kh_kernels_index.h states: 45784 B per workgroup (keys 35360, range minima 8320, packed text 1572, marks and wave
totals 528, padded to 8), three workgroups per CU = three waves per SIMD, which is also what the launch bounds hold the registers to.
The keep test on keys uses no LDS.  The minimizer and all-window kernels are still there with the resources they had."""
import json
import os

import pytest

from kmerhash_amd import build as B

NEW = {"k_syncmers_count": 8, "k_syncmers_emit": 16, "k_syncmer_mask": 16}
TEXT_PASSES = ("k_syncmers_count", "k_syncmers_emit")
LDS_BYTES = 45784
WAVES_PER_SIMD = 3
# (instantiations, LDS bytes, waves per SIMD) of the kernels this feature sits next to, as they were before it
OLD = {"k_minimizers_count": (8, 50656, 3), "k_minimizers_emit": (8, 50656, 3), "k_kmers_count": (2, None, None), "k_kmers_emit": (2, None, None),
       "k_kmers_emit_pos": (2, None, None), "kw_kmers_emit": (2, None, None), "kw_kmers_emit_pos": (2, None, None), "k_fastq_mask": (1, None, None),
       "k_index_add_base": (1, None, None)}


@pytest.fixture(scope="module")
def resources():
    B.build_library()
    if not os.path.exists(B.RES):
        B.build_library(force=True)
    return json.load(open(B.RES))


def of(resources, kernel):
    return {n: r for n, r in resources.items() if "%d%s" % (len(kernel), kernel) in n}      # (mangled: <length><name>)


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_instantiations_without_scratch_or_spills(resources, kernel):
    hits = of(resources, kernel)
    assert len(hits) == NEW[kernel], (kernel, sorted(hits))
    widths = ("",) if kernel == "k_syncmers_count" else ("ELi1", "ELi2")
    for hash_ in range(4):                                  # KH_SWITCH_HASH x canonical x key width
        for canon in (0, 1):
            for kw in widths:
                assert sum("ILi%dELb%d%sEE" % (hash_, canon, kw) in n for n in hits) == 1, (kernel, hash_, canon, kw)
    for name, r in hits.items():
        assert r["Scratch"] == 0 and r["VGPRSpill"] == 0 and r["SGPRSpill"] == 0, (name, r)


@pytest.mark.parametrize("kernel", TEXT_PASSES)
def test_lds_and_occupancy_are_the_documented_ones(resources, kernel):
    assert 35360 + 8320 + 1048 + 524 + 512 + 16 == 45780 and (45780 + 7) // 8 * 8 == LDS_BYTES
    for name, r in of(resources, kernel).items():
        assert r["LDS"] == LDS_BYTES, (name, r)
        assert 3 * r["LDS"] <= 160 * 1024 < 4 * r["LDS"]      # three workgroups of four waves per CU
        assert r["Occupancy"] == WAVES_PER_SIMD, (name, r)
        assert r["VGPRs"] <= 512 // WAVES_PER_SIMD, (name, r)


def test_the_key_test_needs_no_lds(resources):
    for name, r in of(resources, "k_syncmer_mask").items():
        assert r["LDS"] == 0 and r["VGPRs"] <= 64, (name, r)      # (64: the full eight waves per SIMD)


def test_the_minimizer_and_all_window_kernels_are_unchanged(resources):
    for kernel, (n, lds, occ) in OLD.items():
        hits = of(resources, kernel)
        assert len(hits) == n, (kernel, sorted(hits))
        for name, r in hits.items():
            assert r["Scratch"] == 0 and r["VGPRSpill"] == 0 and r["SGPRSpill"] == 0, (name, r)
            if lds is not None:
                assert (r["LDS"], r["Occupancy"]) == (lds, occ), (name, r)
