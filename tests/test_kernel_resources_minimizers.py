"""Compiler report of the minimizer kernels (CPU test over kmerhash_amd/kernel_resources.json): both passes are in the library once per
ordering hash and strand rule (4 hashes x canonical on / off), keep their registers in registers, and hold the LDS layout and the
occupancy DESIGN.md §3 states: 50656 B per workgroup (keys 39168, range minima 9216, packed text 1740, marks and wave totals 528, padded
to 8), three workgroups per CU = three waves per SIMD, which is also what the launch bounds hold the registers to."""
import json
import os

import pytest

from kmerhash_amd import build as B

NEW = {"k_minimizers_count": 8, "k_minimizers_emit": 8}
LDS_BYTES = 50656
WAVES_PER_SIMD = 3


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
    for hash_ in range(4):                                  # KH_SWITCH_HASH x canonical
        for canon in (0, 1):
            assert sum("ILi%dELb%dEE" % (hash_, canon) in n for n in hits) == 1, (kernel, hash_, canon)
    for name, r in hits.items():
        assert r["Scratch"] == 0 and r["VGPRSpill"] == 0 and r["SGPRSpill"] == 0, (name, r)


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_lds_and_occupancy_are_the_documented_ones(resources, kernel):
    for name, r in of(resources, kernel).items():
        assert r["LDS"] == LDS_BYTES, (name, r)
        assert 3 * r["LDS"] <= 160 * 1024 < 4 * r["LDS"]      # three workgroups of four waves per CU
        assert r["Occupancy"] == WAVES_PER_SIMD, (name, r)
        assert r["VGPRs"] <= 512 // WAVES_PER_SIMD, (name, r)


def test_the_all_window_front_end_is_still_there(resources):
    for kernel, n in (("k_kmers_count", 2), ("k_kmers_emit", 2), ("k_kmers_emit_pos", 2), ("k_fastq_mask", 1), ("k_index_add_base", 1)):
        assert len(of(resources, kernel)) == n, kernel
