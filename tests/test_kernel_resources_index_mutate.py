"""Compiler report of the kernels that carry a position index across a change of its key set (CPU test over
kmerhash_amd/kernel_resources.json): every new kernel is in the library exactly as often as it is launched (two slot layouts, or four
hashes), keeps its registers in registers (no scratch, no spilled VGPRs or SGPRs), the streaming passes run at full occupancy and the
kernels that probe the batch keep the occupancy of the lookups they sit beside."""
import json
import os

import pytest

from kmerhash_amd import build as B

# kernel -> number of instantiations (2 slot layouts: 64-bit and wide Robin Hood; 4 hashes)
NEW = {"k_index_stamp": 2, "k_index_rank_carry": 2, "k_index_len_count": 2, "k_index_len_emit": 2, "k_index_move": 1, "k_index_add_base": 1,
       "k_index_count_pairs": 4, "kw_index_count_pairs": 4}


@pytest.fixture(scope="module")
def resources():
    B.build_library()
    if not os.path.exists(B.RES):
        B.build_library(force=True)
    return json.load(open(B.RES))


def of(resources, kernel):
    return {n: r for n, r in resources.items() if "%d%s" % (len(kernel), kernel) in n}      # (mangled: <length><name>)


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_mutation_kernels_are_built_without_scratch_or_spills(resources, kernel):
    hits = of(resources, kernel)
    assert len(hits) == NEW[kernel], (kernel, sorted(hits))
    for name, r in hits.items():
        assert r["Scratch"] == 0 and r["VGPRSpill"] == 0 and r["SGPRSpill"] == 0, (name, r)


def test_occupancy_and_lds(resources):
    for kernel in ("k_index_stamp", "k_index_rank_carry", "k_index_len_count", "k_index_len_emit", "k_index_move", "k_index_add_base"):
        for name, r in of(resources, kernel).items():
            assert r["Occupancy"] >= 8 and r["LDS"] <= 128, (name, r)                 # streaming passes: a (row, wave) count table at most
    # the probes of the batch: no worse than the lookup of the same key width and hash, no LDS
    for mine, beside in (("k_index_count_pairs", "k_index_lookup"), ("kw_index_count_pairs", "kw_index_lookup")):
        floor = min(r["Occupancy"] for r in of(resources, beside).values())
        assert floor >= 4
        for name, r in of(resources, mine).items():
            assert r["Occupancy"] >= floor and r["LDS"] == 0, (name, r, floor)


def test_the_build_kernels_are_still_there_once_each(resources):
    for kernel, n in (("k_index_rank", 1), ("kw_index_rank", 1), ("k_index_scatter", 4), ("kw_index_scatter", 4), ("k_index_tile_sort", 1),
                      ("k_index_seg_radix", 1), ("k_index_gather", 1)):
        assert len(of(resources, kernel)) == n, kernel
