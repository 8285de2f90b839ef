"""Compiler report of the wide position index's kernels (CPU test over kmerhash_amd/kernel_resources.json): every new kernel is in
the library, keeps its registers in registers (no scratch, no spilled VGPRs or SGPRs), and the probe kernels keep the occupancy of
kw_find, whose two-slot step they share."""
import json
import os

import pytest

from kmerhash_amd import build as B

# kernel -> number of instantiations (4 hashes; canonical or not)
NEW = {"kw_index_canon_runs": 1, "kw_index_rank": 1, "kw_index_scatter": 4, "kw_index_lookup": 4, "kw_kmers_emit_pos": 2}


@pytest.fixture(scope="module")
def resources():
    B.build_library()
    if not os.path.exists(B.RES):
        B.build_library(force=True)
    return json.load(open(B.RES))


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_wide_index_kernels_are_built_without_scratch_or_spills(resources, kernel):
    hits = {n: r for n, r in resources.items() if "%d%s" % (len(kernel), kernel) in n}      # (mangled: <length><name>)
    assert len(hits) == NEW[kernel], (kernel, sorted(hits))
    for name, r in hits.items():
        assert r["Scratch"] == 0 and r["VGPRSpill"] == 0 and r["SGPRSpill"] == 0, (name, r)


def test_occupancy_and_lds(resources):
    for name, r in resources.items():
        if "kw_index_scatter" in name or "kw_index_lookup" in name:
            assert r["Occupancy"] >= 4 and r["LDS"] == 0, (name, r)          # <= 128 VGPRs: four 256-lane workgroups per SIMD quartet
        if "kw_kmers_emit_pos" in name:
            assert r["Occupancy"] >= 8 and r["LDS"] <= 2048, (name, r)       # written straight out: the tile words only, no staging
