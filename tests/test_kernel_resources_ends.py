"""Compiler report of the kernels kh_chain_ends adds (CPU test over kmerhash_amd/kernel_resources.json): k_ends_wfa and k_ends_emit are
in the library once each, keep their registers in registers (no scratch, no spills), use no LDS -- furthest-reaching points, moves and
the best score of a diagonal live in registers of its lane -- and run at the full eight waves per SIMD, as DESIGN.md §3 states; the
cigar, edits, chain and anchor kernels they sit beside are still built, each in as many instantiations as before."""
import json
import os

import pytest

from kmerhash_amd import build as B

NEW = {"k_ends_wfa": 1, "k_ends_emit": 1}
LDS_BYTES = 0
WAVES_PER_SIMD = 8
OLD = {"k_cigar_classify": 1, "k_cigar_wfa": 1, "k_cigar_emit": 1, "k_edits_classify": 1, "k_edits_wfa": 1, "k_chain_dp": 1, "k_chain_link": 1, "k_chain_emit": 2, "k_anchors_expand": 1, "k_pos_strand": 2,
       "k_index_tile_sums": 1, "k_index_scan_sums": 1, "k_index_scan_apply": 2}


@pytest.fixture(scope="module")
def resources():
    B.build_library()
    if not os.path.exists(B.RES):
        B.build_library(force=True)
    return json.load(open(B.RES))


def of(resources, kernel):
    return {n: r for n, r in resources.items() if "%d%s" % (len(kernel), kernel) in n}      # (mangled: <length><name>)


def test_every_ends_kernel_is_a_listed_one(resources):
    names = [n for n in resources if "k_ends_" in n]
    assert len(names) == sum(NEW.values()), names
    for n in names:
        assert any("%d%s" % (len(k), k) in n for k in NEW), n


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_built_once_without_scratch_or_spills(resources, kernel):
    hits = of(resources, kernel)
    assert len(hits) == NEW[kernel], (kernel, sorted(hits))
    for name, r in hits.items():
        assert r["Scratch"] == 0 and r["VGPRSpill"] == 0 and r["SGPRSpill"] == 0, (name, r)


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_lds_and_occupancy_are_the_documented_ones(resources, kernel):
    hits = of(resources, kernel)
    assert len(hits) == NEW[kernel], (kernel, sorted(hits))
    for name, r in hits.items():
        assert r["LDS"] == LDS_BYTES, (name, r)
        assert r["Occupancy"] == WAVES_PER_SIMD, (name, r)
        assert r["VGPRs"] <= 512 // WAVES_PER_SIMD, (name, r)


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_design_states_these_numbers(kernel):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = [l for l in open(os.path.join(root, "DESIGN.md")) if kernel in l and l.lstrip().startswith("|")]
    assert rows, "DESIGN.md §3 has no row for %s" % kernel
    assert any("no LDS" in l and "8 waves/SIMD" in l for l in rows), rows


@pytest.mark.parametrize("kernel", sorted(OLD))
def test_the_kernels_beside_them_are_still_built_as_often(resources, kernel):
    assert len(of(resources, kernel)) == OLD[kernel], kernel
