"""Compiler report of the kernels kh_chain_records and kh_cigar_text add (CPU test over kmerhash_amd/kernel_resources.json): each is in
the library once, keeps its registers in registers (no scratch, no spills), uses no LDS, and runs at the waves per SIMD DESIGN.md §3
states -- seven for k_records_count, whose pointers and wave-uniform walk state take 101 scalar registers, eight for the rest; the scan,
ends, cigar, edits, chain and select kernels they sit beside are still built, each in as many instantiations as before."""
import json
import os

import pytest

from kmerhash_amd import build as B

NEW = {"k_records_count": 7, "k_records_emit": 8, "k_text_count": 8, "k_text_rows": 8, "k_text_emit": 8}      # kernel: waves per SIMD
OLD = {"k_ends_wfa": 1, "k_ends_emit": 1, "k_select_wave": 1, "k_select_block": 1, "k_cigar_classify": 1, "k_cigar_wfa": 1, "k_cigar_emit": 1, "k_edits_classify": 1,
       "k_edits_wfa": 1, "k_chain_dp": 1, "k_chain_link": 1, "k_chain_emit": 2, "k_anchors_expand": 1, "k_pos_strand": 2, "k_index_tile_sums": 1, "k_index_scan_sums": 1,
       "k_index_scan_apply": 2}


@pytest.fixture(scope="module")
def resources():
    B.build_library()
    if not os.path.exists(B.RES):
        B.build_library(force=True)
    return json.load(open(B.RES))


def of(resources, kernel):
    return {n: r for n, r in resources.items() if "%d%s" % (len(kernel), kernel) in n}      # (mangled: <length><name>)


def test_every_new_kernel_is_a_listed_one(resources):
    names = [n for n in resources if "k_records_" in n or "k_text_" in n]
    assert len(names) == len(NEW), names
    for n in names:
        assert any("%d%s" % (len(k), k) in n for k in NEW), n


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_built_once_without_scratch_or_spills(resources, kernel):
    hits = of(resources, kernel)
    assert len(hits) == 1, (kernel, sorted(hits))
    for name, r in hits.items():
        assert r["Scratch"] == 0 and r["VGPRSpill"] == 0 and r["SGPRSpill"] == 0, (name, r)


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_lds_and_occupancy_are_the_documented_ones(resources, kernel):
    (name, r), = of(resources, kernel).items()
    assert r["LDS"] == 0, (name, r)
    assert r["Occupancy"] == NEW[kernel], (name, r)
    assert r["VGPRs"] <= 512 // 8, (name, r)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = [l for l in open(os.path.join(root, "DESIGN.md")) if kernel in l and l.lstrip().startswith("|")]
    assert rows, "DESIGN.md §3 has no row for %s" % kernel
    assert any("no LDS" in l and "%d waves/SIMD" % NEW[kernel] in l and "%d VGPRs" % r["VGPRs"] in l for l in rows), (rows, r)


@pytest.mark.parametrize("kernel", sorted(OLD))
def test_the_kernels_beside_them_are_still_built_as_often(resources, kernel):
    assert len(of(resources, kernel)) == OLD[kernel], kernel
