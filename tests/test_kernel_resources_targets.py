"""Compiler report of the kernels kh_anchor_targets adds (CPU test over kmerhash_amd/kernel_resources.json): each instantiation of
k_target_find (tables staged in LDS or read through L2) and of k_target_group (count or emit) is in the library once, keeps its registers
in registers (no scratch, no spills), declares no static LDS (the staged tables are dynamic LDS, sized per call) and runs at the waves
per SIMD and with the vector registers DESIGN.md §3 states; the scan and chain kernels they sit beside are still built, each in as many
instantiations as before."""
import json
import os

import pytest

from kmerhash_amd import build as B

# (kernel, mangled template argument): waves per SIMD
NEW = {("k_target_find", "ILb0E"): 8, ("k_target_find", "ILb1E"): 8, ("k_target_group", "ILb0E"): 8, ("k_target_group", "ILb1E"): 8}
OLD = {"k_records_count": 1, "k_records_emit": 1, "k_text_count": 1, "k_text_rows": 1, "k_text_emit": 1, "k_select_wave": 1, "k_select_block": 1, "k_chain_dp": 1,
       "k_chain_link": 1, "k_chain_emit": 2, "k_anchors_expand": 1, "k_index_tile_sums": 1, "k_index_scan_sums": 1, "k_index_scan_apply": 2}


@pytest.fixture(scope="module")
def resources():
    B.build_library()
    if not os.path.exists(B.RES):
        B.build_library(force=True)
    return json.load(open(B.RES))


def of(resources, kernel, targ=""):
    return {n: r for n, r in resources.items() if "%d%s%s" % (len(kernel), kernel, targ) in n}      # (mangled: <length><name><template arguments>)


def test_every_new_kernel_is_a_listed_one(resources):
    names = [n for n in resources if "k_target_" in n]
    assert len(names) == len(NEW), names
    for n in names:
        assert any("%d%s%s" % (len(k), k, t) in n for k, t in NEW), n


@pytest.mark.parametrize("kernel,targ", sorted(NEW))
def test_built_once_without_scratch_or_spills(resources, kernel, targ):
    hits = of(resources, kernel, targ)
    assert len(hits) == 1, (kernel, targ, sorted(hits))
    for name, r in hits.items():
        assert r["Scratch"] == 0 and r["VGPRSpill"] == 0 and r["SGPRSpill"] == 0, (name, r)


@pytest.mark.parametrize("kernel,targ", sorted(NEW))
def test_lds_and_occupancy_are_the_documented_ones(resources, kernel, targ):
    (name, r), = of(resources, kernel, targ).items()
    assert r["LDS"] == 0, (name, r)
    assert r["Occupancy"] == NEW[kernel, targ], (name, r)
    assert r["VGPRs"] <= 512 // 8, (name, r)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = [l for l in open(os.path.join(root, "DESIGN.md")) if kernel in l and l.lstrip().startswith("|")]
    assert rows, "DESIGN.md §3 has no row for %s" % kernel
    which = "`<%s>`: %d VGPRs" % ("true" if targ == "ILb1E" else "false", r["VGPRs"])
    lds = "no static LDS" if kernel == "k_target_find" else "no LDS"
    assert any(lds in l and "%d waves/SIMD" % NEW[kernel, targ] in l and which in l for l in rows), (rows, r)
    if kernel == "k_target_find":
        assert any("dynamic LDS" in l and "KH_TARGETS_STAGED_MAX" in l for l in rows)


@pytest.mark.parametrize("kernel", sorted(OLD))
def test_the_kernels_beside_them_are_still_built_as_often(resources, kernel):
    assert len(of(resources, kernel)) == OLD[kernel], kernel
