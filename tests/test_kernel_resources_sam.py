"""Compiler report of the kernels kh_record_diffs and kh_oriented_rows add (CPU test over kmerhash_amd/kernel_resources.json): each
instantiation of k_diffs_count and k_diffs_emit (cs or MD) and the two k_orient_ kernels is in the library once, keeps its registers in
registers (no scratch, no spills), uses no LDS and runs at the waves per SIMD and with the vector registers DESIGN.md §3 states -- eight
but for k_diffs_emit<KH_DIFF_CS>, whose 105 scalar registers leave seven; the record, text, scan and target kernels they sit beside are
still built, each in as many instantiations as before."""
import json
import os

import pytest

from kmerhash_amd import build as B

# (kernel, mangled template argument): waves per SIMD
NEW = {("k_diffs_count", "ILj0E"): 8, ("k_diffs_count", "ILj1E"): 8, ("k_diffs_emit", "ILj0E"): 7, ("k_diffs_emit", "ILj1E"): 8, ("k_orient_len", ""): 8,
       ("k_orient_copy", ""): 8}
OLD = {"k_records_count": 1, "k_records_emit": 1, "k_text_count": 1, "k_text_rows": 1, "k_text_emit": 1, "k_target_find": 2, "k_target_group": 2, "k_select_wave": 1,
       "k_edits_classify": 1, "k_edits_wfa": 1, "k_index_tile_sums": 1, "k_index_scan_sums": 1, "k_index_scan_apply": 2}


@pytest.fixture(scope="module")
def resources():
    B.build_library()
    if not os.path.exists(B.RES):
        B.build_library(force=True)
    return json.load(open(B.RES))


def of(resources, kernel, targ=""):
    return {n: r for n, r in resources.items() if "%d%s%s" % (len(kernel), kernel, targ) in n}      # (mangled: <length><name><template arguments>)


def test_every_new_kernel_is_a_listed_one(resources):
    names = [n for n in resources if "k_diffs_" in n or "k_orient_" in n]
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
    which = {"ILj0E": "`<KH_DIFF_CS>`: ", "ILj1E": "`<KH_DIFF_MD>`: ", "": ""}[targ] + "%d VGPRs, %d SGPRs, %d waves/SIMD" % (r["VGPRs"], r["SGPRs"], NEW[kernel, targ])
    assert any("no LDS" in l and "no scratch" in l and which in l for l in rows), (which, r)


@pytest.mark.parametrize("kernel", sorted(OLD))
def test_the_kernels_beside_them_are_still_built_as_often(resources, kernel):
    assert len(of(resources, kernel)) == OLD[kernel], kernel
