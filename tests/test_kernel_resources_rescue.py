"""Compiler report of the kernels kh_mate_rescue adds (CPU test over kmerhash_amd/kernel_resources.json): the five instantiations of
k_rescue_scan, k_rescue_wfa and k_rescue_emit are in the library once each, keep their registers in registers (no scratch, no spills),
use no LDS and have the registers and waves per SIMD that DESIGN.md §3 states; the kernels whose device functions they share --
k_ends_wfa, k_ends_emit, k_cigar_wfa, k_cigar_emit, k_edits_wfa -- are still built once each."""
import json
import os

import pytest

from kmerhash_amd import build as B

NEW = {("k_rescue_scan", "ILi1EE"): 8, ("k_rescue_scan", "ILi2EE"): 8, ("k_rescue_scan", "ILi3EE"): 7, ("k_rescue_scan", "ILi4EE"): 5, ("k_rescue_scan", "ILi8EE"): 3,
       ("k_rescue_wfa", ""): 8, ("k_rescue_emit", ""): 8}      # (kernel, template arguments): waves per SIMD
SHARED = ("k_ends_wfa", "k_ends_emit", "k_cigar_wfa", "k_cigar_emit", "k_edits_wfa")


@pytest.fixture(scope="module")
def resources():
    B.build_library()
    if not os.path.exists(B.RES):
        B.build_library(force=True)
    return json.load(open(B.RES))


def of(resources, kernel, targ=""):
    return {n: r for n, r in resources.items() if "%d%s%s" % (len(kernel), kernel, targ) in n}      # (mangled: <length><name><template arguments>)


def test_every_new_kernel_is_a_listed_one(resources):
    names = [n for n in resources if "k_rescue_" in n]
    assert len(names) == len(NEW), names
    for n in names:
        assert any("%d%s%s" % (len(k), k, t) in n for k, t in NEW), n


@pytest.mark.parametrize("kernel,targ", sorted(NEW))
def test_built_once_without_scratch_spills_or_lds_at_the_documented_occupancy(resources, kernel, targ):
    hits = of(resources, kernel, targ)
    assert len(hits) == 1, (kernel, targ, sorted(hits))
    (name, r), = hits.items()
    assert r["Scratch"] == 0 and r["VGPRSpill"] == 0 and r["SGPRSpill"] == 0 and r["LDS"] == 0, (name, r)
    assert r["Occupancy"] == NEW[kernel, targ], (name, r)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = [l for l in open(os.path.join(root, "DESIGN.md")) if kernel in l and l.lstrip().startswith("|")]
    assert rows, "DESIGN.md §3 has no row for %s" % kernel
    which = "%d VGPRs, %d SGPRs, %d waves/SIMD" % (r["VGPRs"], r["SGPRs"], NEW[kernel, targ])
    assert any("no lds" in l.lower() and "no scratch" in l.lower() and which in l for l in rows), (which, r)


@pytest.mark.parametrize("kernel", SHARED)
def test_the_kernels_that_share_their_device_functions_are_still_built_once(resources, kernel):
    assert len(of(resources, kernel)) == 1, kernel
