"""Compiler report of the kernel kh_pair_chains adds (CPU test over kmerhash_amd/kernel_resources.json): k_pair_wave is in the library
once, keeps its registers in registers (no scratch, no spills), uses no LDS and runs at the waves per SIMD and with the registers
DESIGN.md §3 states; the kernels tests/test_kernel_resources_sam.py lists -- the six it calls NEW and the ones beside them -- are still
built, each in as many instantiations as before."""
import json
import os
import sys

import pytest

from kmerhash_amd import build as B

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_kernel_resources_sam import NEW as SAM_NEW, OLD as SAM_OLD  # noqa: E402

NEW = {"k_pair_wave": 8}      # kernel: waves per SIMD


@pytest.fixture(scope="module")
def resources():
    B.build_library()
    if not os.path.exists(B.RES):
        B.build_library(force=True)
    return json.load(open(B.RES))


def of(resources, kernel, targ=""):
    return {n: r for n, r in resources.items() if "%d%s%s" % (len(kernel), kernel, targ) in n}      # (mangled: <length><name><template arguments>)


def test_every_new_kernel_is_a_listed_one(resources):
    names = [n for n in resources if "k_pair_" in n]
    assert len(names) == len(NEW), names
    for n in names:
        assert any("%d%s" % (len(k), k) in n for k in NEW), n


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_built_once_without_scratch_spills_or_lds(resources, kernel):
    hits = of(resources, kernel)
    assert len(hits) == 1, (kernel, sorted(hits))
    (name, r), = hits.items()
    assert r["Scratch"] == 0 and r["VGPRSpill"] == 0 and r["SGPRSpill"] == 0 and r["LDS"] == 0, (name, r)


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_occupancy_and_registers_are_the_documented_ones(resources, kernel):
    (name, r), = of(resources, kernel).items()
    assert r["Occupancy"] == NEW[kernel], (name, r)
    assert r["VGPRs"] <= 512 // 8, (name, r)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = [l for l in open(os.path.join(root, "DESIGN.md")) if kernel in l and l.lstrip().startswith("|")]
    assert rows, "DESIGN.md §3 has no row for %s" % kernel
    which = "%d VGPRs, %d SGPRs, %d waves/SIMD" % (r["VGPRs"], r["SGPRs"], NEW[kernel])
    assert any("no LDS" in l and "no scratch" in l and which in l for l in rows), (which, r)


@pytest.mark.parametrize("kernel,targ", sorted(SAM_NEW))
def test_the_sam_kernels_are_still_built_once(resources, kernel, targ):
    assert len(of(resources, kernel, targ)) == 1, (kernel, targ)


@pytest.mark.parametrize("kernel", sorted(SAM_OLD))
def test_the_kernels_beside_them_are_still_built_as_often(resources, kernel):
    assert len(of(resources, kernel)) == SAM_OLD[kernel], kernel
