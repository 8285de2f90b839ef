"""Compiler report of the kernels the strand stamp and the anchor expansion add (CPU test over kmerhash_amd/kernel_resources.json):
k_pos_strand is in the library twice (CHECK = true: the public call, CHECK = false: a stranded index), k_anchors_expand once; each keeps
its registers in registers, uses no LDS and runs at the full eight waves per SIMD, as DESIGN.md §3 states; the index kernels they sit
beside are still there in their old numbers -- no template flag was added to any of them."""
import json
import os

import pytest

from kmerhash_amd import build as B
from tests.test_kernel_resources_csr import OLD

NEW = {"k_pos_strand": 2, "k_anchors_expand": 1}
LDS_BYTES = 0
WAVES_PER_SIMD = 8


@pytest.fixture(scope="module")
def resources():
    B.build_library()
    if not os.path.exists(B.RES):
        B.build_library(force=True)
    return json.load(open(B.RES))


def of(resources, kernel):
    return {n: r for n, r in resources.items() if "%d%s" % (len(kernel), kernel) in n}      # (mangled: <length><name>)


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_built_in_the_expected_number_without_scratch_or_spills(resources, kernel):
    hits = of(resources, kernel)
    assert len(hits) == NEW[kernel], (kernel, sorted(hits))
    for name, r in hits.items():
        assert r["Scratch"] == 0 and r["VGPRSpill"] == 0 and r["SGPRSpill"] == 0, (name, r)


def test_both_forms_of_the_stamp_are_there(resources):
    names = sorted(of(resources, "k_pos_strand"))
    assert [("ILb0E" in n, "ILb1E" in n) for n in names] == [(True, False), (False, True)], names


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_lds_and_occupancy_are_the_documented_ones(resources, kernel):
    for name, r in of(resources, kernel).items():
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
def test_the_index_kernels_are_still_there_in_their_old_numbers(resources, kernel):
    assert len(of(resources, kernel)) == OLD[kernel], kernel
