"""Compiler report of the kernels kh_fastq_records and kh_pack_rows add (CPU test over kmerhash_amd/kernel_resources.json):
k_fastq_line_ends, k_fastq_records and k_pack_rows are in the library once each, keep their registers in registers (no scratch, no
spills), use the LDS and run at the waves per SIMD and with the registers DESIGN.md §3 states; the kernels they reuse or sit beside --
the FASTQ line counting, the scan, the copy kernels of the SAM path -- are still built, each in as many instantiations as before."""
import json
import os

import pytest

from kmerhash_amd import build as B

NEW = {"k_fastq_line_ends": (8, 16), "k_fastq_records": (8, 0), "k_pack_rows": (8, 0)}      # waves per SIMD, LDS bytes
OLD = {"k_fastq_mask": 1, "k_newline_tile_sums": 1, "k_scan_u32_to_u64": 1, "k_orient_len": 1, "k_orient_copy": 1, "k_samtext_count": 1, "k_samtext_emit": 1}


@pytest.fixture(scope="module")
def resources():
    B.build_library()
    if not os.path.exists(B.RES):
        B.build_library(force=True)
    return json.load(open(B.RES))


def of(resources, kernel):
    return {n: r for n, r in resources.items() if "%d%s" % (len(kernel), kernel) in n}      # (mangled: <length><name>)


def test_every_new_kernel_is_a_listed_one(resources):
    names = [n for n in resources if "k_fastq_line" in n or "k_fastq_rec" in n or "k_pack_" in n]
    assert len(names) == len(NEW) and all(any("%d%s" % (len(k), k) in n for k in NEW) for n in names), names


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_built_once_without_scratch_or_spills(resources, kernel):
    hits = of(resources, kernel)
    assert len(hits) == 1, (kernel, sorted(hits))
    for name, r in hits.items():
        assert r["Scratch"] == 0 and r["VGPRSpill"] == 0 and r["SGPRSpill"] == 0, (name, r)


@pytest.mark.parametrize("kernel", sorted(NEW))
def test_lds_and_occupancy_are_the_documented_ones(resources, kernel):
    (name, r), = of(resources, kernel).items()
    waves, lds = NEW[kernel]
    assert r["LDS"] == lds and r["Occupancy"] == waves and r["VGPRs"] <= 512 // 8, (name, r)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rows = [l for l in open(os.path.join(root, "DESIGN.md")) if kernel in l and l.lstrip().startswith("|")]
    assert rows, "DESIGN.md §3 has no row for %s" % kernel
    which = "%d VGPRs, %d SGPRs, %d waves/SIMD" % (r["VGPRs"], r["SGPRs"], waves)
    assert any(("%d B LDS" % lds if lds else "no LDS") in l and "no scratch" in l and which in l for l in rows), (which, r)


@pytest.mark.parametrize("kernel", sorted(OLD))
def test_the_kernels_beside_them_are_still_built_as_often(resources, kernel):
    assert len(of(resources, kernel)) == OLD[kernel], kernel
