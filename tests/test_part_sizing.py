"""CPU: the sub-slot sizing of the histogram-free partition (kmerhash_amd/csrc/kh_part_sizing.h) as a stand-alone host program:
the benchmark shape, the fall-back conditions (fewer than eight buckets or digits, a slot that does not divide by eight, an eighth of
the slot below mean + 7 sigma, fewer tiles per sub-slot than asked) and the invariants the kernels rely on over a sweep of shapes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_part_sizing_stand_alone(tmp_path):
    exe = tmp_path / "test_part_sizing"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "test_part_sizing.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "part sizing ok" in r.stdout, r.stdout + r.stderr
