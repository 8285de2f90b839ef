"""CPU: the scratch carver (kmerhash_amd/csrc/kh_scratch.h) as a stand-alone host program: over a sweep of three-array layouts with
counts 0, 1, 63, 64, 65 and 2^32 + 1 and element sizes 1, 4, 8 and 16 the measured size is where the carving pass ends, every array
is 256-byte aligned and inside the block, non-empty arrays are disjoint and follow one another in the order taken, and an array of
zero elements is null and consumes nothing.  Built with the address and undefined-behaviour sanitizers where the toolchain links them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_scratch.cpp")
BASE = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror"]


def test_scratch_layout_stand_alone(tmp_path):
    exe = tmp_path / "test_scratch"
    r = subprocess.run(BASE + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0:      # a toolchain without the sanitizer runtimes: the same program without them
        r = subprocess.run(BASE + [SRC, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scratch layout ok" in r.stdout, r.stdout + r.stderr
