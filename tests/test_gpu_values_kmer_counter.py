"""GPU: benchmark/kmer_counter.py --histo / --min-count for 64-bit (k = 31) and 16-byte (k = 63) k-mers: the spectrum file parses and its
counts sum to the number of distinct k-mers before the filter, --verify accepts the spectrum predicted from the read positions and the
size that survives --min-count; one more run on a single rank with the collectives forced, so that the spectrum's all-reduce runs over
RCCL."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags, force=False):
    env = {k: v for k, v in os.environ.items() if k != "KH_DIST_FORCE_COLLECTIVES"}
    if force:
        env["KH_DIST_FORCE_COLLECTIVES"] = "1"
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run([sys.executable, os.path.join(ROOT, "benchmark", "kmer_counter.py")] + list(flags), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          universal_newlines=True, timeout=800, env=env)


def _parse_histo(path, nbins):
    """{count: number}; the overflow bin is the line '>=nbins-1'"""
    out = {}
    for line in open(path).read().splitlines():
        c, n = line.split("\t")
        if c.startswith(">="):
            assert int(c[2:]) == nbins - 1
            c = c[2:]
        assert int(c) not in out and int(n) > 0
        out[int(c)] = int(n)
    assert list(out) == sorted(out)
    return out


def _check(k, tmp_path, force=False, bins=None):
    histo = str(tmp_path / ("spectrum_%d.tsv" % k))
    flags = ["-k", str(k), "--reads", "40000", "--genome", "300000", "--batches", "4", "--verify", "--histo", histo, "--min-count", "2"]
    if bins is not None:
        flags += ["--histo-bins", str(bins)]
    if force:
        flags += ["--gpus", "1"]
    r = _run(*flags, force=force)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["ok"] and d["verify"]["ok"] and d["verify"]["spectrum_ok"] and d["min_count"]["ok"], d
    spec = _parse_histo(histo, bins or 256)
    assert sum(spec.values()) == d["distinct_global"] == d["verify"]["expected_distinct"]        # the size BEFORE the filter
    assert 0 not in spec and 1 in spec and 2 in spec
    if bins is None:
        assert sum(c * n for c, n in spec.items()) == d["verify"]["total_kmers"]                # (no count reaches the overflow bin here)
    assert d["min_count"]["n"] == 2 and d["min_count"]["size_after"] == d["min_count"]["expected_size"] == d["distinct_global"] - spec[1]
    assert d["min_count"]["dropped_rank0"] == spec[1]
    return d, spec


@pytest.mark.parametrize("k", [31, 63])
def test_histo_and_min_count_verify(k, tmp_path):
    _check(k, tmp_path)


def test_histo_over_rccl_on_one_rank_with_forced_collectives(tmp_path):
    d, spec = _check(31, tmp_path, force=True, bins=4)
    assert d["n_gpus"] == 1 and max(spec) == 3                                                # coverage 20: the overflow bin '>=3' is used
