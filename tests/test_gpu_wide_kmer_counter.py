"""GPU: benchmark/kmer_counter.py at k = 63 -- the wide backend behind the driver: insert batches, --verify against the 128-bit prediction
from the read positions, --cycle, --out (16 + 2 bytes per tuple); --hll-reserve is refused with a message, not run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*flags):
    env = {k: v for k, v in os.environ.items() if k != "KH_DIST_FORCE_COLLECTIVES"}
    return subprocess.run([sys.executable, os.path.join(ROOT, "benchmark", "kmer_counter.py")] + list(flags), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          universal_newlines=True, timeout=800, env=env)


def test_kmer_counter_k63_verify_cycle_out(tmp_path):
    out = str(tmp_path / "counts.bin")
    r = _run("-k", "63", "--reads", "40000", "--genome", "300000", "--batches", "3", "--cycle", "--verify", "--sample-ratio", "50", "--out", out)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["k"] == 63 and d["ok"] and d["verify"]["ok"] and d["cycle"]["ok"], d
    assert d["verify"]["sample_mismatches"] == 0 and d["verify"]["total_kmers"] == 40000 * (150 - 63 + 1) == d["verify"]["expected_total"]
    assert d["distinct_global"] == d["verify"]["expected_distinct"] > 100_000
    assert 0 < d["cycle"]["queries_local"] == d["cycle"]["count_hits"] == d["cycle"]["find_hits"] and d["cycle"]["count_hits_after"] == 0
    rec = np.fromfile(out, dtype=np.dtype([("kmer", "<u8", (2,)), ("count", "<u2")]))
    assert os.path.getsize(out) == 18 * len(rec) and len(rec) == d["cycle"]["size_after"]
    assert rec["count"].min() >= 1 and (rec["kmer"][:, 1] >> np.uint64(62)).max() == 0        # k = 63: 126 bits
    assert len(np.unique(rec["kmer"], axis=0)) == len(rec)


def test_kmer_counter_k63_refuses_hll_reserve():
    r = _run("-k", "63", "--reads", "1000", "--genome", "100000", "--batches", "1", "--hll-reserve")
    assert r.returncode != 0 and "--hll-reserve" in r.stderr and not r.stdout.strip()
