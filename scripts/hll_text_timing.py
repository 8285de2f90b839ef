"""The fused text -> HyperLogLog pass next to the two-step route it replaces, on one MI355X: FASTQ text of 2 x 10^6 reads of 150 bases
(synthetic_fastq_fixed, 642 MB on the device), k = 31 and k = 63, farm hash, precision 12.  Call-level times (host clock around calls
that end in a device synchronise), one warm-up repetition, then `reps` repetitions ALTERNATING the two routes; median, min and max:
  fused      : hyperloglog64.update_from_fastq(text, k)
  two_step   : k = 31: kmers_from_fastq + update;  k = 63: kmers128_from_fastq + hash_batch_wide + update_via_hashval
               (the route that existed before update_wide / update_from_fastq)
and, for k = 63, KmerCounter.add_fastq of the same text with and without reserve_from_estimate (a fresh counter per repetition).
The registers of the two routes are compared at the size that is timed.  Bytes moved per route follow the traffic model of DESIGN §3.
Writes profiles/hll_text_timing.json (or the path given) and prints it."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import kmers as KM  # noqa: E402
from kmerhash_amd.hll import hyperloglog64  # noqa: E402

READS, READ_LEN, HASH = 2_000_000, 150, "farm"


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3), "all_ms": [round(x, 3) for x in xs]}


def alternate(fa, fb, reps):
    """reps + 1 rounds of (fa, fb); the first round is the warm-up"""
    a, b = [], []
    for r in range(reps + 1):
        ta, tb = timed(fa)[0], timed(fb)[0]
        if r:
            a.append(ta); b.append(tb)
    return stats(a), stats(b)


def estimator_routes(text, k, reps):
    fused, two = hyperloglog64(12, 0, HASH, 43), hyperloglog64(12, 0, HASH, 43)

    def two_step():
        if k <= 32:
            two.update(KM.kmers_from_fastq(text, k, True))
        else:
            two.update_via_hashval(kh.hash_batch_wide(kh.kmers128_from_fastq(text, k, True), HASH, 43))

    n_kmers = fused.update_from_fastq(text, k, True)
    two_step()
    same = bool(np.array_equal(fused.registers(), two.registers()))
    sf, st = alternate(lambda: fused.update_from_fastq(text, k, True), two_step, reps)
    n = int(text.numel())
    kb = 8 if k <= 32 else 16
    # FASTQ: both routes read the text twice for the line structure and write + read the masked copy (4 B per text byte); then the
    # fused pass is done, the two-step route reads the masked text once more (count pass), writes the k-mers, and reads them again
    # (k > 32: + 8 B of hashes written and read)
    res = {"k": k, "kmers": int(n_kmers), "text_bytes": n, "registers_equal": same, "estimate": fused.estimate(),
           "fused": sf, "two_step": st, "ratio_two_step_over_fused": round(st["median_ms"] / sf["median_ms"], 2),
           "model_bytes_fused": 4 * n, "model_bytes_two_step": 5 * n + int(n_kmers) * (2 * kb + (16 if k > 32 else 0))}
    res["fused_text_GBps"] = round(n / sf["median_ms"] / 1e6, 1)
    fused.close(); two.close()
    return res


def counter_routes(text, k, reps):
    def build(reserve):
        kc = KM.KmerCounter(k, reserve_from_estimate=reserve)
        kc.add_fastq(text)
        out = (kc.table.size(), kc.table.capacity())
        kc.close()
        return out
    a, b = build(True), build(False)
    sr, sp = alternate(lambda: build(True), lambda: build(False), reps)
    return {"k": k, "distinct": a[0], "same_size": a[0] == b[0], "capacity_reserved": a[1], "capacity_doubling": b[1],
            "add_fastq_reserve_from_estimate": sr, "add_fastq_doubling": sp,
            "ratio_doubling_over_reserve": round(sp["median_ms"] / sr["median_ms"], 2)}


def main(argv):
    quick = "--quick" in argv
    paths = [a for a in argv if not a.startswith("--")]
    out = paths[0] if paths else os.path.join("profiles", "hll_text_timing.json")
    reps = 3 if quick else 7
    reads = READS // 10 if quick else READS
    text = torch.from_numpy(KM.synthetic_fastq_fixed(reads, READ_LEN, 20_000_000)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "reads": reads, "read_len": READ_LEN, "hash": HASH, "reps": reps,
           "k31": estimator_routes(text, 31, reps), "k63": estimator_routes(text, 63, reps), "counter_k63": counter_routes(text, 63, reps)}
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
