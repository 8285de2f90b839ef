"""Wide-key (16-byte) Robin Hood table timings, device-synchronised, after warm-up; prints one JSON line:
  insert_ms   : 107 374 184 distinct wide keys into an empty table (murmur3avx64, max load 0.8 reached exactly, capacity 2^27)
  find_ms     : 10^7 per-query finds, half hits
  kc63_ms     : KmerCounter(k=63) over synthetic_fastq_device reads (FASTQ text on the GPU -> 128-bit k-mers -> counting insert)
Run it on its own for timings; run it under `rocprofv3 --kernel-trace --stats -- python scripts/wide_timing.py` separately for the
kernel breakdown (profiles/)."""
import json
import sys
import time

sys.path.insert(0, ".")
import torch  # noqa: E402

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import kmers as KM  # noqa: E402


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main(reps=3):
    n, cap, nq = 107_374_184, 1 << 27, 10_000_000
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    keys = torch.randint(0, 1 << 62, (n, 2), dtype=torch.int64, device="cuda", generator=g)
    vals = torch.arange(n, dtype=torch.int32, device="cuda")
    hits = keys[torch.randint(0, n, (nq // 2,), device="cuda", generator=g)]
    miss = torch.randint(0, 1 << 62, (nq - nq // 2, 2), dtype=torch.int64, device="cuda", generator=g)
    miss[:, 1] |= 1 << 62
    q = torch.cat([hits, miss])[torch.randperm(nq, device="cuda", generator=g)].contiguous()
    ins, fnd = [], []
    for r in range(reps + 1):                 # first repetition: warm-up (allocations, code objects)
        t = kh.hashmap_robinhood_doubling_wide(cap, 0.35, 0.8)
        ms, got = timed(lambda: t.insert(keys, vals))
        assert got == n and t.capacity() == cap
        fms, (v, f) = timed(lambda: t.find_values(q))
        assert int(f.sum()) == nq // 2
        if r:
            ins.append(ms); fnd.append(fms)
        t.close()
    text, _, _ = KM.synthetic_fastq_device(400_000, 150, 2_000_000, 7, 8, 0)
    kc_ms = []
    for r in range(2):
        kc = KM.KmerCounter(k=63)
        ms, nk = timed(lambda: kc.add_fastq(text))
        if r:
            kc_ms.append(ms)
        distinct = kc.table.size()
        kc.close()
    print(json.dumps({"insert_ms": round(min(ins), 3), "insert_keys_per_s": round(n / (min(ins) / 1e3)), "find_ms": round(min(fnd), 3),
                      "find_queries_per_s": round(nq / (min(fnd) / 1e3)), "kc63_ms": round(min(kc_ms), 3), "kc63_kmers": int(nk),
                      "kc63_distinct": int(distinct), "insert_ms_all": [round(x, 3) for x in ins], "find_ms_all": [round(x, 3) for x in fnd]}))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
