"""read_fastq on a device text against the host route a user had before it, on one MI355X, in one process.  Call-level times: host
clock, device synchronised before and after the call, one warm-up, then --reps calls.  Per-kernel times: device durations from
torch.profiler over three calls of read_fastq, in a run of their own (--per-kernel).

The input is generated here: --reads simulated reads of --read-bases random bases with random qualities and names read<i>, as one
FASTQ text (2 * 10^5 reads of 150 bases: about 66 MB).  The host route: bytes.split, every fourth line, two joins, names_csr, and the
upload of seq, qual, the starts and the names CSR.  Its parts are timed as well.  The two routes must give the same bytes.

  python scripts/fastq_timing.py --out profiles/fastq_timing.json
  python scripts/fastq_timing.py --out profiles/fastq_timing.json --per-kernel
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from minimizer_timing import runs, summary  # noqa: E402
from samtext_timing import per_kernel  # noqa: E402


def fastq_text(n_reads, read_bases, seed):
    rng = np.random.RandomState(seed)
    seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(n_reads, read_bases))
    qual = rng.randint(35, 74, size=(n_reads, read_bases)).astype(np.uint8)
    return b"".join(b"@read%d 1:N:0:ACGT\n%s\n+\n%s\n" % (i, seq[i].tobytes(), qual[i].tobytes()) for i in range(n_reads))


def host_route(raw, kh, torch, parts=None):
    """-> (seq, qual, starts, (name offsets, name bytes)) on the device, the way a user made them without read_fastq"""
    t = [time.perf_counter()]
    lines = raw.split(b"\n")
    t.append(time.perf_counter())
    seqs, quals = lines[1::4], lines[3::4]
    seq, qual = b"\n".join(seqs) + b"\n", b"\n".join(quals) + b"\n"
    t.append(time.perf_counter())
    names = [l[1:].split(b" ", 1)[0].decode() for l in lines[0:len(lines) - 1:4]]
    csr = kh.names_csr(names)
    starts = np.concatenate([[0], np.cumsum(np.fromiter(map(len, seqs), dtype=np.int64, count=len(seqs)) + 1)[:-1]])
    t.append(time.perf_counter())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype)).cuda()      # noqa: E731
    out = up(np.frombuffer(seq, dtype=np.uint8)), up(np.frombuffer(qual, dtype=np.uint8)), up(starts), (up(csr[0]), up(csr[1]))
    torch.cuda.synchronize()
    t.append(time.perf_counter())
    if parts is not None:
        for name, a, b in zip(("split", "join", "names_csr_and_starts", "upload"), t, t[1:]):
            parts.setdefault(name, []).append(round((b - a) * 1e3, 3))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--read-bases", type=int, default=150)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--per-kernel", action="store_true", help="only the profiled calls of read_fastq, merged into --out")
    ap.add_argument("--tag", default="all")
    ap.add_argument("--out", default="profiles/fastq_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    if not torch.cuda.is_available():
        sys.exit("fastq_timing.py measures on a GPU; none is visible")
    raw = fastq_text(a.reads, a.read_bases, 3)
    text = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec = out.setdefault(a.tag, {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "reads": a.reads,
                                 "read_bases": a.read_bases, "text_bytes": len(raw),
                                 "method": "host clock around the call, device synchronised before and after; one warm-up, then reps calls"})
    if a.per_kernel:
        rec["per_kernel_read_fastq"] = per_kernel(lambda: kh.read_fastq(text), torch)
    else:
        r = kh.read_fastq(text)
        seq, qual, starts, names = host_route(raw, kh, torch)
        same = all(torch.equal(x, y) for x, y in ((r.seq, seq), (r.qual, qual), (r.read_starts, starts), (r.names[0], names[0]), (r.names[1], names[1])))
        assert same, "the two routes differ"
        parts = {}
        res = {"routes_equal": same, "packed_bytes": int(r.seq.numel()) * 2 + int(r.names[1].numel()),
               "read_fastq": summary(runs(lambda: kh.read_fastq(text), a.reps, torch)),
               "fastq_records": summary(runs(lambda: kh.fastq_records(text), a.reps, torch)),
               "upload_of_the_raw_text": summary(runs(lambda: torch.from_numpy(np.frombuffer(raw, dtype=np.uint8)).cuda(), a.reps, torch)),
               "host_route": summary(runs(lambda: host_route(raw, kh, torch, parts), a.reps, torch))}
        res["host_route_parts_median_ms"] = {k: summary(v[1:])["median_ms"] for k, v in parts.items()}      # (without the warm-up call)
        rec.update(res)
        print({k: (v["median_ms"] if isinstance(v, dict) and "median_ms" in v else v) for k, v in res.items()}, flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
