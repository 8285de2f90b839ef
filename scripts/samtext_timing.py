"""write_sam against write_sam_bytes / sam_text on one MI355X: the SAM lines formatted on the host against the lines assembled on the
device.  Call-level times: host clock, device synchronised before and after the call, one warm-up, then --reps calls; all three in one
process.  Per-kernel times: device durations from torch.profiler over three calls of sam_text, in a run of their own (--per-kernel).

The workload is that of scripts/sam_timing.py: a stranded closed-syncmer index, k = 15, s = 11, of a random text of --n bases, --reads
reads of --read-bases bases, MD strings, with and without QUAL.  The two files must be equal byte for byte; the byte count is recorded.

  python scripts/samtext_timing.py --out profiles/samtext_timing.json
  python scripts/samtext_timing.py --out profiles/samtext_timing.json --per-kernel
"""
import argparse
import io
import json
import os
import statistics
import sys

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edits_timing import K, S  # noqa: E402
from minimizer_timing import genome_text, runs, summary  # noqa: E402
from select_timing import reads_of  # noqa: E402


def per_kernel(fn, torch, calls=3):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    by = {}
    for ev in prof.events():
        if ev.name.startswith(("k_", "void k_")):
            by.setdefault(ev.name.split("(")[0].replace("void ", ""), []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
    return {n: {"launches": len(v), "median_ms": round(statistics.median(v) / 1e3, 4), "sum_per_call_ms": round(sum(v) / 1e3 / calls, 4)} for n, v in sorted(by.items())}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text")
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-bases", type=int, default=150)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--per-kernel", action="store_true", help="only the profiled calls of sam_text, merged into --out")
    ap.add_argument("--tag", default="all")
    ap.add_argument("--out", default="profiles/samtext_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    if not torch.cuda.is_available():
        sys.exit("samtext_timing.py measures on a GPU; none is visible")
    text = genome_text(a.n, 0, 7, torch)
    x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
    x.build_sequences(text)
    reads, rs = reads_of(torch, text, a.reads, a.read_bases, 11)
    mp = x.map(reads, text, read_starts=rs)
    x.close()
    ends = rs + a.read_bases
    names = ["read%d" % i for i in range(a.reads)]
    names_dev = tuple(torch.from_numpy(c.view(c.dtype if c.dtype == "uint8" else "int64")).cuda() for c in kh.names_csr(names))
    qual = (33 + torch.arange(reads.numel(), device="cuda") % 41).to(torch.uint8)
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec = out.setdefault(a.tag, {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "reads": a.reads,
                                 "read_bases": a.read_bases, "text_bytes": int(text.numel()), "rows": int(mp.table.seg.numel()),
                                 "method": "host clock around the call, device synchronised before and after; one warm-up, then reps calls"})
    for label, q in (("md", None), ("md_qual", qual)):
        args = (mp, reads, text, names, rs, ends)
        kw = dict(qual=q, ref_name="ref", ref_len=a.n)
        if a.per_kernel:
            rec.setdefault(label, {})["per_kernel_sam_text"] = per_kernel(lambda: kh.sam_text(*args, **kw), torch)
            continue
        fh, bh = io.StringIO(), io.BytesIO()
        want = kh.write_sam(fh, *args, **kw)
        got = kh.write_sam_bytes(bh, *args, **kw)
        assert bh.getvalue() == fh.getvalue().encode(), "the two files differ"
        assert tuple(want) == tuple(got), (want, got)
        res = {"file_bytes": len(bh.getvalue()), "lines_skipped_unmapped": list(got), "files_equal": True,
               "write_sam": summary(runs(lambda: kh.write_sam(io.StringIO(), *args, **kw), a.reps, torch)),
               "write_sam_bytes": summary(runs(lambda: kh.write_sam_bytes(io.BytesIO(), *args, **kw), a.reps, torch)),
               "sam_text": summary(runs(lambda: kh.sam_text(*args, **kw), a.reps, torch)),
               "sam_text_names_on_device": summary(runs(lambda: kh.sam_text(mp, reads, text, names_dev, rs, ends, **kw), a.reps, torch))}
        res["write_sam_bytes_median_below_write_sam_min"] = res["write_sam_bytes"]["median_ms"] < res["write_sam"]["min_ms"]
        rec.setdefault(label, {}).update(res)
        print(label, {k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in res.items()}, flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
