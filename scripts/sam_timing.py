"""kh_record_diffs, kh_oriented_rows and write_sam on one MI355X.  Call-level times: host clock, device synchronised before and after the
call, one warm-up, then the median of --reps.  Per-kernel times: device durations from torch.profiler over three further calls.

The workload is that of scripts/records_timing.py (a): a stranded closed-syncmer index, k = 15, s = 11, of a random text of --n bases,
--reads reads of --read-bases bases.  In one process: ix.map and kmers.chain_records for comparison, record_diffs of both kinds,
oriented_rows of both modes over one row per record, and write_sam split into its device calls and the host formatting (sam_lines).

  python scripts/sam_timing.py --out profiles/sam_timing.json
"""
import argparse
import io
import json
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edits_timing import K, S  # noqa: E402
from minimizer_timing import genome_text, runs, summary  # noqa: E402
from select_timing import reads_of  # noqa: E402


def per_kernel(fn, torch, calls=3):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        by = {}
        for ev in prof.events():
            if "k_diffs" in ev.name or "k_orient" in ev.name:
                by.setdefault(ev.name.split("(")[0].replace("void ", ""), []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        return {n: {"launches": len(v), "median_ms": round(statistics.median(v) / 1e3, 4)} for n, v in sorted(by.items())} or "no kernel events recorded"
    except Exception as e:                                  # noqa: BLE001
        return "torch.profiler not usable: %r" % (e,)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text")
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-bases", type=int, default=150)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sam-reps", type=int, default=3)
    ap.add_argument("--tag", default="all")
    ap.add_argument("--out", default="profiles/sam_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    from kmerhash_amd import kmers as KM
    from kmerhash_amd import sam as SM
    if not torch.cuda.is_available():
        sys.exit("sam_timing.py measures on a GPU; none is visible")
    rec = {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps"}
    text = genome_text(a.n, 0, 7, torch)
    x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
    x.build_sequences(text)
    reads, rs = reads_of(torch, text, a.reads, a.read_bases, 11)
    whole = lambda: x.map(reads, text, read_starts=rs)                                                                    # noqa: E731
    mp = whole()
    t = mp.table
    lo = torch.from_numpy(rs).cuda()[t.seg.long()].int()
    hi = lo + a.read_bases
    idx = torch.arange(t.chain.numel(), device="cuda", dtype=torch.int64)
    member = t.chain >= 0
    n_ch = int(t.seg.numel())
    first = torch.full((n_ch,), t.chain.numel(), dtype=torch.int64, device="cuda").scatter_reduce(0, t.chain[member].long(), idx[member], "amin").int()
    last = torch.zeros(n_ch, dtype=torch.int64, device="cuda").scatter_reduce(0, t.chain[member].long(), idx[member], "amax").int()
    q, r, v = t.anchors
    records = lambda: KM.chain_records(q, r, v, t.chain, mp.cigars, first, last, lo, hi, mp.ends, K, True)      # noqa: E731
    diffs = {kind: (lambda kind=kind: SM.record_diffs(reads, text, mp.records, t.rev, lo, hi, kind)) for kind in ("cs", "md")}
    rows = {name: (lambda c=c: SM.oriented_rows(reads, lo, hi, t.rev, c)) for name, c in (("seq", True), ("qual", False))}
    got = {kind: f() for kind, f in diffs.items()}
    out_rows = rows["seq"]()
    torch.cuda.synchronize()
    res = {"reads": a.reads, "read_bases": a.read_bases, "text_bytes": int(text.numel()), "rows": n_ch, "valid": int(mp.records.valid.sum()),
           "runs": int(mp.records.ops.numel()), "ok_cs": int(got["cs"].ok.sum()), "ok_md": int(got["md"].ok.sum()), "cs_bytes": int(got["cs"].text.numel()),
           "md_bytes": int(got["md"].text.numel()), "oriented_bytes": int(out_rows[1].numel()),
           "map": summary(runs(whole, a.reps, torch)), "chain_records": summary(runs(records, a.reps, torch)),
           "record_diffs_cs": summary(runs(diffs["cs"], a.reps, torch)), "record_diffs_md": summary(runs(diffs["md"], a.reps, torch)),
           "oriented_rows_seq": summary(runs(rows["seq"], a.reps, torch)), "oriented_rows_qual": summary(runs(rows["qual"], a.reps, torch)),
           "per_kernel": per_kernel(lambda: (diffs["cs"](), diffs["md"](), rows["seq"](), rows["qual"]()), torch)}
    # write_sam: the whole call, then its host half alone over the same device results
    names = ["read%d" % i for i in range(a.reads)]
    ends = rs + a.read_bases
    whole_ms, host_ms, counts = [], [], None
    for _ in range(a.sam_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        counts = SM.write_sam(io.StringIO(), mp, reads, text, names, rs, ends, ref_name="ref", ref_len=a.n)
        whole_ms.append((time.perf_counter() - t0) * 1e3)
    hm = SM._host_columns(mp)
    toff, ctext = KM.cigar_text(mp.records.offsets, mp.records.ops)
    all_lo = torch.cat([lo, torch.from_numpy(rs).cuda().int()])
    seq_rows = SM.oriented_rows(reads, all_lo, torch.cat([hi, torch.from_numpy(rs).cuda().int()]), torch.cat([t.rev, torch.zeros(a.reads, dtype=torch.uint8, device="cuda")]), True)
    torch.cuda.synchronize()
    for _ in range(a.sam_reps):
        t0 = time.perf_counter()
        SM.sam_lines(hm, toff, ctext, seq_rows, names, None, got["md"], None, "ref", a.n, unmapped=False)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    res["write_sam"] = {"lines_skipped_unmapped": list(counts), "whole_ms": [round(v, 1) for v in whole_ms], "host_formatting_ms": [round(v, 1) for v in host_ms],
                        "device_calls_and_copies_ms": round(statistics.median(whole_ms) - statistics.median(host_ms), 1)}
    rec["a"] = res
    print({k: (res[k]["median_ms"] if isinstance(res[k], dict) and "median_ms" in res[k] else res[k]) for k in res}, flush=True)
    x.close()
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out[a.tag] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
