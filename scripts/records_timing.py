"""kh_chain_records and kh_cigar_text on one MI355X.  Call-level times: host clock, device synchronised before and after the call, one
warm-up, then the median of --reps.  Per-kernel times: device durations from torch.profiler over three further calls.

  (a) the 10^5-read workload of scripts/select_timing.py (a) (stranded closed-syncmer index, k = 15, s = 11, of a random text of --n
      bases; reads of 150 bases), in one process: ix.chain_ends followed by select_table (the entry points that existed before),
      ix.map, kmers.chain_records and kmers.cigar_text alone, and every new kernel from a profiled run
  (b) the host route -- read_cigar + extended_intervals per row -- over --host-rows rows of the same result, beside the device route
      (chain_records + cigar_text + the copy of every column to the host) over all rows

  python scripts/records_timing.py --out profiles/records_timing.json
"""
import argparse
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
            if "k_records" in ev.name or "k_text" in ev.name:
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
    ap.add_argument("--host-rows", type=int, default=1000)
    ap.add_argument("--tag", default="all")
    ap.add_argument("--out", default="profiles/records_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    from kmerhash_amd import kmers as KM
    if not torch.cuda.is_available():
        sys.exit("records_timing.py measures on a GPU; none is visible")
    rec = {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps"}
    text = genome_text(a.n, 0, 7, torch)
    x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
    x.build_sequences(text)
    reads, rs = reads_of(torch, text, a.reads, a.read_bases, 11)
    before = lambda: (lambda r: (r, KM.select_table(r[0], a.reads)))(x.chain_ends(reads, text, read_starts=rs))      # noqa: E731
    whole = lambda: x.map(reads, text, read_starts=rs)                                                                    # noqa: E731
    mp = whole()
    t = mp.table
    lo = torch.from_numpy(rs).cuda()[t.seg.long()].int()
    hi = lo + a.read_bases
    # first and last anchor of every chain from the chain numbers (the anchors of a chain ascend)
    idx = torch.arange(t.chain.numel(), device="cuda", dtype=torch.int64)
    member = t.chain >= 0
    n_ch = int(t.seg.numel())
    first = torch.full((n_ch,), t.chain.numel(), dtype=torch.int64, device="cuda").scatter_reduce(0, t.chain[member].long(), idx[member], "amin").int()
    last = torch.zeros(n_ch, dtype=torch.int64, device="cuda").scatter_reduce(0, t.chain[member].long(), idx[member], "amax").int()
    q, r, v = t.anchors
    records = lambda: KM.chain_records(q, r, v, t.chain, mp.cigars, first, last, lo, hi, mp.ends, K, True)      # noqa: E731
    got = records()
    torch.cuda.synchronize()
    assert all(torch.equal(g, e) for g, e in zip(got, mp.records)), "chain_records alone differs from the records of map()"
    texts = lambda: KM.cigar_text(got.offsets, got.ops)      # noqa: E731
    rec["a"] = {"reads": a.reads, "read_bases": a.read_bases, "text_bytes": int(text.numel()), "anchors": int(q.numel()), "chains": n_ch,
                "valid": int(got.valid.sum()), "runs": int(got.ops.numel()), "chain_ends_then_select_table": summary(runs(before, a.reps, torch)),
                "map": summary(runs(whole, a.reps, torch)), "chain_records": summary(runs(records, a.reps, torch)), "cigar_text": summary(runs(texts, a.reps, torch)),
                "per_kernel": per_kernel(lambda: (records(), texts()), torch)}
    rec["a"]["text_bytes_out"] = int(texts()[1].numel())
    rec["a"]["map_over_before"] = round(rec["a"]["map"]["median_ms"] / rec["a"]["chain_ends_then_select_table"]["median_ms"], 4)
    print("a", {k: rec["a"][k]["median_ms"] for k in ("chain_ends_then_select_table", "map", "chain_records", "cigar_text")}, rec["a"]["per_kernel"], flush=True)

    def device_route():
        g = records()
        to, tx = KM.cigar_text(g.offsets, g.ops)
        return [z.cpu() for z in g] + [to.cpu(), tx.cpu()]

    rows = min(a.host_rows, n_ch)
    mh = KM.Mapping(*(type(p)(*((tuple(z.cpu().numpy() for z in f) if isinstance(f, tuple) else f.cpu().numpy()) for f in p)) for p in mp))      # the host helpers on host arrays
    t0 = time.perf_counter()
    for row in range(rows):
        KM.read_cigar(mh.cigars, mh.ends, mh.table, row, K)
    KM.extended_intervals(mh.table, mh.ends)
    host_ms = (time.perf_counter() - t0) * 1e3
    rec["b"] = {"host_rows": rows, "host_route_ms": round(host_ms, 1), "host_ms_per_row": round(host_ms / rows, 3), "device_route_all_rows": summary(runs(device_route, a.reps, torch)),
                "rows": n_ch}
    rec["b"]["per_row_ratio"] = round(rec["b"]["host_ms_per_row"] / (rec["b"]["device_route_all_rows"]["median_ms"] / n_ch), 1)
    print("b", rec["b"], flush=True)
    x.close()
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out[a.tag] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
