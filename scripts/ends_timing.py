"""kh_chain_ends on one MI355X, on the workloads (a), (c), (d) and (e) of scripts/cigars_timing.py (the stranded closed-syncmer index,
k = 15, s = 11, of a random text of --n bases).  Call-level times: host clock, device synchronised before and after the call, one
warm-up, then the median of --reps.  Per-kernel times: device durations from torch.profiler over three further calls.  One process
measures one library, the one of the package in the working directory (KH_LIB_SUFFIX picks a library built beside it).

  --mode all     per workload: kmers.chain_ends alone (count pass + emit pass, as the Python call makes them), kmers.chain_cigars over the
                 same anchors beside it, the ends that align, clip and hold edits, and the k_ends_* kernels one by one
  --mode base    build_sequences, anchors() of the query, chains(), chain_edits() and chain_cigars() of the reads: calls that exist in
                 the parent commit too, so processes on the parent's library and processes on this one can alternate into one --out file

  python scripts/ends_timing.py --out profiles/ends_timing.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edits_timing import K, S, mutated  # noqa: E402
from minimizer_timing import genome_text, runs, summary, timed  # noqa: E402


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
            if "k_ends" in ev.name or "k_index_scan" in ev.name or "k_index_tile" in ev.name:
                by.setdefault(ev.name.split("(")[0].replace("void ", ""), []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        return {n: {"launches": len(v), "median_ms": round(statistics.median(v) / 1e3, 4)} for n, v in sorted(by.items())} or "no kernel events recorded"
    except Exception as e:                                  # noqa: BLE001
        return "torch.profiler not usable: %r" % (e,)


def ends_shape(torch, qtext, rtext, q, r, v, seg, cuts, n_text, reps):
    """cuts: the start of every segment in qtext (None: one segment)"""
    from kmerhash_amd import kmers as KM
    c = KM.chain_anchors(q, r, v, K, seg)
    nc = int(c.first.numel())
    if seg is None:
        lo, hi = torch.zeros(nc, dtype=torch.int32, device="cuda"), torch.full((nc,), n_text, dtype=torch.int32, device="cuda")
    else:
        sg = torch.searchsorted(seg, c.first.long(), right=True) - 1
        lo, hi = cuts[sg].int(), torch.cat([cuts[1:], torch.tensor([n_text], dtype=torch.int64, device="cuda")])[sg].int()
    e = KM.chain_edits(qtext, rtext, q, r, v, c.pred, c.chain, nc, K)
    cigars = lambda: KM.chain_cigars(qtext, rtext, q, r, v, c.pred, c.chain, nc, K, e.link)          # noqa: E731
    call = lambda: KM.chain_ends(qtext, rtext, q, r, v, c.first, c.last, lo, hi, K)                  # noqa: E731
    rec = summary(runs(call, reps, torch))
    rec["chain_cigars"] = summary(runs(cigars, reps, torch))
    g = call()
    torch.cuda.synchronize()
    n = (g.q + g.clip)
    rec.update(anchors=int(q.numel()), kept_chains=nc, ends=2 * nc, ends_with_bases=int((n > 0).sum()), ends_with_edits=int((g.edits > 0).sum()),
               ends_clipped=int((g.clip > 0).sum()), bases_aligned=int(g.q.sum()), bases_clipped=int(g.clip.sum()), edits_total=int(g.edits.sum()),
               runs=int(g.ops.numel()), over_chain_cigars=round(rec["median_ms"] / rec["chain_cigars"]["median_ms"], 2), per_kernel=per_kernel(call, torch))
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text")
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-bases", type=int, default=150)
    ap.add_argument("--query-bases", type=int, default=10_000_000)
    ap.add_argument("--segment-bases", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mode", choices=["all", "base"], default="all")
    ap.add_argument("--tag", default=None, help="key of this process's record (default: the mode)")
    ap.add_argument("--out", default="profiles/ends_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    if not torch.cuda.is_available():
        sys.exit("ends_timing.py measures on a GPU; none is visible")
    text = genome_text(a.n, 0, 7, torch)
    q0 = a.n // 2
    query = text[q0: q0 + a.query_bases].contiguous()
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    starts = torch.randint(0, a.n - a.read_bases, (a.reads,), dtype=torch.int64, device="cuda", generator=g)
    reads = text[(starts[:, None] + torch.arange(a.read_bases, device="cuda")[None, :]).reshape(-1)].contiguous()
    read_starts = torch.arange(0, a.reads * a.read_bases, a.read_bases, dtype=torch.int64, device="cuda")
    rs = read_starts.cpu().numpy()
    rec = {"version": kh._capi.lib().kh_version().decode(), "library": os.path.basename(kh._capi.LIB), "device": torch.cuda.get_device_name(0), "text_bytes": a.n,
           "reps": a.reps, "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps"}
    x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
    if a.mode == "base":
        out = []
        for _ in range(a.reps + 1):
            y = kh.KmerPositionIndex(k=K, s=S, stranded=True)
            ms, _r = timed(lambda: y.build_sequences(text), torch)
            out.append(round(ms, 3))
            y.close()
        x.build_sequences(text)
        rec["build_sequences_stranded_s11"] = summary(out[1:])
        rec["anchors_query"] = summary(runs(lambda: x.anchors(query), a.reps, torch))
        rec["chains_reads"] = summary(runs(lambda: x.chains(reads, read_starts=rs), a.reps, torch))
        rec["chain_edits_reads"] = summary(runs(lambda: x.chain_edits(reads, text, read_starts=rs), a.reps, torch))
        rec["chain_cigars_reads"] = summary(runs(lambda: x.chain_cigars(reads, text, read_starts=rs), a.reps, torch))
        print("base", *(rec[n]["median_ms"] for n in ("build_sequences_stranded_s11", "anchors_query", "chains_reads", "chain_edits_reads", "chain_cigars_reads")), flush=True)
    else:
        x.build_sequences(text)
        q, r, v = x.anchors(reads)
        seg = torch.cat([torch.searchsorted(q.long(), read_starts), torch.tensor([q.numel()], dtype=torch.int64, device="cuda")])
        rec["a_short_reads"] = dict(ends_shape(torch, reads, text, q, r, v, seg, read_starts, int(reads.numel()), a.reps), reads=a.reads, read_bases=a.read_bases)
        rec["a_short_reads"]["chain_ends_call"] = summary(runs(lambda: x.chain_ends(reads, text, read_starts=rs), a.reps, torch))
        rec["a_short_reads"]["chain_cigars_call"] = summary(runs(lambda: x.chain_cigars(reads, text, read_starts=rs), a.reps, torch))
        print("a", rec["a_short_reads"]["median_ms"], rec["a_short_reads"]["chain_cigars"]["median_ms"], rec["a_short_reads"]["ends_with_bases"], flush=True)
        del q, r, v, seg
        for key, rate in (("c_query_1pct", 0.01), ("d_query_10pct", 0.10)):
            qt = mutated(torch, query, rate, 5)
            q, r, v = x.anchors(qt)
            rec[key] = dict(ends_shape(torch, qt, text, q, r, v, None, None, a.query_bases, max(3, a.reps // 2)), query_bases=a.query_bases, substitution_rate=rate)
            print(key, rec[key]["median_ms"], rec[key]["chain_cigars"]["median_ms"], rec[key]["ends"], flush=True)
            del q, r, v
        qt = mutated(torch, query, 0.01, 5)
        q, r, v = x.anchors(qt)
        cuts = torch.arange(0, a.query_bases, a.segment_bases, dtype=torch.int64, device="cuda")
        seg = torch.cat([torch.searchsorted(q.long(), cuts), torch.tensor([q.numel()], dtype=torch.int64, device="cuda")])
        rec["e_query_1pct_segments"] = dict(ends_shape(torch, qt, text, q, r, v, seg, cuts, a.query_bases, max(3, a.reps // 2)), query_bases=a.query_bases,
                                            substitution_rate=0.01, segment_bases=a.segment_bases)
        print("e", rec["e_query_1pct_segments"]["median_ms"], rec["e_query_1pct_segments"]["chain_cigars"]["median_ms"], rec["e_query_1pct_segments"]["ends"], flush=True)
        del q, r, v, seg
    x.close()
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out[a.tag or a.mode] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
