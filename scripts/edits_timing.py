"""kh_chain_edits on one MI355X, on the stranded closed-syncmer index (k = 15, s = 11) of a random text of --n bases (the workloads of
scripts/chain_timing.py, the helpers of scripts/minimizer_timing.py).  Call-level times: host clock, device synchronised before and
after the call, one warm-up, then the median of --reps (10).  Per-kernel times: device durations from torch.profiler over three
further calls.  One process measures one library, the one of the package in the working directory.

  --mode all     (a) --reads (10^5) reads of --read-bases (150) cut from the text, one segment per read; (b) one --query-bases (10^7)
                 query as a single segment; (c), (d) that query with every base substituted at 1 % and at 10 %, so that the worklist of
                 the wavefront kernel is not empty; (e) the 1 % query cut into segments of --segment-bases (1000), so that the
                 links with edits belong to many chains.  chain_edits over the anchors, pred and chain of chain_anchors; links, worklist
                 share (links with a distance > 0 or over) and the byte model beside the measured time.
  --mode base    build_sequences, anchors() of the query and chains() of the reads: calls that exist in the parent commit too, so
                 processes started in a built checkout of the parent commit (this script given by its path) and processes started here
                 can alternate into one --out file (the timing condition: inside the spread of the parent's own repeats)

  python scripts/edits_timing.py --out profiles/edits_timing.json
  (cd ../parent && python ../here/scripts/edits_timing.py --mode base --tag parent_1 --out ../here/profiles/edits_timing.json)
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from minimizer_timing import genome_text, runs, summary, timed  # noqa: E402

K, S = 15, 11
HBM_BYTES_PER_MS = 8e9          # 8 TB/s


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
            if "k_edits" in ev.name:
                by.setdefault(ev.name.split("(")[0].replace("void ", ""), []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        return {n: {"launches": len(v), "median_ms": round(statistics.median(v) / 1e3, 4)} for n, v in sorted(by.items())} or "no kernel events recorded"
    except Exception as e:                                  # noqa: BLE001
        return "torch.profiler not usable: %r" % (e,)


def edits_shape(torch, qtext, rtext, q, r, v, seg, reps):
    from kmerhash_amd import kmers as KM
    c = KM.chain_anchors(q, r, v, K, seg)
    nc = int(c.first.numel())
    call = lambda: KM.chain_edits(qtext, rtext, q, r, v, c.pred, c.chain, nc, K)
    rec = summary(runs(call, reps, torch))
    e = call()
    torch.cuda.synchronize()
    link = e.link
    links, bases = int((link != -1).sum()), int((q - q[c.pred.clamp(min=0).long()])[link != -1].sum())
    # per anchor 17 B of arrays read (+ 13 B of its predecessor's, mostly the neighbour's cache lines) and 4 B written; per link its two strings
    model = (21 * int(q.numel()) + 2 * bases) / HBM_BYTES_PER_MS
    rec.update(anchors=int(q.numel()), kept_chains=nc, links=links, link_bases=bases, links_exact=int((link == 0).sum()), links_with_edits=int((link > 0).sum()),
               links_over=int((link == -2).sum()), edits_total=int(e.edits.sum()), byte_model_ms=round(model, 4), over_byte_model=round(rec["median_ms"] / model, 1),
               us_per_link=round(rec["median_ms"] * 1e3 / max(links, 1), 5), per_kernel=per_kernel(call, torch))
    return rec


def mutated(torch, text, rate, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    hit = torch.rand(text.numel(), device="cuda", generator=g) < rate
    code = ((text >> 1) & 3).long()                          # A 0, C 1, T 2, G 3
    other = torch.tensor([65, 67, 84, 71], dtype=torch.uint8, device="cuda")[(code + torch.randint(1, 4, (text.numel(),), device="cuda", generator=g)) & 3]
    return torch.where(hit, other, text).contiguous()


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
    ap.add_argument("--out", default="profiles/edits_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    if not torch.cuda.is_available():
        sys.exit("edits_timing.py measures on a GPU; none is visible")
    text = genome_text(a.n, 0, 7, torch)
    q0 = a.n // 2
    query = text[q0: q0 + a.query_bases].contiguous()
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    starts = torch.randint(0, a.n - a.read_bases, (a.reads,), dtype=torch.int64, device="cuda", generator=g)
    reads = text[(starts[:, None] + torch.arange(a.read_bases, device="cuda")[None, :]).reshape(-1)].contiguous()
    read_starts = torch.arange(0, a.reads * a.read_bases, a.read_bases, dtype=torch.int64, device="cuda")
    rec = {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "text_bytes": a.n, "reps": a.reps,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps"}
    if a.mode == "base":
        out = []
        for _ in range(a.reps + 1):
            x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
            ms, _r = timed(lambda: x.build_sequences(text), torch)
            out.append(round(ms, 3))
            x.close()
        x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
        x.build_sequences(text)
        rec["build_sequences_stranded_s11"] = summary(out[1:])
        rec["anchors_query"] = summary(runs(lambda: x.anchors(query), a.reps, torch))
        rs = read_starts.cpu().numpy()
        rec["chains_reads"] = summary(runs(lambda: x.chains(reads, read_starts=rs), a.reps, torch))
        x.close()
        print("base", rec["build_sequences_stranded_s11"]["median_ms"], rec["anchors_query"]["median_ms"], rec["chains_reads"]["median_ms"], flush=True)
    else:
        x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
        x.build_sequences(text)
        q, r, v = x.anchors(reads)
        seg = torch.cat([torch.searchsorted(q.long(), read_starts), torch.tensor([q.numel()], dtype=torch.int64, device="cuda")])
        # B of a read's links lies in the text the reads were cut from
        rec["a_short_reads"] = dict(edits_shape(torch, reads, text, q, r, v, seg, a.reps), reads=a.reads, read_bases=a.read_bases)
        rs = read_starts.cpu().numpy()
        rec["a_short_reads"]["chain_edits_call"] = summary(runs(lambda: x.chain_edits(reads, text, read_starts=rs), a.reps, torch))
        rec["a_short_reads"]["chains_call"] = summary(runs(lambda: x.chains(reads, read_starts=rs), a.reps, torch))
        print("a", rec["a_short_reads"]["median_ms"], rec["a_short_reads"]["links"], flush=True)
        del q, r, v, seg
        for key, rate in (("b_one_segment", 0.0), ("c_query_1pct", 0.01), ("d_query_10pct", 0.10)):
            qt = mutated(torch, query, rate, 5) if rate else query
            q, r, v = x.anchors(qt)
            rec[key] = dict(edits_shape(torch, qt, text, q, r, v, None, max(3, a.reps // 2)), query_bases=a.query_bases, substitution_rate=rate)
            print(key, rec[key]["median_ms"], rec[key]["links"], rec[key]["links_with_edits"], rec[key]["links_over"], flush=True)
            del q, r, v
        # (e) the 1 % query again, cut into segments of --segment-bases: the same links spread over many chains, so the per-chain sums
        # no longer meet in one counter (the worklist counter still is one address)
        qt = mutated(torch, query, 0.01, 5)
        q, r, v = x.anchors(qt)
        cuts = torch.arange(0, a.query_bases, a.segment_bases, dtype=torch.int64, device="cuda")
        seg = torch.cat([torch.searchsorted(q.long(), cuts), torch.tensor([q.numel()], dtype=torch.int64, device="cuda")])
        rec["e_query_1pct_segments"] = dict(edits_shape(torch, qt, text, q, r, v, seg, max(3, a.reps // 2)), query_bases=a.query_bases, substitution_rate=0.01,
                                            segment_bases=a.segment_bases)
        print("e", rec["e_query_1pct_segments"]["median_ms"], rec["e_query_1pct_segments"]["kept_chains"], rec["e_query_1pct_segments"]["links_with_edits"], flush=True)
        del q, r, v, seg
        x.close()
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out[a.tag or a.mode] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
