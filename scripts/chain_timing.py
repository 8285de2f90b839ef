"""kh_chain_anchors on one MI355X, on the stranded closed-syncmer index (k = 15, s = 11) of a random text of --n bases (the helpers of
scripts/minimizer_timing.py).  Call-level times: host clock, device synchronised before and after the call, one warm-up, then the
median of --reps (10).  Per-kernel times: device durations from torch.profiler over three further calls, median per kernel name.
One process measures one library, the one of the package in the working directory.

  --mode all     (a) --reads (10^5) reads of --read-bases (150) cut from the text at random places, one segment per read: anchors of the
                 concatenated reads, then chain_anchors; (b) one --query-bases (10^7) query as a single segment.  Both with the byte
                 model (21 B per anchor + 16 B per kept chain at 8 TB/s) beside the measured time.
  --mode base    build_sequences of the stranded s = 11 index and anchors() of the --query-bases query: calls that exist in the parent
                 commit too, so processes started in a built checkout of the parent commit (this script given by its path) and processes
                 started here can alternate into one --out file (the timing condition: inside the spread of the parent's own repeats)

  python scripts/chain_timing.py --out profiles/chain_timing.json
  (cd ../parent && python ../here/scripts/chain_timing.py --mode base --tag parent_1 --out ../here/profiles/chain_timing.json)
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
    """median device time per kernel name over `calls` calls of fn (torch.profiler; None with the reason if it is not available)"""
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
            if "k_chain" in ev.name or "k_index_" in ev.name:
                name = ev.name.split("(")[0].split("<")[0].replace("void ", "") + ("<1>" if "k_chain_emit<1>" in ev.name else "<0>" if "k_chain_emit<0>" in ev.name else "")
                by.setdefault(name, []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        return {n: {"launches": len(v), "median_ms": round(statistics.median(v) / 1e3, 4)} for n, v in sorted(by.items())} or "no kernel events recorded"
    except Exception as e:                                  # noqa: BLE001
        return "torch.profiler not usable: %r" % (e,)


def chain_shape(kh, torch, q, r, v, seg, reps):
    from kmerhash_amd import kmers as KM
    call = lambda: KM.chain_anchors(q, r, v, K, seg)
    rec = summary(runs(call, reps, torch))
    c = call()
    m, n_chains = int(q.numel()), int(c.first.numel())
    model = (21 * m + 16 * n_chains) / HBM_BYTES_PER_MS
    rec.update(anchors=m, segments=1 if seg is None else int(seg.numel()) - 1, kept_chains=n_chains, anchors_in_kept_chains=int((c.chain >= 0).sum()),
               byte_model_ms=round(model, 4), over_byte_model=round(rec["median_ms"] / model, 1), us_per_anchor=round(rec["median_ms"] * 1e3 / max(m, 1), 4),
               per_kernel=per_kernel(call, torch))
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text")
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-bases", type=int, default=150)
    ap.add_argument("--query-bases", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mode", choices=["all", "base"], default="all")
    ap.add_argument("--tag", default=None, help="key of this process's record (default: the mode)")
    ap.add_argument("--out", default="profiles/chain_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    if not torch.cuda.is_available():
        sys.exit("chain_timing.py measures on a GPU; none is visible")
    text = genome_text(a.n, 0, 7, torch)
    q0 = a.n // 2
    query = text[q0: q0 + a.query_bases].contiguous()
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
        x.close()
        print("base", rec["build_sequences_stranded_s11"]["median_ms"], rec["anchors_query"]["median_ms"], flush=True)
    else:
        x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
        x.build_sequences(text)
        # (a) many short segments
        g = torch.Generator(device="cuda"); g.manual_seed(11)
        starts = torch.randint(0, a.n - a.read_bases, (a.reads,), dtype=torch.int64, device="cuda", generator=g)
        reads = text[(starts[:, None] + torch.arange(a.read_bases, device="cuda")[None, :]).reshape(-1)].contiguous()
        q, r, v = x.anchors(reads)
        read_starts = torch.arange(0, a.reads * a.read_bases, a.read_bases, dtype=torch.int64, device="cuda")
        seg = torch.cat([torch.searchsorted(q.long(), read_starts), torch.tensor([q.numel()], dtype=torch.int64, device="cuda")])
        rec["a_short_reads"] = dict(chain_shape(kh, torch, q, r, v, seg, a.reps), reads=a.reads, read_bases=a.read_bases,
                                    chains_call=summary(runs(lambda: x.chains(reads, read_starts=read_starts.cpu().numpy()), a.reps, torch)),
                                    anchors_call=summary(runs(lambda: x.anchors(reads), a.reps, torch)))
        print("a", rec["a_short_reads"]["median_ms"], rec["a_short_reads"]["anchors"], rec["a_short_reads"]["kept_chains"], flush=True)
        del q, r, v, seg, reads
        # (b) one long segment
        q, r, v = x.anchors(query)
        rec["b_one_segment"] = dict(chain_shape(kh, torch, q, r, v, None, a.reps), query_bases=a.query_bases)
        print("b", rec["b_one_segment"]["median_ms"], rec["b_one_segment"]["anchors"], rec["b_one_segment"]["kept_chains"], flush=True)
        x.close()
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out[a.tag or a.mode] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
