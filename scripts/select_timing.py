"""kh_chain_select on one MI355X.  Call-level times: host clock, device synchronised before and after the call, one warm-up, then the
median of --reps.  Per-kernel times: device durations from torch.profiler over three further calls.

  (a) the 10^5-read workload of scripts/ends_timing.py (stranded closed-syncmer index, k = 15, s = 11, of a random text of --n bases;
      reads of 150 bases): mostly one chain per read -- the floor of the call
  (b) reads against a reference in which every block occurs 4 and 16 times with 2 % substitutions: several chains per read, still a
      wavefront per read (10^5 reads at 4 copies, a quarter of them at 16: chain_anchors takes 2^24 anchors per call)
  (c) one group of 10^4 and of 10^5 chains with random intervals and scores: the workgroup path (LDS tile and scratch)
For (a) and (b): kmers.select_chains alone over the chain table, and ix.chain_select end to end beside ix.chains on the same input.

  python scripts/select_timing.py --out profiles/select_timing.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edits_timing import K, S, mutated  # noqa: E402
from minimizer_timing import genome_text, runs, summary  # noqa: E402


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
            if "k_select" in ev.name:
                by.setdefault(ev.name.split("(")[0].replace("void ", ""), []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        return {n: {"launches": len(v), "median_ms": round(statistics.median(v) / 1e3, 4)} for n, v in sorted(by.items())} or "no kernel events recorded"
    except Exception as e:                                  # noqa: BLE001
        return "torch.profiler not usable: %r" % (e,)


def reads_of(torch, text, n_reads, read_bases, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    starts = torch.randint(0, text.numel() - read_bases, (n_reads,), dtype=torch.int64, device="cuda", generator=g)
    reads = text[(starts[:, None] + torch.arange(read_bases, device="cuda")[None, :]).reshape(-1)].contiguous()
    return reads, torch.arange(0, n_reads * read_bases, read_bases, dtype=torch.int64).numpy()


def index_shape(torch, kh, text, n_reads, read_bases, reps):
    from kmerhash_amd import kmers as KM
    x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
    x.build_sequences(text)
    reads, rs = reads_of(torch, text, n_reads, read_bases, 11)
    table = x.chains(reads, read_starts=rs)
    offs = torch.searchsorted(table.seg.long(), torch.arange(n_reads + 1, dtype=torch.int64, device="cuda"))
    alone = lambda: KM.select_chains(table.q_start, table.q_end, table.score, table.count, offs)      # noqa: E731
    rec = {"select_chains": summary(runs(alone, reps, torch)), "chains": summary(runs(lambda: x.chains(reads, read_starts=rs), reps, torch)),
           "chain_select": summary(runs(lambda: x.chain_select(reads, read_starts=rs), reps, torch))}
    sel = alone()
    torch.cuda.synchronize()
    per_read = (offs[1:] - offs[:-1])
    rec.update(reads=n_reads, read_bases=read_bases, text_bytes=int(text.numel()), chains_total=int(table.score.numel()),
               reads_without_chains=int((per_read == 0).sum()), max_chains_per_read=int(per_read.max()), primaries=int((sel.flag & 1).sum()),
               kept=int(((sel.flag >> 1) & 1).sum()), mapq_60=int((sel.mapq == 60).sum()), mapq_0_primaries=int(((sel.mapq == 0) & ((sel.flag & 1) == 1)).sum()),
               select_over_chains=round(rec["select_chains"]["median_ms"] / rec["chains"]["median_ms"], 4),
               chain_select_over_chains=round(rec["chain_select"]["median_ms"] / rec["chains"]["median_ms"], 4), per_kernel=per_kernel(alone, torch))
    x.close()
    return rec


def one_group(torch, n, reps):
    from kmerhash_amd import kmers as KM
    g = torch.Generator(device="cuda"); g.manual_seed(n)
    qs = torch.randint(0, 20 * n, (n,), dtype=torch.int32, device="cuda", generator=g)
    qe = qs + torch.randint(50, 5000, (n,), dtype=torch.int32, device="cuda", generator=g)
    sc = torch.randint(40, 4000, (n,), dtype=torch.int32, device="cuda", generator=g)
    cn = torch.randint(3, 60, (n,), dtype=torch.int32, device="cuda", generator=g)
    call = lambda: KM.select_chains(qs, qe, sc, cn)         # noqa: E731
    rec = summary(runs(call, reps, torch))
    sel = call()
    torch.cuda.synchronize()
    rec.update(chains=n, primaries=int((sel.flag & 1).sum()), per_kernel=per_kernel(call, torch))
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text in (a)")
    ap.add_argument("--n-repeat", type=int, default=20_000_000, help="bases of the repeated references in (b)")
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-bases", type=int, default=150)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="all")
    ap.add_argument("--out", default="profiles/select_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    if not torch.cuda.is_available():
        sys.exit("select_timing.py measures on a GPU; none is visible")
    rec = {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps"}
    rec["a_short_reads"] = index_shape(torch, kh, genome_text(a.n, 0, 7, torch), a.reads, a.read_bases, a.reps)
    print("a", {k: rec["a_short_reads"][k]["median_ms"] for k in ("select_chains", "chains", "chain_select")}, flush=True)
    for copies in (4, 16):
        base = genome_text(a.n_repeat // copies, 0, 9, torch)
        text = torch.cat([mutated(torch, base, 0.02, 100 + i) for i in range(copies)]).contiguous()
        key = "b_repeats_x%d" % copies
        n_reads = a.reads * 4 // max(4, copies)             # 16 copies: a quarter of the reads, so that the anchors stay within 2^24 per call
        rec[key] = dict(index_shape(torch, kh, text, n_reads, a.read_bases, a.reps), copies=copies, substitution_rate=0.02)
        print(key, {k: rec[key][k]["median_ms"] for k in ("select_chains", "chains", "chain_select")}, rec[key]["chains_total"], flush=True)
        del base, text
    for n in (10_000, 100_000):
        key = "c_one_group_%d" % n
        rec[key] = one_group(torch, n, max(3, a.reps // 2))
        print(key, rec[key]["median_ms"], rec[key]["primaries"], flush=True)
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out[a.tag] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
