"""Mate rescue on one MI355X.  Call-level times: host clock, device synchronised before and after the call, one warm-up, then the
median of --reps.  The kernels' times: device durations from torch.profiler over three further calls.

The workload is that of scripts/pair_timing.py with the seeds of 10 % of the mates destroyed: a stranded closed-syncmer index, k = 15,
s = 11, of a random text of --n bases; --frags fragments of 300..500 bases give mates of --read-bases bases, interleaved; in every
fifth fragment mate 2 carries a substitution every 12 bases, none within 5 bases of either end, so that it has no seed and no chain row.
In one process: ix.map_pairs (the yardstick: what the parent commit offers on this workload), rescue_requests over its result,
rescue_mates over those requests, ix.map_pairs_rescued.

  python scripts/rescue_timing.py --out profiles/rescue_timing.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from edits_timing import K, S  # noqa: E402
from minimizer_timing import genome_text, runs, summary  # noqa: E402
from pair_timing import mates_of  # noqa: E402


def destroy_seeds(torch, reads, read_bases, n_frags, every):
    """a substitution at the bases 5, 17, 29, ... of mate 2 of every `every`-th fragment -> the numbers of the damaged reads"""
    frags = torch.arange(0, n_frags, every, device="cuda")
    at = torch.arange(5, read_bases - 5, 12, device="cuda")
    pos = ((2 * frags + 1) * (read_bases + 1))[:, None] + at[None, :]
    nxt = torch.zeros(256, dtype=torch.uint8, device="cuda")
    for x, y in (b"AC", b"CG", b"GT", b"TA"):
        nxt[x] = y
    reads[pos.reshape(-1)] = nxt[reads[pos.reshape(-1)].long()]
    return (2 * frags + 1).cpu().numpy()


def kernel_time(fn, torch, calls=3):
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
            if "k_rescue" in ev.name:
                by.setdefault(ev.name.split("(")[0].replace("void ", ""), []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        return {n: {"launches": len(v), "median_ms": round(statistics.median(v) / 1e3, 4)} for n, v in sorted(by.items())} or "no kernel events recorded"
    except Exception as e:                                  # noqa: BLE001
        return "torch.profiler not usable: %r" % (e,)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text")
    ap.add_argument("--frags", type=int, default=50_000)
    ap.add_argument("--read-bases", type=int, default=150, help="100 or 150")
    ap.add_argument("--every", type=int, default=5, help="mate 2 of every n-th fragment loses its seeds: 5 = 10 %% of the mates")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default="profiles/rescue_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    from kmerhash_amd import kmers as KM
    if not torch.cuda.is_available():
        sys.exit("rescue_timing.py measures on a GPU; none is visible")
    rec = {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps"}
    text = genome_text(a.n, 0, 7, torch)
    x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
    x.build_sequences(text)
    reads, rs, frag = mates_of(torch, text, a.frags, a.read_bases, 11)
    damaged = destroy_seeds(torch, reads, a.read_bases, a.frags, a.every)
    re_ = rs + a.read_bases
    pairs_only = lambda: x.map_pairs(reads, text, rs, re_)                                       # noqa: E731
    mp, pr = pairs_only()
    requests = lambda: KM.rescue_requests(mp, pr, rs, re_, ref_len=int(text.numel()))          # noqa: E731
    rq = requests()
    alone = lambda: KM.rescue_mates(reads, text, rq.q_lo, rq.q_hi, rq.w_lo, rq.w_hi, rq.rev)   # noqa: E731
    whole = lambda: x.map_pairs_rescued(reads, text, rs, re_)                                    # noqa: E731
    res = alone()
    torch.cuda.synchronize()
    edits, read = res.edits.cpu().numpy(), rq.read.cpu().numpy()
    placed = edits >= 0
    want = len(range(5, a.read_bases - 5, 12))
    out = {"frags": a.frags, "read_bases": a.read_bases, "text_bytes": int(text.numel()), "damaged_mates": int(len(damaged)), "requests": int(len(read)),
           "requests_are_the_damaged_mates": bool(set(read.tolist()) >= set(damaged.tolist())), "rescued": int(placed.sum()),
           "rescued_with_the_planted_edits": int((edits == want).sum()), "over": int((edits == -2).sum()), "none": int((edits == -1).sum()),
           "window_bases_median": int(statistics.median((rq.w_hi - rq.w_lo).cpu().numpy().tolist())) if len(read) else 0,
           "map_pairs": summary(runs(pairs_only, a.reps, torch)), "rescue_requests": summary(runs(requests, a.reps, torch)),
           "rescue_mates": summary(runs(alone, a.reps, torch)), "map_pairs_rescued": summary(runs(whole, a.reps, torch)), "per_kernel": kernel_time(alone, torch)}
    out["added_share_of_map_pairs"] = round(out["map_pairs_rescued"]["median_ms"] / out["map_pairs"]["median_ms"] - 1.0, 4)
    rec["a"] = out
    print({k: (out[k]["median_ms"] if isinstance(out[k], dict) and "median_ms" in out[k] else out[k]) for k in out}, flush=True)
    x.close()
    js = json.load(open(a.out)) if os.path.exists(a.out) else {}
    js[a.tag or "mates_%d" % a.read_bases] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(js, open(a.out, "w"), indent=1)
    print("wrote", a.out)
