"""kh_pair_chains on one MI355X.  Call-level times: host clock, device synchronised before and after the call, one warm-up, then the
median of --reps.  The kernel's time: device durations from torch.profiler over three further calls.

The workload is that of scripts/sam_timing.py turned into pairs: a stranded closed-syncmer index, k = 15, s = 11, of a random text of
--n bases; --frags fragments of 300..500 bases give mates of --read-bases bases, mate 1 the fragment's first bases, mate 2 the reverse
complement of its last ones, interleaved.  In one process: ix.map for comparison, pair_chains over the Mapping's columns, pair_mapping
(the same with the columns derived on the device), ix.map_pairs.

  python scripts/pair_timing.py --out profiles/pair_timing.json
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


def mates_of(torch, text, n_frags, read_bases, seed):
    """-> (reads text, read_starts, fragment lengths): read 2p = text[s:s + L], read 2p + 1 = revcomp(text[s + f - L:s + f]), an 'N' behind each"""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    frag = torch.randint(300, 501, (n_frags,), dtype=torch.int64, device="cuda", generator=g)
    starts = torch.randint(0, text.numel() - 501, (n_frags,), dtype=torch.int64, device="cuda", generator=g)
    span = torch.arange(read_bases, device="cuda")[None, :]
    m1 = text[(starts[:, None] + span).reshape(-1)].reshape(n_frags, read_bases)
    m2 = text[((starts + frag)[:, None] - 1 - span).reshape(-1)].reshape(n_frags, read_bases)      # back to front
    comp = torch.arange(256, dtype=torch.uint8, device="cuda")
    for x, y in (b"AT", b"TA", b"CG", b"GC"):
        comp[x] = y
    gap = torch.full((n_frags, 2, 1), ord("N"), dtype=torch.uint8, device="cuda")      # one byte that is no base behind every read: no seed spans two reads
    reads = torch.cat([torch.stack([m1, comp[m2.long()]], dim=1), gap], dim=2).reshape(-1).contiguous()
    return reads, torch.arange(0, 2 * n_frags * (read_bases + 1), read_bases + 1, dtype=torch.int64).numpy(), frag


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
            if "k_pair" in ev.name:
                by.setdefault(ev.name.split("(")[0].replace("void ", ""), []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        return {n: {"launches": len(v), "median_ms": round(statistics.median(v) / 1e3, 4)} for n, v in sorted(by.items())} or "no kernel events recorded"
    except Exception as e:                                  # noqa: BLE001
        return "torch.profiler not usable: %r" % (e,)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text")
    ap.add_argument("--frags", type=int, default=50_000)
    ap.add_argument("--read-bases", type=int, default=150, help="100 or 150")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default="profiles/pair_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    from kmerhash_amd import kmers as KM
    if not torch.cuda.is_available():
        sys.exit("pair_timing.py measures on a GPU; none is visible")
    rec = {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps"}
    text = genome_text(a.n, 0, 7, torch)
    x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
    x.build_sequences(text)
    reads, rs, frag = mates_of(torch, text, a.frags, a.read_bases, 11)
    n_reads = 2 * a.frags
    re_ = rs + a.read_bases
    whole = lambda: x.map(reads, text, read_starts=rs, read_ends=re_)                                       # noqa: E731
    mp = whole()
    t, sel, r = mp.table, mp.select, mp.records
    offs = torch.searchsorted(t.seg.long(), torch.arange(n_reads + 1, dtype=torch.int64, device="cuda"))
    use = (((sel.flag & 2) != 0) & (r.valid != 0)).to(torch.uint8)
    alone = lambda: KM.pair_chains(r.rs, r.re, t.rev, t.score, offs, None, use, sel.mapq)      # noqa: E731
    derived = lambda: KM.pair_mapping(mp, n_reads)                                           # noqa: E731
    both = lambda: x.map_pairs(reads, text, rs, re_)                                            # noqa: E731
    pr = alone()
    torch.cuda.synchronize()
    flag, tlen = pr.flag.cpu().numpy(), pr.tlen.cpu().numpy().astype("int64")
    mapped = (pr.row.cpu().numpy().reshape(-1, 2) >= 0).all(axis=1)
    res = {"frags": a.frags, "read_bases": a.read_bases, "text_bytes": int(text.numel()), "rows": int(t.seg.numel()), "candidates": int(use.sum()),
           "pairs_with_both_mates": int(mapped.sum()), "proper": int((flag & 1).sum()),
           "tlen_is_the_fragment": int((abs(tlen[0::2]) == frag.cpu().numpy())[(flag & 1) != 0].sum()),
           "mapq60_mates": int((pr.mapq.cpu().numpy() == 60).sum()), "single_mapq60_rows": int((sel.mapq == 60).sum()),
           "map": summary(runs(whole, a.reps, torch)), "pair_chains": summary(runs(alone, a.reps, torch)), "pair_mapping": summary(runs(derived, a.reps, torch)),
           "map_pairs": summary(runs(both, a.reps, torch)), "per_kernel": kernel_time(alone, torch)}
    rec["a"] = res
    print({k: (res[k]["median_ms"] if isinstance(res[k], dict) and "median_ms" in res[k] else res[k]) for k in res}, flush=True)
    x.close()
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out[a.tag or "mates_%d" % a.read_bases] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
