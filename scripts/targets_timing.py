"""kh_anchor_targets and the multi-target mapper on one MI355X.  Call-level times: host clock, device synchronised before and after the
call, one warm-up, then the median of --reps.  Per-kernel times: device durations from torch.profiler over three further calls.

The workload of scripts/records_timing.py (a) -- a stranded closed-syncmer index, k = 15, s = 11, of --n random bases; --reads reads
of 150 bases -- with the same bases cut into 1, 24 and 10 000 contigs of equal length, laid out by kh.Targets with the default spacer:
24 targets are searched in LDS, 10 000 through L2 (more than KH_TARGETS_STAGED_MAX).  Per layout: kmers.group_anchors alone over the
anchors of all reads, both of its kernels, and ix.map(targets=T) beside ix.map() of the same build over the same text.

  python scripts/targets_timing.py --out profiles/targets_timing.json
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
            if "k_target" in ev.name:
                by.setdefault(ev.name.split("(")[0].replace("void ", ""), []).append(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
        return {n: {"launches": len(v), "median_ms": round(statistics.median(v) / 1e3, 4)} for n, v in sorted(by.items())} or "no kernel events recorded"
    except Exception as e:                                  # noqa: BLE001
        return "torch.profiler not usable: %r" % (e,)


def lay_out(torch, kh, bases, n_contigs):
    """the bases cut into n_contigs contigs of equal length (the last takes the rest) -> (Targets, the laid-out text on the device)"""
    n = int(bases.numel())
    ln = n // n_contigs
    lengths = [ln] * (n_contigs - 1) + [n - ln * (n_contigs - 1)]
    T = kh.Targets(["ctg%d" % i for i in range(n_contigs)], lengths)
    text = torch.full((int(T.ends[-1]),), ord("N"), dtype=torch.uint8, device="cuda")
    at = torch.arange(n, dtype=torch.int64, device="cuda")
    text[at + torch.clamp(at // ln, max=n_contigs - 1) * T.spacer] = bases
    return T, text


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text")
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-bases", type=int, default=150)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--contigs", type=int, nargs="+", default=[1, 24, 10_000])
    ap.add_argument("--tag", default="all")
    ap.add_argument("--out", default="profiles/targets_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    from kmerhash_amd import kmers as KM
    if not torch.cuda.is_available():
        sys.exit("targets_timing.py measures on a GPU; none is visible")
    rec = {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps"}
    bases = genome_text(a.n, 0, 7, torch)
    for nc in a.contigs:
        T, text = lay_out(torch, kh, bases, nc)
        x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
        x.build_sequences(text)
        reads, rs = reads_of(torch, text, a.reads, a.read_bases, 11)
        q, r, v = x.anchors(reads)
        seg = kh.mapper.read_segments(kh.mapper.namespace_of(q), q, kh.mapper.ReadLayout(rs, None, None))
        group = lambda: KM.group_anchors(q, r, v, T, K, seg)                            # noqa: E731
        plain = lambda: x.map(reads, text, read_starts=rs)                              # noqa: E731
        multi = lambda: x.map(reads, text, read_starts=rs, targets=T)                   # noqa: E731
        g, mp, mt = group(), plain(), multi()
        torch.cuda.synchronize()
        tid = g.tid.long() & 0xFFFFFFFF
        e = {"contigs": nc, "staged_in_lds": nc <= 8192, "text_bytes": int(text.numel()), "reads": a.reads, "anchors": int(q.numel()), "groups": int(g.seg.numel()),
             "anchors_without_target": int((tid == kh.TARGET_NONE).sum()), "rows_plain": int(mp.table.seg.numel()), "rows_targets": int(mt.table.seg.numel()),
             "valid_plain": int(mp.records.valid.sum()), "valid_targets": int(mt.records.valid.sum()),
             "group_anchors": summary(runs(group, a.reps, torch)), "map": summary(runs(plain, a.reps, torch)), "map_targets": summary(runs(multi, a.reps, torch)),
             "per_kernel": per_kernel(group, torch)}
        e["map_targets_over_map"] = round(e["map_targets"]["median_ms"] / e["map"]["median_ms"], 4)
        rec["contigs_%d" % nc] = e
        print(nc, {k: e[k]["median_ms"] for k in ("group_anchors", "map", "map_targets")}, e["map_targets_over_map"], e["per_kernel"], flush=True)
        x.close()
        del text, reads, q, r, v, g, mp, mt
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out[a.tag] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
