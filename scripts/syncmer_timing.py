"""Closed-syncmer sampling on one MI355X: the sampling front end for both key widths and the wide position index built over it, against
the minimizer and all-window front ends and the unsampled wide index on the same text -- a random genome of --n bases with one poly-A
stretch (the input of scripts/minimizer_timing.py, whose helpers this script uses).  Call-level times (host clock, device synchronised
before and after the call), one warm-up, then the median of --reps (10); a fresh index for every repetition.  One process measures one
library, the one of the package in the working directory.

  --mode all     (a) syncmers_from_sequence(k=15, s=11) and syncmers128_from_sequence(k=63, s=31) against minimizers_from_sequence(k=15,
                 w=10) and kmers_from_sequence / kmers128_from_sequence(with_positions=True); the count and emit kernels separately, from
                 one profiled index build each, (b) build_sequences of WideKmerPositionIndex(k=63, s=31) against the unsampled wide
                 build, with the phases of one profiled build, (c) the kept fraction outside the stretch against 2 / (k - s + 1),
                 (d) device memory held after the two wide builds
  --mode base    only build_sequences without s, 64-bit (k=15) and wide (k=63): the calls exist in the parent commit too, so processes
                 started in a built checkout of the parent commit (this script given by its path) and processes started here can
                 alternate into one --out file (the timing condition: inside the spread of the parent's own repeats)

  python scripts/syncmer_timing.py --out profiles/syncmer_timing.json
  (cd ../parent && python ../here/scripts/syncmer_timing.py --mode base --tag parent_1 --out ../here/profiles/syncmer_timing.json)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from minimizer_timing import genome_text, runs, summary, timed  # noqa: E402

K, S, W = 15, 11, 10
KW, SW = 63, 31


def build_runs(cls, text, reps, torch, **kw):
    out = []
    for _ in range(reps + 1):
        x = cls(**kw)
        ms, _ = timed(lambda: x.build_sequences(text), torch)
        x.close()
        out.append(round(ms, 3))
    return out[1:]


def held_after_build(kh, cls, text, torch, slot_bytes, **kw):
    """device memory the index holds after the build (driver-level: free memory before and after, the library's cache returned first) and
    the phases of this one profiled build"""
    L = kh._capi.lib()
    torch.cuda.synchronize(); L.kh_release_cached_memory(0)
    free0 = torch.cuda.mem_get_info()[0]
    x = cls(**kw)
    x.profile_enable(True)
    x.build_sequences(text)
    prof = {n: {"launches": c, "ms": round(ms, 3)} for n, (c, ms) in sorted(x.profile().items())}
    x.profile_enable(False)
    torch.cuda.synchronize(); L.kh_release_cached_memory(0)
    held = free0 - torch.cuda.mem_get_info()[0]
    res = {"positions": x.total(), "distinct": x.size(), "capacity": x.capacity(), "device_bytes_held": int(held),
           "model_bytes": x.capacity() * slot_bytes + (x.size() + 1) * 4 + x.total() * 4, "profiled_build": prof}
    x.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text")
    ap.add_argument("--poly-a", type=int, default=1_200_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mode", choices=["all", "base"], default="all")
    ap.add_argument("--tag", default=None, help="key of this process's record (default: the mode)")
    ap.add_argument("--out", default="profiles/syncmer_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    from kmerhash_amd import kmers as KM
    from kmerhash_amd import wide as WD
    if not torch.cuda.is_available():
        sys.exit("syncmer_timing.py measures on a GPU; none is visible")
    text = genome_text(a.n, a.poly_a, 7, torch)
    rec = {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "text_bytes": a.n, "poly_a": a.poly_a,
           "reps": a.reps,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps; fresh index per repetition"}
    if a.mode == "base":
        rec["build_sequences_k15"] = summary(build_runs(kh.KmerPositionIndex, text, a.reps, torch, k=K))
        rec["build_sequences_wide_k63"] = summary(build_runs(kh.WideKmerPositionIndex, text, a.reps, torch, k=KW))
        print("base", rec["build_sequences_k15"]["median_ms"], rec["build_sequences_wide_k63"]["median_ms"], flush=True)
    else:
        front = {}
        calls = {"kmers_from_sequence_pos_k15": lambda: KM.kmers_from_sequence(text, K, True, with_positions=True),
                 "minimizers_k15_w10": lambda: KM.minimizers_from_sequence(text, K, W),
                 "syncmers_k15_s11": lambda: KM.syncmers_from_sequence(text, K, S),
                 "kmers128_from_sequence_pos_k63": lambda: WD.kmers128_from_sequence(text, KW, True, with_positions=True),
                 "syncmers128_k63_s31": lambda: WD.syncmers128_from_sequence(text, KW, SW)}
        for name, fn in calls.items():
            r = summary(runs(fn, a.reps, torch))
            r["pairs"] = int(fn()[1].numel())
            front[name] = r
            print(name, r["median_ms"], r["pairs"], flush=True)
        # (c) outside the poly-A stretch (which keeps every window): the density of a random text
        for name, allname, k, s in (("syncmers_k15_s11", "kmers_from_sequence_pos_k15", K, S), ("syncmers128_k63_s31", "kmers128_from_sequence_pos_k63", KW, SW)):
            m, nw = front[name]["pairs"], front[allname]["pairs"]
            front[name].update(fraction_outside_poly_a=round((m - a.poly_a) / (nw - a.poly_a), 5), two_over_k_minus_s_plus_1=round(2.0 / (k - s + 1), 5),
                               over_all_windows=round(front[name]["median_ms"] / front[allname]["median_ms"], 3))
        front["syncmers_k15_s11"]["over_minimizers"] = round(front["syncmers_k15_s11"]["median_ms"] / front["minimizers_k15_w10"]["median_ms"], 3)
        rec["front_end"] = front
        # the count and emit kernels on their own, from one profiled index build each
        kern = {}
        for tag, cls, kw in (("k15_s11", kh.KmerPositionIndex, dict(k=K, s=S)), ("k15_w10", kh.KmerPositionIndex, dict(k=K, w=W))):
            prof = held_after_build(kh, cls, text, torch, 16, **kw)["profiled_build"]
            kern[tag] = {n: v for n, v in prof.items() if n.startswith(("k_syncmers", "k_minimizers"))}
        # (b), (d) the wide index, sampled and not
        rec["build_wide_all_windows"] = summary(build_runs(kh.WideKmerPositionIndex, text, a.reps, torch, k=KW))
        b = summary(build_runs(kh.WideKmerPositionIndex, text, a.reps, torch, k=KW, s=SW))
        b["over_all_windows"] = round(b["median_ms"] / rec["build_wide_all_windows"]["median_ms"], 3)
        rec["build_wide_s31"] = b
        rec["held_wide_all_windows"] = held_after_build(kh, kh.WideKmerPositionIndex, text, torch, 32, k=KW)
        rec["held_wide_s31"] = held_after_build(kh, kh.WideKmerPositionIndex, text, torch, 32, k=KW, s=SW)
        kern["k63_s31"] = {n: v for n, v in rec["held_wide_s31"]["profiled_build"].items() if n.startswith("k_syncmers")}
        rec["sampling_kernels"] = kern
        print("wide build", rec["build_wide_all_windows"]["median_ms"], b["median_ms"], "held", rec["held_wide_all_windows"]["device_bytes_held"],
              rec["held_wide_s31"]["device_bytes_held"], json.dumps(kern), flush=True)
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out[a.tag or a.mode] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
