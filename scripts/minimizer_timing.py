"""(w,k)-minimizer sampling on one MI355X: the sampling front end and the position index built over it, against the all-window front end
and index on the same text -- a random genome of --n bases with one poly-A stretch (the input of scripts/index_timing.py).  Call-level
times (host clock, device synchronised before and after the call), one warm-up, then the median of --reps (10); a fresh index for
every repetition.  One process measures one library, the one of the package in the working directory.

  --mode all     (a) minimizers_from_sequence at every --w against kmers_from_sequence(with_positions=True),
                 (b) build_sequences with w = --w[0] against build_sequences without w, both with the phases of one profiled build,
                 (c) the emitted fraction against 2 / (w + 1), (d) device memory held by the index after the build, both ways
  --mode base    only the two all-window calls: they exist in the parent commit too, so processes started in a built checkout of the
                 parent commit (this script given by its path) and processes started here can alternate into one --out file (the
                 timing condition: build_sequences without w stays inside the spread of the parent's own repeats)

  python scripts/minimizer_timing.py --out profiles/minimizer_timing.json
  (cd ../parent && python ../here/scripts/minimizer_timing.py --mode base --tag parent_1 --out ../here/profiles/minimizer_timing.json)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, ".")

K = 15


def genome_text(n, poly_a, seed, torch):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    text = lut[torch.randint(0, 4, (n,), dtype=torch.int64, device="cuda", generator=g)]
    if poly_a:
        text[n // 3: n // 3 + poly_a] = ord("A")
    return text.contiguous()


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def runs(fn, reps, torch):
    out = []
    for _ in range(reps + 1):                               # first: warm-up
        ms, r = timed(fn, torch)
        del r
        out.append(round(ms, 3))
    return out[1:]


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": min(xs), "max_ms": max(xs), "runs_ms": xs}


def build_runs(kh, text, reps, torch, **kw):
    out = []
    for _ in range(reps + 1):
        x = kh.KmerPositionIndex(k=K, **kw)
        ms, _ = timed(lambda: x.build_sequences(text), torch)
        x.close()
        out.append(round(ms, 3))
    return out[1:]


def held_after_build(kh, text, torch, **kw):
    """device memory the index holds after the build (driver-level: free memory before and after, the library's cache returned first)
    and the phases of this one profiled build"""
    L = kh._capi.lib()
    torch.cuda.synchronize(); L.kh_release_cached_memory(0)
    free0 = torch.cuda.mem_get_info()[0]
    x = kh.KmerPositionIndex(k=K, **kw)
    x.profile_enable(True)
    x.build_sequences(text)
    prof = {n: {"launches": c, "ms": round(ms, 3)} for n, (c, ms) in sorted(x.profile().items())}
    x.profile_enable(False)
    torch.cuda.synchronize(); L.kh_release_cached_memory(0)
    held = free0 - torch.cuda.mem_get_info()[0]
    res = {"positions": x.total(), "distinct": x.size(), "capacity": x.capacity(), "device_bytes_held": int(held),
           "model_bytes": x.capacity() * 16 + (x.size() + 1) * 4 + x.total() * 4, "profiled_build": prof}
    x.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text")
    ap.add_argument("--poly-a", type=int, default=1_200_000)
    ap.add_argument("--w", type=int, nargs="+", default=[10, 19])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mode", choices=["all", "base"], default="all")
    ap.add_argument("--tag", default=None, help="key of this process's record (default: the mode)")
    ap.add_argument("--out", default="profiles/minimizer_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    from kmerhash_amd import kmers as KM
    if not torch.cuda.is_available():
        sys.exit("minimizer_timing.py measures on a GPU; none is visible")
    text = genome_text(a.n, a.poly_a, 7, torch)
    rec = {"version": kh._capi.lib().kh_version().decode(), "library": os.path.basename(kh._capi.LIB), "device": torch.cuda.get_device_name(0),
           "k": K, "text_bytes": a.n, "poly_a": a.poly_a, "reps": a.reps,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps; fresh index per repetition"}
    allw = runs(lambda: KM.kmers_from_sequence(text, K, True, with_positions=True), a.reps, torch)
    n_windows = int(KM.kmers_from_sequence(text, K, True, with_positions=True)[0].numel())
    rec["all_windows"] = dict(summary(allw), pairs=n_windows)
    rec["build_sequences_all_windows"] = summary(build_runs(kh, text, a.reps, torch))
    print("all windows", rec["all_windows"]["median_ms"], "build", rec["build_sequences_all_windows"]["median_ms"], flush=True)
    if a.mode == "all":
        rec["minimizers"] = {}
        for w in a.w:
            r = summary(runs(lambda: KM.minimizers_from_sequence(text, K, w), a.reps, torch))
            m = int(KM.minimizers_from_sequence(text, K, w)[0].numel())
            # outside the poly-A stretch (which keeps every window): the density of a random text
            r.update(pairs=m, fraction=round(m / n_windows, 5), fraction_outside_poly_a=round((m - a.poly_a) / (n_windows - a.poly_a), 5),
                     two_over_w_plus_1=round(2.0 / (w + 1), 5), over_all_windows=round(r["median_ms"] / rec["all_windows"]["median_ms"], 3))
            rec["minimizers"]["w=%d" % w] = r
            print("w", w, json.dumps({k: r[k] for k in ("median_ms", "pairs", "fraction_outside_poly_a", "two_over_w_plus_1")}), flush=True)
        w0 = a.w[0]
        b = summary(build_runs(kh, text, a.reps, torch, w=w0))
        b["over_all_windows"] = round(b["median_ms"] / rec["build_sequences_all_windows"]["median_ms"], 3)
        rec["build_sequences_w=%d" % w0] = b
        rec["held_all_windows"] = held_after_build(kh, text, torch)
        rec["held_w=%d" % w0] = held_after_build(kh, text, torch, w=w0)
        print("build w", w0, b["median_ms"], "held", rec["held_all_windows"]["device_bytes_held"], rec["held_w=%d" % w0]["device_bytes_held"], flush=True)
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out[a.tag or a.mode] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
