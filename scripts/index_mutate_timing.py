"""Changing a built k-mer position index on one MI355X: append, erase and erase by occurrence count against the build, on the canonical
k-mers of a random genome with ONE poly-A stretch (a segment of 1.2 * 10^6 positions).  Call-level times (host clock, device synchronised
before and after the call), one warm-up, then the median of --reps (10), all in one process; every repetition starts from a fresh index
(the builds that only set a repetition up are not timed).  k = 31 on KmerPositionIndex, k = 63 on WideKmerPositionIndex.

Measured per k (N = --n pairs, B = --batch pairs; defaults 10^8 and 10^7):
  (a) build of N + B pairs                                  -- the unchanged path, the yardstick
  (a100) build of the first N pairs                         -- what (c) is compared with
  (b) build of the first N pairs, then append of the last B -- the append is timed
  (c) append of the first N pairs onto an empty index       -- the build's own path
  (d) erase_counts(10^6, 2^32 - 1) on the index of all N + B pairs: removes the poly-A segment
  (e) erase of 10^7 keys sampled from the input
and, from one extra profiled call each, the per-kernel split of (a), (b), (d) and (e).

  python scripts/index_mutate_timing.py --out profiles/index_mutate_timing.json

--only build --label X [--out X.json]: (a) alone, with nothing but build() called -- it runs on the parent commit's checkout too.  Parent
and this commit are measured in alternating processes (the discipline of scripts/reduce_ops_timing.py) and put side by side with
--combine parent_*.json this_*.json --into profiles/index_mutate_timing.json."""
import argparse
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, ".")


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


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3), "runs_ms": [round(v, 3) for v in xs]}


def pairs(k, n_pairs, poly_a, torch, KM, W):
    text = genome_text(n_pairs + k - 1, poly_a, 7, torch)
    if k <= 32:
        keys, pos = KM.kmers_from_sequence(text, k, True, with_positions=True)
    else:
        keys, pos = W.kmers128_from_sequence(text, k, True, with_positions=True)
    assert pos.numel() == n_pairs
    return keys.contiguous(), pos.contiguous()


def measure_build_only(k, n_pairs, poly_a, reps, torch, kh, KM, W):
    keys, pos = pairs(k, n_pairs, poly_a, torch, KM, W)
    cls = kh.KmerPositionIndex if k <= 32 else kh.WideKmerPositionIndex
    ms = []
    for _ in range(reps + 1):
        x = cls(k=k)
        ms.append(timed(lambda: x.build(keys, pos), torch)[0])
        x.close()
    return stats(ms[1:])


def measure(k, n, batch, poly_a, n_erase, reps, torch, kh, KM, W):
    keys, pos = pairs(k, n + batch, poly_a, torch, KM, W)
    cls = kh.KmerPositionIndex if k <= 32 else kh.WideKmerPositionIndex
    k0, p0, k1, p1 = keys[:n], pos[:n], keys[n:], pos[n:]
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    gone = keys[torch.randint(0, n + batch, (n_erase,), device="cuda", generator=g)].contiguous()

    def fresh(profile=False):
        x = cls(k=k)
        if profile:
            x.profile_enable(True)
        return x

    def run(what, profile=False):
        """-> (ms of the timed call, its result, the index)"""
        x = fresh()
        if what == "a":
            call = lambda: x.build(keys, pos)                 # noqa: E731
        elif what == "a100":
            call = lambda: x.build(k0, p0)                    # noqa: E731
        elif what == "c":
            call = lambda: x.append(k0, p0)                   # noqa: E731
        elif what == "b":
            x.build(k0, p0)
            call = lambda: x.append(k1, p1)                   # noqa: E731
        elif what == "d":
            x.build(keys, pos)
            call = lambda: x.erase_counts(1_000_000, 2 ** 32 - 1)      # noqa: E731
        else:
            x.build(keys, pos)
            call = lambda: x.erase(gone)                      # noqa: E731
        if profile:
            x.profile_enable(True)
        ms, r = timed(call, torch)
        return ms, r, x

    order = ["a", "a100", "c", "b", "d", "e"]
    ms = {w: [] for w in order}
    results = {}
    for r in range(reps + 1):                                 # interleaved: a drift of the device lands on all alike; first round: warm-up
        for w in order:
            t, res, x = run(w)
            results[w] = (res, x.size(), x.total(), x.capacity())
            x.close()
            ms[w].append(t)
    out = {"k": k, "pairs_N": n, "pairs_B": batch, "poly_a": poly_a, "erase_keys": n_erase}
    names = {"a": "a_build_N_plus_B", "a100": "a100_build_N", "b": "b_append_B_onto_N", "c": "c_append_N_onto_empty", "d": "d_erase_counts_poly_a", "e": "e_erase_keys"}
    for w in order:
        out[names[w]] = stats(ms[w][1:])
        out[names[w]]["after"] = {"size": results[w][1], "total": results[w][2], "capacity": results[w][3]}
    out[names["d"]]["erased_keys_positions"] = list(results["d"][0])
    out[names["e"]]["erased_keys_positions"] = list(results["e"][0])
    assert results["b"][1:] == results["a"][1:], "build + append and the one-shot build disagree on size / total / capacity"
    out["profiles"] = {}
    for w in ("a", "b", "d", "e"):
        _, _, x = run(w, profile=True)
        out["profiles"][names[w]] = {kn: {"launches": v[0], "ms": round(v[1], 3)} for kn, v in sorted(x.profile().items())}
        x.close()
    md = lambda w: out[names[w]]["median_ms"]                 # noqa: E731
    out["b_over_a"] = round(md("b") / md("a"), 3)
    out["c_over_a100"] = round(md("c") / md("a100"), 3)
    out["d_over_a"] = round(md("d") / md("a"), 3)
    out["e_over_a"] = round(md("e") / md("a"), 3)
    print("k=%d" % k, json.dumps({names[w]: md(w) for w in order}), flush=True)
    for w in ("b", "d", "e"):
        print("k=%d" % k, names[w], json.dumps(out["profiles"][names[w]]), flush=True)
    return out


def combine(files, into):
    parts = [json.load(open(f)) for f in files]
    labels = sorted({p["label"] for p in parts})
    res = {"method": "build of N + B pairs (a), alternating processes, one library per process; per process one warm-up and the median of reps",
           "processes": [{"label": p["label"], **p["a_build_N_plus_B"]} for p in parts]}
    for lb in labels:
        meds = [p["a_build_N_plus_B"]["median_ms"] for p in parts if p["label"] == lb]
        res[lb] = {"median_of_process_medians_ms": round(statistics.median(meds), 3), "spread_ms": [min(meds), max(meds)]}
    if "parent" in res and "this" in res:
        lo, hi = res["parent"]["spread_ms"]
        m = res["this"]["median_of_process_medians_ms"]
        res["this_within_parent_spread"] = bool(lo <= m <= hi)
        res["this_not_above_parent_spread"] = bool(m <= hi)
    doc = json.load(open(into)) if os.path.exists(into) else {}
    doc["build_against_parent"] = res
    json.dump(doc, open(into, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "processes"}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="pairs of the first batch")
    ap.add_argument("--batch", type=int, default=10_000_000, help="pairs appended")
    ap.add_argument("--poly-a", type=int, default=1_200_000)
    ap.add_argument("--erase", type=int, default=10_000_000, help="keys of the erase batch (sampled occurrences)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ks", default="31,63")
    ap.add_argument("--only", default="", help="build: (a) alone, through build() only")
    ap.add_argument("--label", default="this")
    ap.add_argument("--combine", nargs="*", help="per-process files of --only build (globs allowed)")
    ap.add_argument("--into", default="profiles/index_mutate_timing.json")
    ap.add_argument("--out", default="profiles/index_mutate_timing.json")
    a = ap.parse_args()
    if a.combine:
        combine(sorted(f for pat in a.combine for f in glob.glob(pat)), a.into)
        sys.exit(0)
    import torch

    import kmerhash_amd as kh
    from kmerhash_amd import kmers as KM
    from kmerhash_amd import wide as W
    if not torch.cuda.is_available():
        sys.exit("index_mutate_timing.py measures on a GPU; none is visible")
    head = {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "reps": a.reps,
            "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps; fresh index per repetition"}
    if a.only == "build":
        out = dict(head, label=a.label, k=31, a_build_N_plus_B=measure_build_only(31, a.n + a.batch, a.poly_a, a.reps, torch, kh, KM, W))
        print(a.label, json.dumps(out["a_build_N_plus_B"]), flush=True)
    else:
        out = dict(head, workloads={})
        for k in [int(v) for v in a.ks.split(",")]:
            out["workloads"]["k%d" % k] = measure(k, a.n, a.batch, a.poly_a, a.erase, a.reps, torch, kh, KM, W)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
