"""Reducer inserts on one MI355X: the loaded-table case -- 10^7 records over 3*10^6 distinct keys (half of them present) into a Robin
Hood table that holds 3*10^6 keys -- for std::plus with explicit values and for min / max / or.  Call-level times (host clock, device
synchronised before and after the call), one warm-up, then the median of 10; a fresh table is loaded for every repetition.

One process measures ONE library under ONE set of KH_DISABLE_* switches (they are read when the library loads).  The parent's figure
comes from a checkout of the parent commit with its own built library: this script is run there, from that checkout's root, with
--ops plus (the parent knows insert_reduce_plus only):

  (parent checkout)  python reduce_ops_timing.py --label parent --ops plus --out parent_1.json          # five times each, alternating
  python scripts/reduce_ops_timing.py --label this --ops plus,min,max,or --out this_1.json                 # ... parent_2, this_2, ...
  KH_DISABLE_FUSED_REBUILD=1 python scripts/reduce_ops_timing.py --label this_general --ops plus,min,max,or --out general.json
  python scripts/reduce_ops_timing.py --combine parent_*.json this_*.json general.json --out profiles/reduce_ops_timing.json

--repeats R repeats the whole median-of-10 measurement R times inside one process; files that carry the same label are pooled as
repeats by --combine (the spread of the figure), which adds the ratios against the first label's plus figure and says whether plus
lies within the parent's spread.  Back-to-back blocks (all parent repeats, then all of this commit) drifted by more than the spread
of five repeats when this was first measured -- the parent measured again at the end lay above its own first spread -- hence the
alternation."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, ".")

N_TABLE, N_DISTINCT, N_RECORDS = 3_000_000, 3_000_000, 10_000_000


def measure(args):
    import torch

    import kmerhash_amd as kh

    g = torch.Generator(device="cuda"); g.manual_seed(7)
    pool = torch.unique(torch.randint(0, 1 << 62, (N_TABLE + N_DISTINCT // 2 + 4096,), dtype=torch.int64, device="cuda", generator=g))
    pool = pool[torch.randperm(pool.numel(), device="cuda", generator=g)][: N_TABLE + N_DISTINCT // 2]
    tkeys = pool[:N_TABLE].contiguous()
    tvals = torch.randint(-(1 << 31), 1 << 31, (N_TABLE,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)
    distinct = pool[N_TABLE - N_DISTINCT // 2:]                                    # half present, half new
    bkeys = distinct[torch.randint(0, N_DISTINCT, (N_RECORDS,), device="cuda", generator=g)].contiguous()
    bvals = torch.randint(-(1 << 31), 1 << 31, (N_RECORDS,), dtype=torch.int64, device="cuda", generator=g).to(torch.int32)

    def once(op, profile=False):
        t = kh.hashmap_robinhood_doubling(128, 0.35, 0.8)
        t.insert(tkeys, tvals)
        if profile:
            t.profile_enable(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if op == "plus":
            t.insert_reduce_plus(bkeys, bvals)
        else:
            t.insert_reduce(bkeys, bvals, op)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        prof = {k: [v[0], round(v[1], 3)] for k, v in t.profile().items()} if profile else None
        size, cap = t.size(), t.capacity()
        t.close()
        return ms, prof, size, cap

    res = {"label": args.label, "library": os.path.basename(kh.build.LIB), "version": kh._capi.lib().kh_version().decode(),
           "switches": sorted(k for k in os.environ if k.startswith("KH_DISABLE_")),
           "shape": {"table_keys": N_TABLE, "records": N_RECORDS, "distinct": N_DISTINCT, "present": N_DISTINCT // 2}, "ops": {}}
    for op in args.ops.split(","):
        medians, runs = [], []
        for _ in range(args.repeats):
            ms = [once(op)[0] for _ in range(11)][1:]                              # first: warm-up
            medians.append(round(statistics.median(ms), 3)); runs.append([round(x, 3) for x in ms])
        _, prof, size, cap = once(op, profile=True)
        res["ops"][op] = {"median_ms": round(statistics.median(medians), 3), "medians_ms": medians, "spread_ms": [min(medians), max(medians)],
                          "runs_ms": runs, "route": prof, "size_after": size, "capacity_after": cap}
        print(op, res["ops"][op]["median_ms"], medians, sorted(prof), flush=True)
    return res


def combine(files):
    """files with the same label are repeats of one measurement (separate processes, e.g. alternating with the other library so that
    a drift of the device over the run lands on both alike): their medians are pooled; the first label is the parent"""
    parts = []
    for f in files:
        p = json.load(open(f))
        q = next((x for x in parts if x["label"] == p["label"]), None)
        if q is None:
            parts.append(p)
            continue
        for op, r in p["ops"].items():
            o = q["ops"][op]
            o["medians_ms"] += r["medians_ms"]; o["runs_ms"] += r["runs_ms"]
            o["median_ms"] = round(statistics.median(o["medians_ms"]), 3); o["spread_ms"] = [min(o["medians_ms"]), max(o["medians_ms"])]
    ref = parts[0]["ops"]["plus"]
    lo, hi = ref["spread_ms"]
    out = {"parent_plus_ms": ref["median_ms"], "parent_plus_spread_ms": [lo, hi], "measurements": parts, "against_parent_plus": {}}
    for p in parts[1:]:
        for op, r in p["ops"].items():
            out["against_parent_plus"]["%s/%s" % (p["label"], op)] = {
                "median_ms": r["median_ms"], "ratio": round(r["median_ms"] / ref["median_ms"], 4),
                "within_parent_spread": bool(lo <= r["median_ms"] <= hi), "not_above_parent_spread": bool(r["median_ms"] <= hi), "kernels": sorted(r["route"])}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    ap.add_argument("--ops", default="plus,min,max,or")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--combine", nargs="+")
    ap.add_argument("--out", default="profiles/reduce_ops_timing.json")
    a = ap.parse_args()
    result = combine(a.combine) if a.combine else measure(a)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(result, open(a.out, "w"), indent=1)
    print(json.dumps(result if a.combine else {k: v["median_ms"] for k, v in result["ops"].items()}))
