"""K-mer position index on one MI355X: build and lookup of a synthetic genome's canonical 31-mers, once at low repeat content and once
with a poly-A stretch that makes ONE segment longer than 10^6 positions.  Call-level times (host clock, device synchronised before and
after the call), one warm-up, then the median of --reps (10); a fresh index / table is made for every repetition.  One process
measures one library (the discipline of scripts/reduce_ops_timing.py).

Recorded per workload:
  * build (kh_index_build of device pairs) and its split by phase from one extra, profiled build (HIP events per kernel): the counting
    insert's kernels, k_index_rank (run order + ranks + counts), k_index_scan, k_index_scatter, k_index_tile_sort, k_index_seg_radix;
  * count and find of 10^7 keys sampled from the input;
  * the floors, in the same process and on the same keys: insert_reduce_plus into a plain Robin Hood table (the index runs this very
    code as its first phase; it is the parent commit's code, unchanged) and the plain table's find of the same 10^7 keys;
  * the ratios build / counting insert and find / plain find;
  * for every new phase the bytes it has to move against the time it took (model_ms at the 8 TB/s of the HBM, and time / model).

  python scripts/index_timing.py --out profiles/index_timing.json            # both workloads, 10^8 occurrences each
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, ".")

K = 31
HBM_BYTES_PER_MS = 8.0e9      # 8 TB/s


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


def med(xs):
    return round(statistics.median(xs), 3)


def measure_workload(name, n_text, poly_a, n_query, reps, torch, kh, KM):
    text = genome_text(n_text, poly_a, 7, torch)
    keys, pos = KM.kmers_from_sequence(text, K, True, with_positions=True)
    keys, pos = keys.contiguous(), pos.contiguous()
    n = keys.numel()
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    # queries: sampled occurrences from outside the poly-A stretch, plus the poly-A k-mer ONCE (one query with >= 10^6 hits; sampling it by
    # occurrence would ask for it 10^5 times over)
    if poly_a:
        lo, hi = n_text // 3 - K, n_text // 3 + poly_a
        idx = torch.randint(0, n - (hi - lo), (n_query,), device="cuda", generator=g)
        idx = torch.where(idx >= lo, idx + (hi - lo), idx)
        q = keys[idx].contiguous()
        q[0] = keys[n_text // 3 + K]
    else:
        q = keys[torch.randint(0, n, (n_query,), device="cuda", generator=g)].contiguous()

    def build_once(profile=False):
        x = kh.KmerPositionIndex(k=K)
        if profile:
            x.profile_enable(True)
        ms, _ = timed(lambda: x.build(keys, pos), torch)
        return ms, x

    def floor_once():
        t = kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash="farm", seed=43)
        ms, _ = timed(lambda: t.insert_reduce_plus(keys), torch)
        return ms, t

    b_ms, f_ms = [], []
    for r in range(reps + 1):                               # alternating: a drift of the device lands on both alike; first: warm-up
        ms, x = build_once(); x.close(); b_ms.append(ms)
        ms, t = floor_once(); t.close(); f_ms.append(ms)
    b_ms, f_ms = b_ms[1:], f_ms[1:]
    _, x = build_once(profile=True)
    prof = x.profile()
    x.profile_enable(False)
    _, t = floor_once()
    size, total, cap = x.size(), x.total(), x.capacity()
    longest = int(x.count(q[:1_000_000]).max())
    n_pos = int(x.find(q, positions=False)[0][-1])
    c_ms, fi_ms, pf_ms = [], [], []
    for r in range(reps + 1):
        c_ms.append(timed(lambda: x.count(q), torch)[0])
        ms, (offs, p) = timed(lambda: x.find(q, cap_out=n_pos), torch)      # (one kh_index_find call: the room is known)
        assert int(p.numel()) == n_pos
        fi_ms.append(ms)
        pf_ms.append(timed(lambda: t.find(q), torch)[0])
    c_ms, fi_ms, pf_ms = c_ms[1:], fi_ms[1:], pf_ms[1:]
    x.close(); t.close()
    new = {k: v for k, v in prof.items() if k.startswith("k_index_")}
    insert_ms = round(sum(v[1] for k, v in prof.items() if not k.startswith("k_index_")), 3)
    # bytes every new phase has to move (n pairs, `size` distinct keys, `cap` slots of 16 B)
    model = {
        "k_index_rank": cap * 16 * 3 + size * 8,            # run order, tile count and rank pass read the slots; counts out, ranks in
        "k_index_scan": size * 4 * 3,                       # counts read twice, offsets written
        "k_index_scatter": n * (8 + 4 + 64 + 4 + 4),        # key + position in, one 64 B sector probed, cursor atomic, 4 B random write
        "k_index_tile_sort": n * 8,                         # positions streamed in and out
        "k_index_seg_radix": None,                          # depends on the crossing segments: 4 passes x 12 B over their entries
    }
    phases = {}
    for k, (launches, ms) in sorted(new.items()):
        b = model.get(k)
        phases[k] = {"launches": launches, "ms": round(ms, 3), "model_bytes": b,
                     "model_ms_at_8TBs": round(b / HBM_BYTES_PER_MS, 3) if b else None, "time_over_model": round(ms / (b / HBM_BYTES_PER_MS), 2) if b else None}
    res = {"text_bytes": n_text, "poly_a": poly_a, "occurrences": n, "distinct": size, "capacity": cap, "queries": n_query, "positions_found": n_pos,
           "largest_count_among_first_1e6_queries": longest,
           "build_ms": med(b_ms), "build_runs_ms": [round(v, 3) for v in b_ms],
           "counting_insert_floor_ms": med(f_ms), "floor_runs_ms": [round(v, 3) for v in f_ms],
           "build_over_counting_insert": round(med(b_ms) / med(f_ms), 3),
           "profiled_build": {"counting_insert_kernels_ms": insert_ms, "phases": phases},
           "count_ms": med(c_ms), "find_ms": med(fi_ms), "plain_find_floor_ms": med(pf_ms), "find_over_plain_find": round(med(fi_ms) / med(pf_ms), 3),
           "find_runs_ms": [round(v, 3) for v in fi_ms], "plain_find_runs_ms": [round(v, 3) for v in pf_ms]}
    print(name, json.dumps({k: res[k] for k in ("occurrences", "distinct", "build_ms", "counting_insert_floor_ms", "count_ms", "find_ms", "plain_find_floor_ms")}), flush=True)
    print(name, "phases", json.dumps(phases), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text (= occurrences + k - 1)")
    ap.add_argument("--poly-a", type=int, default=1_200_000)
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="profiles/index_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    from kmerhash_amd import kmers as KM
    if not torch.cuda.is_available():
        sys.exit("index_timing.py measures on a GPU; none is visible")
    out = {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "k": K, "reps": a.reps,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps; fresh index per repetition",
           "workloads": {}}
    out["workloads"]["low_repeat"] = measure_workload("low_repeat", a.n, 0, a.queries, a.reps, torch, kh, KM)
    out["workloads"]["poly_a"] = measure_workload("poly_a", a.n, a.poly_a, a.queries, a.reps, torch, kh, KM)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
