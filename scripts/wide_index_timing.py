"""Position index over 16-byte k-mers on one MI355X: build and lookup of a random genome's canonical 63-mers (10^8 of them: a 4 GB
table).  Call-level times (host clock, device synchronised before and after the call), one warm-up, then the median of --reps (10); a
fresh index / table is made for every repetition, index and floor alternate.  One process measures one library (the discipline of
scripts/index_timing.py, whose shape this script has).

Recorded:
  * build (kh_wide_index_build of device pairs) and its split by phase from one extra, profiled build (HIP events per kernel): the wide
    counting insert's kernels, kw_index_rank (run order + ranks + counts), k_index_scan, kw_index_scatter, k_index_tile_sort,
    k_index_seg_radix;
  * count and find of 10^7 keys sampled from the input;
  * the floors, in the same process: insert_reduce_plus of the same keys into a plain wide table (the index runs this very code as its
    first phase), the plain wide table's per-query find (kw_find) of the same 10^7 keys, and the 64-bit index (k = 31) over the same text:
    its build, its phases, count and find;
  * for every phase the bytes it has to move against the time it took (model_ms at the 8 TB/s of the HBM, and time / model).

  python scripts/wide_index_timing.py --out profiles/wide_index_timing.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, ".")

K_WIDE, K_NARROW = 63, 31
HBM_BYTES_PER_MS = 8.0e9      # 8 TB/s


def genome_text(n, seed, torch):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    return lut[torch.randint(0, 4, (n,), dtype=torch.int64, device="cuda", generator=g)].contiguous()


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def med(xs):
    return round(statistics.median(xs), 3)


def phase_table(prof, model):
    """{kernel: launches, ms, model bytes, model ms at 8 TB/s, time over model} for the index's own phases"""
    phases = {}
    for k, (launches, ms) in sorted(prof.items()):
        if "_index_" not in k:
            continue
        b = model.get(k)
        phases[k] = {"launches": launches, "ms": round(ms, 3), "model_bytes": b,
                     "model_ms_at_8TBs": round(b / HBM_BYTES_PER_MS, 3) if b else None, "time_over_model": round(ms / (b / HBM_BYTES_PER_MS), 2) if b else None}
    return phases


def measure_index(make_index, make_table, table_find, keys, pos, q, reps, slot_bytes, key_bytes, probe_bytes, prefix, torch):
    """build / count / find of one index against its counting-insert and plain-find floors"""
    n = pos.numel()

    def build_once(profile=False):
        x = make_index()
        if profile:
            x.profile_enable(True)
        ms, _ = timed(lambda: x.build(keys, pos), torch)
        return ms, x

    def floor_once():
        t = make_table()
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
    assert total == n
    n_pos = int(x.find(q, positions=False)[0][-1])
    c_ms, fi_ms, pf_ms = [], [], []
    for r in range(reps + 1):
        c_ms.append(timed(lambda: x.count(q), torch)[0])
        ms, (offs, p) = timed(lambda: x.find(q, cap_out=n_pos), torch)      # (one find call: the room is known)
        assert int(p.numel()) == n_pos
        fi_ms.append(ms)
        pf_ms.append(timed(lambda: table_find(t, q), torch)[0])
    c_ms, fi_ms, pf_ms = c_ms[1:], fi_ms[1:], pf_ms[1:]
    x.close(); t.close()
    insert_ms = round(sum(v[1] for k, v in prof.items() if "_index_" not in k), 3)
    # bytes every phase has to move (n pairs, `size` distinct keys, `cap` slots)
    model = {
        prefix + "_index_rank": cap * slot_bytes * 3 + size * 8,            # run order, tile count and rank pass read the slots; counts out, ranks in
        "k_index_scan": size * 4 * 3,                                       # counts read twice, offsets written
        prefix + "_index_scatter": n * (key_bytes + 4 + probe_bytes + 4 + 4),      # key + position in, the probe, cursor atomic, 4 B random write
        "k_index_tile_sort": n * 8,                                         # positions streamed in and out
        "k_index_seg_radix": None,                                          # depends on the crossing segments
    }
    res = {"occurrences": n, "distinct": size, "capacity": cap, "table_bytes": cap * slot_bytes, "queries": int(q.shape[0]), "positions_found": n_pos,
           "build_ms": med(b_ms), "build_runs_ms": [round(v, 3) for v in b_ms],
           "counting_insert_floor_ms": med(f_ms), "floor_runs_ms": [round(v, 3) for v in f_ms],
           "build_over_counting_insert": round(med(b_ms) / med(f_ms), 3),
           "profiled_build": {"counting_insert_kernels_ms": insert_ms, "phases": phase_table(prof, model)},
           "count_ms": med(c_ms), "find_ms": med(fi_ms), "plain_find_floor_ms": med(pf_ms), "find_over_plain_find": round(med(fi_ms) / med(pf_ms), 3),
           "count_runs_ms": [round(v, 3) for v in c_ms], "find_runs_ms": [round(v, 3) for v in fi_ms], "plain_find_runs_ms": [round(v, 3) for v in pf_ms]}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text (= occurrences + k - 1)")
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="profiles/wide_index_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    from kmerhash_amd import kmers as KM
    from kmerhash_amd import wide as W
    if not torch.cuda.is_available():
        sys.exit("wide_index_timing.py measures on a GPU; none is visible")
    out = {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "k_wide": K_WIDE, "k_narrow": K_NARROW, "reps": a.reps,
           "text_bytes": a.n,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps; fresh index per repetition, "
                     "index and floor alternating; phases from one extra profiled build (HIP events per kernel)",
           "model": "bytes per phase over 8 TB/s; the scatter's probe is counted as 96 B per pair for 16-byte keys (two 32-byte slots: one 64-byte "
                    "sector on an even home, two on an odd one) and 64 B for 8-byte keys"}
    text = genome_text(a.n, 7, torch)
    g = torch.Generator(device="cuda"); g.manual_seed(11)

    keys, pos = W.kmers128_from_sequence(text, K_WIDE, True, with_positions=True)
    keys, pos = keys.contiguous(), pos.contiguous()
    q = keys[torch.randint(0, pos.numel(), (a.queries,), device="cuda", generator=g)].contiguous()
    out["wide_k63"] = measure_index(lambda: kh.WideKmerPositionIndex(k=K_WIDE), lambda: kh.hashmap_robinhood_doubling_wide(128, 0.35, 0.8, hash="farm", seed=43),
                                    lambda t, qq: t.find_values(qq), keys, pos, q, a.reps, 32, 16, 96, "kw", torch)
    print("wide_k63", json.dumps({k: v for k, v in out["wide_k63"].items() if not k.endswith("_runs_ms")}), flush=True)
    del keys, pos, q
    torch.cuda.empty_cache()

    keys, pos = KM.kmers_from_sequence(text, K_NARROW, True, with_positions=True)
    keys, pos = keys.contiguous(), pos.contiguous()
    q = keys[torch.randint(0, pos.numel(), (a.queries,), device="cuda", generator=g)].contiguous()
    out["narrow_k31"] = measure_index(lambda: kh.KmerPositionIndex(k=K_NARROW), lambda: kh.hashmap_robinhood_doubling(128, 0.35, 0.8, hash="farm", seed=43),
                                      lambda t, qq: t.find(qq), keys, pos, q, a.reps, 16, 8, 64, "k", torch)
    print("narrow_k31", json.dumps({k: v for k, v in out["narrow_k31"].items() if not k.endswith("_runs_ms")}), flush=True)

    w, nrw = out["wide_k63"], out["narrow_k31"]
    out["wide_over_narrow"] = {k: round(w[k] / nrw[k], 3) for k in ("build_ms", "counting_insert_floor_ms", "count_ms", "find_ms", "plain_find_floor_ms")}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
