"""Value-range operations at the bench table's size on one MI355X: 107 374 184 keys at capacity 2^27, the 64-bit Robin Hood table and
the 16-byte-key table at the same fill.  Call-level times (host clock around calls that end in a stream synchronise), after one
warm-up repetition, medians over the rest:
  hist_uniform / hist_equal : value_histogram(256), values uniform in 0..255 / all equal
  select_1pct / select_all  : select_values(..., device=True) for ranges matching ~1 % and 100 %
  erase_values_10pct        : erase_values of ~10 %, next to erase() of the same keys (device tensor) on a twin table
  baseline_*                : the route without these operations: to_vector() + numpy (+ erase(keys) for the filter)
For the 64-bit table the per-kernel HIP-event times of the new kernels are reported too (kh_profile_*).  Writes
profiles/values_timing.json (or the path given) and prints it.  Run under `rocprofv3 --kernel-trace --stats -- python
scripts/values_timing.py --quick` in a run of its own for the kernel breakdown."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd.wide import hashmap_robinhood_doubling_wide  # noqa: E402

N, CAP, U32 = 107_374_184, 1 << 27, 0xFFFFFFFF


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def med(f, reps):
    out = [timed(f)[0] for _ in range(reps + 1)][1:]          # first repetition: warm-up
    return round(statistics.median(out), 3), [round(x, 3) for x in out]


def run(wide, reps, base_reps):
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    keys = torch.randint(0, 1 << 62, (N, 2) if wide else (N,), dtype=torch.int64, device="cuda", generator=g)
    if not wide:
        keys = torch.unique(keys)
        assert keys.numel() >= N - 64                         # (random 62-bit keys: a handful of repeats at most)
    n = keys.shape[0]
    uni = torch.randint(0, 256, (n,), dtype=torch.int32, device="cuda", generator=g)
    cls = hashmap_robinhood_doubling_wide if wide else kh.hashmap_robinhood_doubling

    def table(vals):
        t = cls(CAP, 0.35, 0.8)
        assert t.insert(keys, vals) == n and t.capacity() == CAP
        return t

    res = {"keys": int(n), "capacity": CAP, "slot_bytes": 32 if wide else 16}
    t = table(uni)
    if not wide:
        t.profile_enable(True)
    res["hist_uniform_ms"], res["hist_uniform_all"] = med(lambda: t.value_histogram(256), reps)
    h = t.value_histogram(256)
    assert int(h.sum()) == n and np.array_equal(h, torch.bincount(uni, minlength=256).cpu().numpy().astype(np.uint64))
    res["select_1pct_ms"], res["select_1pct_all"] = med(lambda: t.select_values(0, 2, device=True), reps)
    res["select_1pct_matches"] = t.count_values(0, 2)
    res["count_1pct_ms"], _ = med(lambda: t.count_values(0, 2), reps)
    res["select_all_ms"], res["select_all_all"] = med(lambda: t.select_values(0, U32, device=True), reps)
    if not wide:
        res["kernels_ms_per_launch"] = {k: round(v[1] / v[0], 4) for k, v in t.profile().items() if k.startswith(("k_value", "k_scan"))}
        t.profile_enable(False)
    # the route without the new operations: the whole table to the host, numpy there
    b = {}
    b["spectrum_ms"], _ = med(lambda: np.bincount(np.minimum(t.to_vector()[1], 255), minlength=256), base_reps)

    def host_select(lo, hi):
        k, v = t.to_vector()
        m = (v >= lo) & (v <= hi)
        return k[m], v[m]
    b["select_1pct_ms"], _ = med(lambda: host_select(0, 2), base_reps)
    b["select_all_ms"], _ = med(lambda: t.to_vector(), base_reps)
    t.close()
    # erase ~10 % (values 0..25 of 0..255): a fresh table per repetition
    ev, er, bf = [], [], []
    for r in range(reps + 1):
        a, tw = table(uni), table(uni)
        sel = tw.select_values(0, 25, device=True)[0]
        ms, ne = timed(lambda: a.erase_values(0, 25))
        ms2, ne2 = timed(lambda: tw.erase(sel))
        assert ne == ne2 == sel.shape[0] and a.size() == tw.size() == n - ne
        if r:
            ev.append(ms); er.append(ms2)
        a.close(); tw.close()
    res["erase_values_10pct_ms"], res["erase_values_10pct_all"] = round(statistics.median(ev), 3), [round(x, 3) for x in ev]
    res["erase_same_keys_ms"], res["erase_same_keys_all"] = round(statistics.median(er), 3), [round(x, 3) for x in er]
    res["erase_10pct_erased"] = int(ne)
    for r in range(base_reps + 1):
        a = table(uni)

        def host_filter():
            k, v = a.to_vector()
            return a.erase(k[v <= 25])
        ms, ne3 = timed(host_filter)
        assert ne3 == ne
        if r:
            bf.append(ms)
        a.close()
    b["filter_10pct_ms"] = round(statistics.median(bf), 3)
    del uni
    t = table(torch.ones(n, dtype=torch.int32, device="cuda"))
    res["hist_equal_ms"], res["hist_equal_all"] = med(lambda: t.value_histogram(256), reps)
    assert t.value_histogram(256)[1] == n
    t.close()
    res["baseline_to_vector_numpy"] = b
    res["ratio_baseline_over_new"] = {"spectrum": round(b["spectrum_ms"] / res["hist_uniform_ms"], 1), "select_1pct": round(b["select_1pct_ms"] / res["select_1pct_ms"], 1),
                                      "select_all": round(b["select_all_ms"] / res["select_all_ms"], 1),
                                      "filter_10pct": round(b["filter_10pct_ms"] / res["erase_values_10pct_ms"], 1)}
    gb = CAP * res["slot_bytes"] / 1e9
    res["hist_uniform_TBps"] = round(gb / res["hist_uniform_ms"], 2)
    res["hist_equal_TBps"] = round(gb / res["hist_equal_ms"], 2)
    return res


def main(argv):
    quick = "--quick" in argv
    paths = [a for a in argv if not a.startswith("--")]
    out = paths[0] if paths else os.path.join("profiles", "values_timing.json")
    reps, base_reps = (2, 1) if quick else (5, 2)
    res = {"device": torch.cuda.get_device_name(0), "reps": reps, "baseline_reps": base_reps,
           "narrow_rh": run(False, reps, base_reps), "wide_rh": run(True, reps, base_reps)}
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
