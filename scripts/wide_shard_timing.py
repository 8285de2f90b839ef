"""Timings behind profiles/wide_shard_timing.json (one GPU, one process, both sides of every comparison in the same run):
  1. kh_wide_shard_permute (16-byte keys) next to kh_shard_permute (64-bit keys): count-only call and full call at n pairs, p ranks;
     scatter = full - count-only.  Bytes: count reads the keys, scatter reads keys + values and writes keys + values.
  2. the streamed wide insert of n keys in 4 device pieces next to one kh_wide_insert of the same keys.
  3. with --sharded: ShardedTable over WideGpuBackend on ONE rank with the collectives forced (KH_DIST_FORCE_COLLECTIVES=1, RCCL) next
     to the unsharded wide insert.
Medians of --reps runs after one warm-up; HIP events around the calls (they include the calls' host work and synchronisation)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", type=int, default=100_000_000)
    ap.add_argument("-p", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sharded", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.sharded:
        os.environ["KH_DIST_FORCE_COLLECTIVES"] = "1"
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            import socket
            s = socket.socket()
            s.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(s.getsockname()[1])
            s.close()
    import torch
    import kmerhash_amd as kh
    from kmerhash_amd import _capi as K
    from kmerhash_amd import dist as khd
    L = K.lib()
    n, p = args.n, args.p
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    wk = torch.randint(-(1 << 62), 1 << 62, (n, 2), dtype=torch.int64, device="cuda", generator=g)
    nk = wk[:, 0].contiguous()
    vals = torch.arange(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        fn()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    res = {"n": n, "p": p, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    counts = (C.c_uint64 * p)()
    for name, fn, keys, kbytes in (("wide", L.kh_wide_shard_permute, wk, 16), ("narrow", L.kh_shard_permute, nk, 8)):
        ok, ov = torch.empty_like(keys), torch.empty_like(vals)

        def call(full):
            st = fn(1, khd.DIST_SEED, p, keys.data_ptr(), vals.data_ptr(), n, ok.data_ptr() if full else None, ov.data_ptr() if full else None,
                    counts, 0, stream)
            assert st == K.KH_OK, st
        c_ms, f_ms = timed(lambda: call(False)), timed(lambda: call(True))
        s_ms = f_ms - c_ms
        res["shard_" + name] = {"count_only_ms": round(c_ms, 3), "full_ms": round(f_ms, 3), "scatter_ms": round(s_ms, 3),
                                "count_GBps": round(n * kbytes / c_ms / 1e6, 1), "scatter_GBps": round(n * 2 * (kbytes + 4) / s_ms / 1e6, 1),
                                "bytes_per_pair": {"count": kbytes, "scatter": 2 * (kbytes + 4)}}
        del ok, ov

    # streamed insert in 4 device pieces vs one insert (fresh tables every repetition; construction and release are not timed)
    bnd = [n * i // 4 for i in range(5)]

    def fresh(cls):
        return cls(128, 0.35, 0.8)

    def once(streamed):
        t = fresh(kh.hashmap_robinhood_doubling_wide_stream)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        m = torch.cuda.Event(enable_timing=True)
        if streamed:
            t.insert_begin(n)
            for i in range(4):
                t.insert_feed(wk[bnd[i]:bnd[i + 1]], vals[bnd[i]:bnd[i + 1]])
            m.record()          # what the feeds queued (the counting half of the partition) ends here; the rest is insert_end
            got = t.insert_end()
        else:
            m.record()
            got = t.insert(wk, vals)
        b.record()
        torch.cuda.synchronize()
        t.close()
        return a.elapsed_time(b), got, a.elapsed_time(m)
    for streamed in (False, True):
        once(streamed)
        runs = [once(streamed) for _ in range(args.reps)]
        r = {"ms": round(statistics.median(r[0] for r in runs), 3), "n_inserted": runs[0][1]}
        if streamed:
            r["feeds_ms"] = round(statistics.median(r_[2] for r_ in runs), 3)       # work that can overlap the transfers of later pieces
        res["insert_streamed_4_pieces" if streamed else "insert_plain"] = r

    if args.sharded:
        import torch.distributed as dist
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))

        def sharded_once():
            st = khd.ShardedTable(khd.WideGpuBackend(0))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            got = st.insert(wk, vals, chunks=4)
            b.record()
            torch.cuda.synchronize()
            st.local.close()
            return a.elapsed_time(b), got
        sharded_once()
        runs = [sharded_once() for _ in range(args.reps)]
        res["insert_sharded_one_rank_forced_collectives_4_pieces"] = {"ms": round(statistics.median(r[0] for r in runs), 3), "n_inserted": runs[0][1]}
        dist.destroy_process_group()
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
