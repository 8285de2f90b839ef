#!/usr/bin/env python3
"""BASELINE configs[4] shape: the distributed k-mer counter with its query cycle, on synthetic FASTQ.

Reference: benchmark/BenchmarkKmerCounter.cpp:1476-1787 (read the input in file batches -> canonical 31-mers -> counting
insert into dsc::counting_batched_robinhood_map, farmhash storage hash, the table doubling under load) followed by the
query phase of benchmark/BenchmarkKmerIndex.cpp:787-843 (count, find, erase over a sample of the input).

  python benchmark/kmer_counter.py [--gpus N] [--reads R] [--batches B] [--cycle] ...

Every rank owns R reads of ONE synthetic genome (150-bp error-free reads on both strands: the count of every k-mer is then
predictable from the read positions alone, which is what --verify checks at any scale), parses its FASTQ text on its GPU
(kh_kmers_from_fastq: record structure, 2-bit packing and canonicalisation), and feeds the k-mers to the sharded counting
table (kmerhash_amd.dist.ShardedTable.insert_counts: hash partition, RCCL exchange, local std::plus insert; one rank: no
exchange).  Launch model as bench.py: without WORLD_SIZE this process starts the N ranks itself and never touches a GPU.
-k 33..64: 16-byte k-mers {w0, w1} (kh_kmers128_from_fastq) in the wide table behind kmerhash_amd.dist.WideGpuBackend; --verify then
predicts 128-bit k-mers, --out writes 16 + 2 bytes per tuple, --hll-reserve (which feeds the estimator 8-byte k-mers) is refused.
--estimate-reserve pre-sizes the table for every -k in 1..64: each batch's TEXT goes through the fused text -> HyperLogLog pass
(kh_hll_update_from_fastq: no k-mer buffer is read back), the registers are merged over the ranks, and every rank reserves its share
before it inserts; the JSON line then carries "estimate_reserve": {estimate, distinct, rel_err, capacity}.
--histo FILE writes the k-mer spectrum (one pass over every rank's table on its GPU, summed over the ranks), --min-count N drops the
k-mers seen fewer than N times before --cycle / --out (the abundance filter; one marks pass + re-layout per rank, no exchange).
Prints ONE JSON line (rank 0).  Informational driver for SURVEY 8f-2 / configs[4]; the contract benchmark is ../bench.py."""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--reads", type=int, default=2_000_000, help="reads per rank")
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--genome", type=int, default=20_000_000)
    ap.add_argument("--batches", type=int, default=4, help="file batches per rank; 0 = sized from the free HBM the way the reference sizes its file batches "
                                                          "from free memory (BenchmarkKmerCounter.cpp:1508-1590: k-mer estimate x working bytes + 2 x text + table growth <= usable)")
    ap.add_argument("--host-gen", action="store_true", help="generate the reads with numpy on the host (default: on the GPU with torch; neither is timed)")
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--hash", default="farm", choices=["farm", "murmur3avx64", "murmur"])
    ap.add_argument("--chunks", type=int, default=0, help="pieces of the pipelined exchange per batch (0 = 4 when N > 1)")
    ap.add_argument("--cycle", action="store_true", help="run the count / find / erase / count query cycle after the inserts")
    ap.add_argument("--sample-ratio", type=int, default=100, help="queries = every s-th k-mer of the rank's input (BenchmarkKmerIndex -q sampling)")
    ap.add_argument("--hll-reserve", action="store_true", help="pre-size the table from a HyperLogLog estimate per batch instead of doubling under load")
    ap.add_argument("--estimate-reserve", action="store_true", help="pre-size the table per batch from a HyperLogLog estimate taken straight from the batch text "
                                                                   "(fused pass, no k-mer buffer); every -k in 1..64")
    ap.add_argument("--profile", action="store_true", help="per-kernel HIP-event times of the local table (kh_profile_*) in the JSON line")
    ap.add_argument("--verify", action="store_true", help="check size, total count and a sample of 10^5 k-mer counts against the prediction from the read positions")
    ap.add_argument("--out", default="", help="write this rank's (k-mer, count) tuples (BenchmarkKmerCounter.cpp:1022-1211): 8 + 2 bytes each (16 + 2 for -k > 32) like the "
                                               "reference, whose CountType is uint16_t (:184) -- the table's 32-bit counts are truncated to 16 bits in the FILE "
                                               "(= the value the reference's wrapping counter would hold); find / count / --verify use the 32-bit counts")
    ap.add_argument("--histo", default="", help="rank 0 writes the k-mer spectrum here: 'count<TAB>number of distinct k-mers' per non-zero bin, the last bin "
                                                 "('>=N') holding every larger count (ShardedKmerCounter.spectrum: kh_value_histogram per rank + one all-reduce)")
    ap.add_argument("--histo-bins", type=int, default=256, help="bins of --histo (1..16384); the last one is the overflow bin")
    ap.add_argument("--min-count", type=int, default=0, help="after counting, drop the k-mers that occur fewer than N times (ShardedKmerCounter.drop_below: "
                                                             "kh_erase_values on every rank's table); applied before --cycle and --out")
    args = ap.parse_args(argv)
    # refused before any process, GPU or process group is set up
    if not 1 <= args.k <= 64:
        ap.error("-k must be 1..64")
    if args.k > 32 and args.hll_reserve:
        ap.error("--hll-reserve needs -k <= 32 (it feeds the HyperLogLog 8-byte k-mers); --estimate-reserve pre-sizes for every -k")
    if not 1 <= args.histo_bins <= 16384:
        ap.error("--histo-bins must be 1..16384")
    if not 0 <= args.min_count <= 0xFFFFFFFF:
        ap.error("--min-count must be 0..2^32-1")
    return args


def canonical_kmers128_at(genome, positions, k):
    """(n, 2) canonical k-mers {w0, w1} of the genome windows starting at `positions`, 32 < k <= 64 (numpy; A0 C1 G2 T3, first base
    most significant; canonical = the smaller of the k-mer and its reverse complement as 128-bit integers)"""
    pos = np.asarray(positions, dtype=np.int64)
    z = lambda: np.zeros(len(pos), dtype=np.uint64)
    f1, f0, r1, r0 = z(), z(), z(), z()
    two, top = np.uint64(2), np.uint64(62)
    mask_hi = np.uint64((1 << (2 * k - 64)) - 1) if k < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    for j in range(k):
        c = genome[pos + j].astype(np.uint64)
        f1 = ((f1 << two) | (f0 >> top)) & mask_hi
        f0 = (f0 << two) | c
        d = np.uint64(3) - c                        # base j of the window is base k-1-j of the reverse complement: bits 2j, 2j+1
        if 2 * j < 64:
            r0 |= d << np.uint64(2 * j)
        else:
            r1 |= d << np.uint64(2 * j - 64)
    fw_less = (f1 < r1) | ((f1 == r1) & (f0 <= r0))
    return np.ascontiguousarray(np.stack([np.where(fw_less, f0, r0), np.where(fw_less, f1, r1)], axis=1))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(args, argv):
    import torch
    if torch.cuda.device_count() < args.gpus:
        print("[kmer_counter] --gpus %d requested, %d visible" % (args.gpus, torch.cuda.device_count()), file=sys.stderr)
        return 2
    port = _free_port()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(args.gpus), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env))
    rc = 0
    for p in procs:
        p.wait()
        rc = rc or p.returncode
    return rc


def run_rank(args):
    world, rank, local = int(os.environ["WORLD_SIZE"]), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print("[kmer_counter] WORLD_SIZE=%d but --gpus %d" % (world, args.gpus), file=sys.stderr)
        return 2
    import torch
    from kmerhash_amd import kmers as KM
    from kmerhash_amd import dist as khd
    from kmerhash_amd.hll import hyperloglog64
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    grouped = world > 1 or khd.FORCE_COLLECTIVES      # (one rank with the collectives forced: the N > 1 code path over RCCL on one GPU)
    if grouped:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    chunks = args.chunks if args.chunks > 0 else (4 if world > 1 else 1)
    wide = args.k > 32          # 16-byte k-mers {w0, w1}: the wide table behind WideGpuBackend (parse() has checked -k and --hll-reserve)

    # ---- input: this rank's reads of the common genome (generation is not timed)
    t0 = time.perf_counter()
    if args.host_gen:
        seq, genome, starts, rev = KM.synthetic_reads(args.reads, args.read_len, args.genome, genome_seed=7, read_seed=100 + rank)   # one genome, own reads
        fq = KM.fastq_from_sequence_lines(seq, args.reads, args.read_len)
        dfq = torch.from_numpy(fq).to(dev)
        del seq, fq
        positions_of = lambda r: torch.from_numpy((starts if r == rank else KM.read_positions(args.reads, args.read_len, args.genome, 100 + r)[0]).astype(np.int64)).to(dev)
    else:
        dfq, dgenome, dstarts = KM.synthetic_fastq_device(args.reads, args.read_len, args.genome, 7, 100 + rank, local)
        genome = None

        def positions_of(r):
            if r == rank:
                return dstarts
            g = torch.Generator(device=dev); g.manual_seed(100 + r)
            return torch.randint(0, args.genome - args.read_len, (args.reads,), dtype=torch.int64, device=dev, generator=g)
    torch.cuda.synchronize()
    t_gen = time.perf_counter() - t0
    n_text = int(dfq.numel())
    rec = n_text // args.reads
    if args.batches <= 0:
        # the reference adds input files to an iteration while kmer_est x 5 x sizeof(tuple) + 2 x file_size + the table's growth stays
        # under the usable memory (BenchmarkKmerCounter.cpp:1508-1590).  Here, per byte of FASTQ text of a batch: 8 B of k-mer output
        # room + 1 B of masked text (kh_kmers_from_fastq), and per k-mer (0.38 per text byte at 150-bp reads) ~70 B of counting-insert
        # workspace (partition records, lists, exchange buffers); the table (16 B x capacity, twice while it is re-laid out) on top
        free_b, _ = torch.cuda.mem_get_info(dev)
        kmers_per_byte = max(args.read_len - args.k + 1, 1) / float(rec)
        per_byte = 9.0 + kmers_per_byte * 70.0
        table_b = 2 * 16 * (1 << max(7, int(np.ceil(np.log2(max(args.genome, 128) / 0.8)))))
        usable = max(0.6 * free_b - table_b, 0.05 * free_b)
        batch_bytes = min(usable / per_byte, 5.0e8 / kmers_per_byte)           # (a batch stays under 2^29 k-mers: one internal pass of the library,
                                                                               #  whose workspace -- allocated once -- then fits every batch)
        nb = max(1, int(np.ceil(n_text / batch_bytes)))
        args.batches = nb
        batch_note = {"free_hbm": int(free_b), "usable": int(usable), "bytes_per_text_byte": round(per_byte, 1), "batch_text_bytes": int(n_text / nb)}
    else:
        batch_note = None
    cuts = [rec * (args.reads * i // args.batches) for i in range(args.batches + 1)]

    be = khd.WideGpuBackend(local, 128, 0.35, 0.8, args.hash, 43) if wide else khd.GpuBackend(local, "rh", 128, 0.35, 0.8, args.hash, 43)
    st = khd.ShardedTable(be, timing=True)
    reserve = args.hll_reserve or args.estimate_reserve
    hll = hyperloglog64(12, 0, args.hash, 43, local) if reserve else None
    kc = KM.ShardedKmerCounter(st, args.k, True, chunks=chunks, reserve_from_estimate=reserve, hll=hll, estimate_from_text=args.estimate_reserve)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    caps = []
    if args.profile and wide:
        print("[kmer_counter] --profile: the wide table has no per-kernel profile; ignored", file=sys.stderr)
        args.profile = False
    if args.profile:
        be.table.profile_enable(True)
    sync()
    t0 = time.perf_counter()
    t_batch = []
    for i in range(args.batches):
        tb = time.perf_counter()
        kc.add_fastq(dfq[cuts[i]:cuts[i + 1]])
        caps.append(be.table.capacity())
        if args.profile:
            torch.cuda.synchronize()
            t_batch.append(round((time.perf_counter() - tb) * 1e3, 2))
    sync()
    t_ins = time.perf_counter() - t0
    total_local = kc.total_kmers
    size_after = kc.size()
    res = {"kmers_local": total_local, "capacity_per_batch_rank0": caps, "distinct_global": size_after,
           "insert_s": t_ins, "phases_ms_rank0": {k: round(v, 3) for k, v in st.timings().items()}, "batch_sizing": batch_note}
    if args.estimate_reserve:
        # the estimate every rank reserved its share of before the last batch (registers merged over the ranks: collective, not timed)
        from kmerhash_amd.hll import estimate_global
        est = estimate_global(hll, st.group)
        res["estimate_reserve"] = {"estimate": est, "distinct": size_after, "rel_err": abs(est - size_after) / max(size_after, 1),
                                   "capacity": int(be.table.capacity())}
    if args.profile:
        res["batch_ms"] = t_batch
        res["insert_kernels_ms"] = {k: round(v[1], 2) for k, v in sorted(be.table.profile().items(), key=lambda kv: -kv[1][1])}
        be.table.profile_reset()

    # ---- the spectrum of the counts as they stand after counting (collective; not part of insert_s)
    spectrum = None
    if args.histo or args.verify:
        t0 = time.perf_counter()
        spectrum = kc.spectrum(args.histo_bins)
        res["spectrum_s"] = time.perf_counter() - t0
        if args.histo and rank == 0:
            with open(args.histo, "w") as f:
                for c in np.nonzero(spectrum)[0].tolist():
                    f.write("%s%d\t%d\n" % (">=" if c == args.histo_bins - 1 else "", c, int(spectrum[c])))

    ok = True
    exp_survivors = None
    if args.verify:
        # counts predicted from the read positions of ALL ranks (cov[p] = reads covering the k-mer at genome position p)
        d = torch.zeros(args.genome + 1, dtype=torch.int64, device=dev)
        one = torch.ones(args.reads, dtype=torch.int64, device=dev)
        for r in range(world):
            s_r = positions_of(r)
            d.index_add_(0, s_r, one)
            d.index_add_(0, s_r + (args.read_len - args.k + 1), -one)
        dcov = torch.cumsum(d, 0)[:args.genome]
        exp_total = int(dcov.sum().item())
        exp_distinct = int((dcov > 0).sum().item())                # exact when the genome's k-mers are pairwise distinct (k = 31: they are)
        rng = np.random.default_rng(99 + rank)
        pos = rng.integers(0, args.genome - args.k, 100_000)
        cov_at = dcov[torch.from_numpy(pos).to(dev)].cpu().numpy()
        # the spectrum predicted from the read positions: bincount of the coverage over the covered positions, clipped into the last bin
        exp_spectrum = torch.bincount(dcov[dcov > 0].clamp(max=args.histo_bins - 1), minlength=args.histo_bins).cpu().numpy().astype(np.uint64)
        if args.min_count > 0:
            exp_survivors = int((dcov >= max(args.min_count, 1)).sum().item())
        del d, dcov, one
        if genome is None:
            genome = dgenome.cpu().numpy()
        qk = canonical_kmers128_at(genome, pos, args.k) if wide else KM.canonical_kmers_at(genome, pos, args.k)
        pk, vals, found = st.find(torch.from_numpy(qk.view(np.int64)).to(dev))
        as_keys = (lambda a: [tuple(r) for r in a.tolist()]) if wide else (lambda a: a.tolist())       # a wide k-mer is the row (w0, w1)
        got = dict(zip(as_keys(pk.cpu().numpy().view(np.uint64)), ((vals.cpu().numpy().view(np.uint32).astype(np.int64)) * found.cpu().numpy()).tolist()))
        exp = {}
        for kk, c in zip(as_keys(qk), cov_at.tolist()):
            exp[kk] = c                                            # (a k-mer sampled twice has the same position-independent count)
        bad = sum(1 for kk, c in exp.items() if got.get(kk, -1) != (c & 0xFFFFFFFF))
        tot = torch.tensor([total_local], dtype=torch.int64, device=dev)
        if world > 1:
            dist.all_reduce(tot)
        spectrum_ok = bool(np.array_equal(spectrum, exp_spectrum))
        ok = bad == 0 and int(tot.item()) == exp_total and size_after == exp_distinct and spectrum_ok
        res["verify"] = {"ok": bool(ok), "sample_mismatches": bad, "total_kmers": int(tot.item()), "expected_total": exp_total,
                         "expected_distinct": exp_distinct, "spectrum_ok": spectrum_ok}

    if args.min_count > 0:
        sync()
        t0 = time.perf_counter()
        dropped = kc.drop_below(args.min_count)
        sync()
        t_drop = time.perf_counter() - t0
        size_kept = kc.size()
        res["min_count"] = {"n": args.min_count, "dropped_rank0": int(dropped), "size_after": size_kept, "seconds": t_drop}
        if exp_survivors is not None:
            res["min_count"].update(expected_size=exp_survivors, ok=bool(size_kept == exp_survivors))
            ok = ok and size_kept == exp_survivors

    if args.cycle:
        # queries: every s-th k-mer of this rank's first batch (BenchmarkKmerIndex samples the input file the same way)
        km = (KM.kmers128_from_fastq if wide else KM.kmers_from_fastq)(dfq[cuts[0]:cuts[1]], args.k, True, local)
        qs = km[:: args.sample_ratio].contiguous()
        sync()
        t0 = time.perf_counter()
        cyc = kc.cycle(qs)
        sync()
        t_cyc = time.perf_counter() - t0
        nq = int(qs.shape[0])
        # (after --min-count the sample also holds dropped k-mers: every query count() sees must then be found, and none afterwards)
        hits_ok = cyc["count_hits"] == cyc["find_hits"] and (cyc["count_hits"] == nq or args.min_count > 1)
        ok = ok and hits_ok and cyc["count_hits_after"] == 0
        # (ops_per_s: the four operations over their own synchronised times; `seconds` is the wall clock of the whole call, which also
        #  holds torch's result reductions -- their first use loads torch kernels, ~0.1 s once per process)
        res["cycle"] = dict(cyc, queries_local=nq, seconds=t_cyc, ops_per_s=4 * nq * world / (sum(cyc["phase_ms"].values()) * 1e-3), size_after=kc.size(),
                            ok=bool(hits_ok and cyc["count_hits_after"] == 0))
    if args.out:
        k_, v_ = be.table.to_vector()
        # (k > 32: 16 + 2 bytes per tuple, the k-mer as {w0, w1} -- what KmerCounter.write gives)
        recs = np.zeros(len(k_), dtype=np.dtype([("kmer", np.dtype(("<u8", (2,))) if wide else "<u8"), ("count", "<u2")]))
        recs["kmer"] = k_; recs["count"] = v_.astype(np.uint16)
        recs.tofile(args.out + (".%d" % rank if world > 1 else ""))
    if rank == 0:
        res.update({"n_gpus": world, "reads_per_rank": args.reads, "batches": args.batches, "k": args.k, "hash": args.hash,
                    "exchange_pieces": chunks, "fastq_bytes_per_rank": n_text, "bases_per_rank": args.reads * args.read_len, "genome": args.genome,
                    "generation_s": round(t_gen, 2),
                    "kmers_per_s": total_local * world / t_ins, "ok": bool(ok)})
        print(json.dumps(res), flush=True)
    be.table.close()
    if grouped:
        dist.destroy_process_group()
    return 0 if ok else 1


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    args = parse(argv)
    if "WORLD_SIZE" in os.environ:
        return run_rank(args)
    if args.gpus == 1:
        os.environ.update({"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
        return run_rank(args)
    return launch(args, argv)


if __name__ == "__main__":
    sys.exit(main())
