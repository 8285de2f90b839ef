"""The sharded position index on one MI355X: ONE rank over RCCL with KH_DIST_FORCE_COLLECTIVES=1 (every exchange is a self-exchange
through RCCL), against the single-GPU index on the same text in the same process -- a random genome of --n bases with one poly-A
stretch (the input of scripts/index_timing.py), k = 15, all windows and w = --w.  Call-level times (host clock, device synchronised
before and after the call), one warm-up, then the median of --reps (10); a fresh index for every build repetition.

  --mode all     (a) ShardedKmerPositionIndex.build_sequences against KmerPositionIndex.build_sequences (the difference: permute + self-exchange),
                 (b) find of --queries keys sharded against the local find, with the per-phase split of the timing=True spans and the
                     time of kh_csr_unpermute alone,
                 (c) kh_csr_unpermute against its byte model at 8 TB/s: two scans (12 B and 16 B per query: the counts read twice, the
                     offsets written), the scatter (12 B read + 8 B written per query) and 8 B per moved position
  --mode base    KmerPositionIndex.build_sequences and find only: they exist in the parent commit too, so processes started in a built
                 checkout of the parent commit (this script given by its path) and processes started here can alternate into one
                 --out file (the timing condition: both calls stay inside the spread of the parent's own repeats)

  python scripts/dist_index_timing.py --out profiles/dist_index_timing.json
  (cd ../parent && python ../here/scripts/dist_index_timing.py --mode base --tag parent_1 --out ../here/profiles/dist_index_timing.json)
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time

sys.path.insert(0, ".")

K = 15
STREAM_BPS = 8e12


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


def build_runs(make, close, text, reps, torch):
    out = []
    for _ in range(reps + 1):
        x = make()
        ms, _ = timed(lambda: x.build_sequences(text), torch)
        close(x)
        out.append(round(ms, 3))
    return out[1:]


def sample_queries(kh, text, nq, torch):
    """nq k-mers of the text in random order: hits, the poly-A k-mer (all A = 0) ONCE among them -- one query with every position of
    the stretch; the other draws that fell into the stretch become the k-mer of the text's first window"""
    from kmerhash_amd import kmers as KM
    km = KM.kmers_from_sequence(text, K, True)
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    q = km[torch.randint(0, km.numel(), (nq,), dtype=torch.int64, device="cuda", generator=g)]
    q = torch.where(q == 0, km[0], q).contiguous()
    q[nq // 2] = 0
    return q


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text")
    ap.add_argument("--poly-a", type=int, default=1_200_000)
    ap.add_argument("--w", type=int, default=10)
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mode", choices=["all", "base"], default="all")
    ap.add_argument("--tag", default=None, help="key of this process's record (default: the mode)")
    ap.add_argument("--out", default="profiles/dist_index_timing.json")
    a = ap.parse_args()
    os.environ["KH_DIST_FORCE_COLLECTIVES"] = "1"
    import torch

    import kmerhash_amd as kh
    if not torch.cuda.is_available():
        sys.exit("dist_index_timing.py measures on a GPU; none is visible")
    torch.cuda.set_device(0)
    text = genome_text(a.n, a.poly_a, 7, torch)
    rec = {"version": kh._capi.lib().kh_version().decode(), "library": os.path.basename(kh._capi.LIB), "device": torch.cuda.get_device_name(0),
           "k": K, "text_bytes": a.n, "poly_a": a.poly_a, "reps": a.reps, "queries": a.queries,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps; fresh index per build repetition"}
    q = sample_queries(kh, text, a.queries, torch)
    single = lambda **kw: (lambda: kh.KmerPositionIndex(k=K, **kw))
    rec["single_build_all_windows"] = summary(build_runs(single(), lambda x: x.close(), text, a.reps, torch))
    x = kh.KmerPositionIndex(k=K)
    x.build_sequences(text)
    rec["single_find"] = summary(runs(lambda: x.find(q), a.reps, torch))
    print("single build", rec["single_build_all_windows"]["median_ms"], "find", rec["single_find"]["median_ms"], flush=True)
    if a.mode == "all":
        import torch.distributed as dist
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(port))
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        from kmerhash_amd import dist as khd
        assert khd.FORCE_COLLECTIVES
        sharded = lambda **kw: (lambda: kh.ShardedKmerPositionIndex(kh.IndexGpuBackend(0, k=K, **kw), timing=True))
        close = lambda s_: s_.local.close()
        # (a) build
        rec["sharded_build_all_windows"] = summary(build_runs(sharded(), close, text, a.reps, torch))
        rec["single_build_w=%d" % a.w] = summary(build_runs(single(w=a.w), lambda x_: x_.close(), text, a.reps, torch))
        rec["sharded_build_w=%d" % a.w] = summary(build_runs(sharded(w=a.w), close, text, a.reps, torch))
        st = sharded()()
        st.build_sequences(text)
        s2 = sharded()()
        s2.build_sequences(text)
        rec["sharded_build_phases_ms"] = {k_: round(v, 3) for k_, v in s2.timings().items()}
        close(s2)
        print("sharded build", rec["sharded_build_all_windows"]["median_ms"], "w", rec["sharded_build_w=%d" % a.w]["median_ms"],
              "single w", rec["single_build_w=%d" % a.w]["median_ms"], flush=True)
        # (b) find
        assert st.total() == x.total()
        rec["sharded_find"] = summary(runs(lambda: st.find(q), a.reps, torch))
        st.timings()
        offs, pos = st.find(q)
        rec["sharded_find_phases_ms"] = {k_: round(v, 3) for k_, v in st.timings().items()}
        o1, p1 = x.find(q)
        assert torch.equal(offs, o1) and torch.equal(pos, p1)
        total = int(pos.numel())
        # (c) kh_csr_unpermute alone: the local CSR of a random permutation of the batch, put back
        perm = torch.randperm(a.queries, device="cuda")
        cnt = (o1[1:] - o1[:-1]).to(torch.int32)
        origin = perm.to(torch.int32)
        cperm = cnt[perm].contiguous()
        _, pperm = x.find(q[perm].contiguous())
        be = st.b
        rec["csr_unpermute"] = summary(runs(lambda: be.csr_unpermute(cperm, pperm, origin), a.reps, torch))
        o2, p2 = be.csr_unpermute(cperm, pperm, origin)
        assert torch.equal(o2, o1) and torch.equal(p2, p1)
        model_bytes = a.queries * (12 + 16 + 20) + total * 8
        rec["csr_unpermute"].update(positions=total, model_bytes=model_bytes, model_ms=round(model_bytes / STREAM_BPS * 1e3, 4),
                                    factor=round(rec["csr_unpermute"]["median_ms"] / (model_bytes / STREAM_BPS * 1e3), 2))
        rec["csr_unpermute_counts_only"] = summary(runs(lambda: be.csr_unpermute(cperm, None, origin), a.reps, torch))
        print("find sharded", rec["sharded_find"]["median_ms"], json.dumps(rec["sharded_find_phases_ms"]), "unpermute", rec["csr_unpermute"]["median_ms"],
              "x model", rec["csr_unpermute"]["factor"], flush=True)
        close(st)
        dist.destroy_process_group()
    x.close()
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out[a.tag or a.mode] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
