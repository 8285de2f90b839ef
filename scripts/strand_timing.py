"""The strand stamp, stranded index builds and anchors on one MI355X, on the input of scripts/minimizer_timing.py and
scripts/syncmer_timing.py (whose helpers this script uses): a random genome of --n bases with one poly-A stretch.  Call-level times (host
clock, device synchronised before and after the call), one warm-up, then the median of --reps (10); a fresh index for every repetition.
One process measures one library, the one of the package in the working directory.

  --mode all     (a) stamp_strand (k = 15) over the closed-syncmer positions (s = 11), over all window positions, and over the positions
                 inside the poly-A stretch, each with its byte model (8 B per position + 2 text bytes per compared pair) at 8 TB/s;
                 (b) build_sequences stranded against not stranded in this one process: all windows k = 15, s = 11, wide k = 63 with
                 s = 31, with k_pos_strand's own time from one profiled build each; (c) anchors() of a --query-base query cut from the
                 text against find_sequences() of the same query on the same stranded index
  --mode base    only build_sequences of indexes that are NOT stranded (all windows k = 15, s = 11, wide k = 63 with s = 31): the calls
                 exist in the parent commit too, so processes started in a built checkout of the parent commit (this script given by
                 its path) and processes started here can alternate into one --out file (the timing condition: inside the spread of
                 the parent's own repeats, since the same kernels are launched)

  python scripts/strand_timing.py --out profiles/strand_timing.json
  (cd ../parent && python ../here/scripts/strand_timing.py --mode base --tag parent_1 --out ../here/profiles/strand_timing.json)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from minimizer_timing import genome_text, runs, summary, timed  # noqa: E402

K, S = 15, 11
KW, SW = 63, 31
HBM_BYTES_PER_MS = 8e9          # 8 TB/s


def build_runs(cls, text, reps, torch, **kw):
    out = []
    for _ in range(reps + 1):
        x = cls(**kw)
        ms, _ = timed(lambda: x.build_sequences(text), torch)
        x.close()
        out.append(round(ms, 3))
    return out[1:]


def profiled_build(cls, text, **kw):
    x = cls(**kw)
    x.profile_enable(True)
    x.build_sequences(text)
    prof = {n: {"launches": c, "ms": round(ms, 3)} for n, (c, ms) in sorted(x.profile().items())}
    total = x.total()
    x.close()
    return prof, total


FORMS = (("all_windows_k15", "KmerPositionIndex", dict(k=K)), ("syncmers_k15_s11", "KmerPositionIndex", dict(k=K, s=S)),
         ("wide_syncmers_k63_s31", "WideKmerPositionIndex", dict(k=KW, s=SW)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000, help="bases of text")
    ap.add_argument("--poly-a", type=int, default=1_200_000)
    ap.add_argument("--query-bases", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mode", choices=["all", "base"], default="all")
    ap.add_argument("--tag", default=None, help="key of this process's record (default: the mode)")
    ap.add_argument("--out", default="profiles/strand_timing.json")
    a = ap.parse_args()
    import torch

    import kmerhash_amd as kh
    from kmerhash_amd import kmers as KM
    if not torch.cuda.is_available():
        sys.exit("strand_timing.py measures on a GPU; none is visible")
    text = genome_text(a.n, a.poly_a, 7, torch)
    rec = {"version": kh._capi.lib().kh_version().decode(), "device": torch.cuda.get_device_name(0), "text_bytes": a.n, "poly_a": a.poly_a,
           "reps": a.reps,
           "method": "host clock around the call, device synchronised before and after; one warm-up, median of reps; fresh index per repetition"}
    if a.mode == "base":
        for name, cls, kw in FORMS:
            rec["build_" + name] = summary(build_runs(getattr(kh, cls), text, a.reps, torch, **kw))
            print("base", name, rec["build_" + name]["median_ms"], flush=True)
    else:
        # (a) the stamp alone.  Byte model: 4 B read + 4 B written per position, 2 text bytes per compared pair -- the public call
        #     compares all ceil(k / 2) pairs (it also checks every byte)
        _, spos = KM.syncmers_from_sequence(text, K, S)
        apos = torch.arange(0, a.n - K + 1, dtype=torch.int32, device="cuda")
        ppos = torch.arange(a.n // 3, a.n // 3 + a.poly_a - K + 1, dtype=torch.int32, device="cuda")
        stamp = {}
        for name, pos in (("syncmer_positions_k15_s11", spos), ("all_window_positions", apos), ("poly_a_positions", ppos)):
            r = summary(runs(lambda: KM.stamp_strand(text, pos, K), a.reps, torch))
            m = int(pos.numel())
            bits = KM.stamp_strand(text, pos, K) & 1
            model_bytes = m * (8 + 2 * ((K + 1) // 2))
            r.update(positions=m, reverse_fraction=round(float(bits.float().mean()), 4), byte_model_ms=round(model_bytes / HBM_BYTES_PER_MS, 4),
                     over_byte_model=round(r["median_ms"] / (model_bytes / HBM_BYTES_PER_MS), 2),
                     positions_per_us=round(m / r["median_ms"] / 1e3, 1))
            stamp[name] = r
            print("stamp", name, r["median_ms"], r["byte_model_ms"], flush=True)
            del bits
        del apos, ppos, spos
        rec["stamp_strand"] = stamp
        # (b) builds, stranded against not stranded, in this process
        builds = {}
        for name, cls, kw in FORMS:
            plain = summary(build_runs(getattr(kh, cls), text, a.reps, torch, **kw))
            stranded = summary(build_runs(getattr(kh, cls), text, a.reps, torch, stranded=True, **kw))
            prof, total = profiled_build(getattr(kh, cls), text, stranded=True, **kw)
            pairs_ms = prof["k_pos_strand"]["ms"]
            model_bytes = total * (8 + 2 * 4.0 / 3.0)       # the index-internal stamp stops at the first difference: 4/3 pairs on random text
            builds[name] = {"plain": plain, "stranded": stranded, "stranded_over_plain": round(stranded["median_ms"] / plain["median_ms"], 4),
                            "pairs": total, "k_pos_strand_ms": pairs_ms, "k_pos_strand_byte_model_ms": round(model_bytes / HBM_BYTES_PER_MS, 4),
                            "k_pos_strand_over_byte_model": round(pairs_ms / (model_bytes / HBM_BYTES_PER_MS), 2), "profiled_stranded_build": prof}
            print("build", name, plain["median_ms"], stranded["median_ms"], pairs_ms, flush=True)
        rec["build_sequences"] = builds
        # (c) anchors against find_sequences, the same query on the same stranded index (closed syncmers k = 15, s = 11)
        q0 = a.n // 2
        query = text[q0: q0 + a.query_bases].contiguous()
        x = kh.KmerPositionIndex(k=K, s=S, stranded=True)
        x.build_sequences(text)
        f = summary(runs(lambda: x.find_sequences(query), a.reps, torch))
        an = summary(runs(lambda: x.anchors(query), a.reps, torch))
        qpos, rpos, rev = x.anchors(query)
        on_diag = int(((rpos - qpos == q0) & (rev == 0)).sum())
        hits = int(rpos.numel())
        expand_bytes = hits * 13 + int(x.find_sequences(query)[0].numel()) * 20
        rec["anchors"] = {"query_bases": a.query_bases, "find_sequences": f, "anchors": an, "anchors_over_find_sequences": round(an["median_ms"] / f["median_ms"], 4),
                          "hits": hits, "hits_on_the_forward_diagonal": on_diag, "reverse_hits": int(rev.sum()),
                          "added_byte_model_ms": round(expand_bytes / HBM_BYTES_PER_MS, 4)}
        print("anchors", f["median_ms"], an["median_ms"], hits, on_diag, flush=True)
        x.close()
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    out[a.tag or a.mode] = rec
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
