"""TEST HELPER (not collected): the definition of kh_pair_chains (include/kmerhash_amd.h) written out literally on Python integers.
Loops only -- a plain double loop over the candidates of the two mates; numpy carries the inputs in and the outputs out and takes no
part in any decision."""
import numpy as np

NONE = 0xFFFFFFFF      # KH_TARGET_NONE
CAP = 64               # candidates per mate
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def clamp_i32(x):
    return max(I32_MIN, min(I32_MAX, x))


def candidates(a, b, rs, re, sc, use):
    """the chains of [a, b) that take part: the CAP best by (score descending, chain number ascending)"""
    took = [c for c in range(a, b) if (use is None or use[c] != 0) and re[c] > rs[c]]
    return sorted(took, key=lambda c: (-sc[c], c))[:CAP]


def concordant(a, b, rs, re, rev, tid, min_ins, max_ins):
    """is (a, b) a concordant combination of a forward-reverse library?  -> the fragment length, or None"""
    ta, tb = (0, 0) if tid is None else (tid[a], tid[b])
    if ta != tb or ta == NONE or (rev[a] & 1) == (rev[b] & 1):
        return None
    f, r = (b, a) if rev[a] & 1 else (a, b)
    if not (rs[f] <= rs[r] and re[f] <= re[r]):
        return None
    frag = re[r] - rs[f]
    return frag if min_ins <= frag <= max_ins else None


def pq(ps, alt):
    return 0 if ps <= 0 else min(60, (60 * (ps - alt)) // ps)


def pair_one(A, B, rs, re, rev, sc, tid, mq, min_ins, max_ins, pen):
    """one pair: A, B the candidate lists of mate 1 and mate 2 (chain numbers) -> (row1, row2, mapq1, mapq2, tlen1, tlen2, flag, score, nconc)"""
    combos = []
    for a in A:
        for b in B:
            if concordant(a, b, rs, re, rev, tid, min_ins, max_ins) is not None:
                combos.append((sc[a] + sc[b], a, b))
    a0 = A[0] if A else -1      # (the candidate order: the first is the best)
    b0 = B[0] if B else -1
    proper, best = False, None
    if combos:
        best = min(combos, key=lambda t: (-t[0], t[1], t[2]))
        proper = best[0] + pen >= sc[a0] + sc[b0]
    if proper:
        ps, r1, r2 = best
        o1 = [t[0] for t in combos if t[1] != r1]
        o2 = [t[0] for t in combos if t[2] != r2]
        alt1 = max(0, max(o1)) if o1 else 0
        alt2 = max(0, max(o2)) if o2 else 0
        m1, m2 = max(mq[r1], pq(ps, alt1)), max(mq[r2], pq(ps, alt2))
    else:
        r1, r2 = a0, b0
        m1 = mq[r1] if r1 >= 0 else 0
        m2 = mq[r2] if r2 >= 0 else 0
    both = r1 >= 0 and r2 >= 0
    share = both and (tid is None or (tid[r1] == tid[r2] and tid[r1] != NONE))
    t1 = t2 = 0
    if share:
        t = min(I32_MAX, max(re[r1], re[r2]) - min(rs[r1], rs[r2]))
        t1, t2 = (t, -t) if rs[r1] <= rs[r2] else (-t, t)
    flag = (1 if proper else 0) | (2 if both else 0) | (4 if share else 0)
    return r1, r2, m1, m2, t1, t2, flag, (clamp_i32(best[0]) if combos else 0), len(combos)


def pair_model(rs, re, rev, score, offsets, tid=None, use=None, mapq_in=None, min_ins=0, max_ins=1000, unpaired_pen=17):
    """-> (row i32[n_reads], mapq u8[n_reads], tlen i32[n_reads], flag u8[n_pairs], score i32[n_pairs], nconc u32[n_pairs])"""
    ints = lambda a: None if a is None else [int(x) for x in np.asarray(a).ravel()]      # noqa: E731
    rs, re, rev, sc, tid, use, mq, offs = (ints(a) for a in (rs, re, rev, score, tid, use, mapq_in, offsets))
    n = len(rs)
    assert len(re) == n and len(rev) == n and len(sc) == n and all(x is None or len(x) == n for x in (tid, use, mq))
    if mq is None:
        mq = [0] * n
    n_reads = len(offs) - 1
    assert n_reads % 2 == 0 and offs[0] == 0 and offs[-1] == n and all(a <= b for a, b in zip(offs, offs[1:])) and min_ins <= max_ins
    row, mapq, tlen, flag, score_out, nconc = [], [], [], [], [], []
    for p in range(n_reads // 2):
        A = candidates(offs[2 * p], offs[2 * p + 1], rs, re, sc, use)
        B = candidates(offs[2 * p + 1], offs[2 * p + 2], rs, re, sc, use)
        r1, r2, m1, m2, t1, t2, fl, s, nc = pair_one(A, B, rs, re, rev, sc, tid, mq, int(min_ins), int(max_ins), int(unpaired_pen))
        row += [r1, r2]; mapq += [m1, m2]; tlen += [t1, t2]
        flag.append(fl); score_out.append(s); nconc.append(nc)
    arr = lambda v, dt: np.array(v, dtype=np.int64).astype(dt)      # noqa: E731
    return arr(row, np.int32), arr(mapq, np.uint8), arr(tlen, np.int32), arr(flag, np.uint8), arr(score_out, np.int32), arr(nconc, np.uint32)


NAMES = ("row", "mapq", "tlen", "flag", "score", "nconc")
