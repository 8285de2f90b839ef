"""TEST HELPER (not collected): Python-integer model of kh_chain_anchors (include/kmerhash_amd.h), loops only.  It states the definition
directly: the banded look-back DP per segment (f, pred), the best chain end reachable through every anchor (g), the best child, the
start rule that partitions the anchors into chains, and the filtered, numbered chain table.  Nothing is vectorised and nothing is
shared with the kernels; every quantity is a Python int."""
import collections

import numpy as np

POS_INVALID = 0xFFFFFFFF
Chained = collections.namedtuple("Chained", "score pred chain first last count cscore g best_child start")


def ilog2(x):
    return x.bit_length() - 1


def cost(k, dd):
    return 0 if dd == 0 else ((k * dd) >> 7) + (ilog2(dd) >> 1)


def segments(m, seg_offsets):
    if seg_offsets is None:
        return [(0, m)]
    so = [int(x) for x in seg_offsets]
    assert so[0] == 0 and so[-1] == m and all(x <= y for x, y in zip(so, so[1:])), "seg_offsets must ascend from 0 to m"
    return list(zip(so[:-1], so[1:]))


def chain(qpos, rpos, rev, k, seg_offsets=None, lookback=64, max_gap=5000, band=500, min_score=40, min_count=3):
    q, r = [int(x) for x in qpos], [int(x) for x in rpos]
    v = [int(x) & 1 for x in rev]
    m = len(q)
    ok = [q[i] < 2 ** 31 and r[i] < 2 ** 31 for i in range(m)]
    f, pred = [k] * m, [-1] * m
    for a, b in segments(m, seg_offsets):
        for i in range(a, b):
            if not ok[i]:
                continue
            best, bp = k, -1
            qi, ri, vi = q[i], r[i], v[i]
            for j in range(max(a, i - lookback), i):
                if v[j] != vi or not ok[j]:
                    continue
                dq = qi - q[j]
                if not 1 <= dq <= max_gap:
                    continue
                dr = r[j] - ri if vi else ri - r[j]
                if not 1 <= dr <= max_gap:
                    continue
                dd = abs(dq - dr)
                if dd > band:
                    continue
                cand = f[j] + min(dq, dr, k) - cost(k, dd)
                if cand > k and cand >= best:           # j ascends: >= keeps the largest j among equals
                    best, bp = cand, j
            f[i], pred[i] = best, bp
    # g(i) = max(f(i), g of the children); a child has a larger index than its parent
    g = list(f)
    children = [[] for _ in range(m)]
    for i in range(m - 1, -1, -1):
        if pred[i] >= 0:
            children[pred[i]].append(i)
            g[pred[i]] = max(g[pred[i]], g[i])
    best_child = [-1] * m
    for j in range(m):
        for c in sorted(children[j]):
            if best_child[j] < 0 or g[c] > g[best_child[j]]:   # ascending c, strict: the smallest index among equals
                best_child[j] = c
    start = [pred[i] < 0 or best_child[pred[i]] != i for i in range(m)]
    head = [0] * m
    count, last = {}, {}
    for i in range(m):
        head[i] = i if start[i] else head[pred[i]]
        count[head[i]] = count.get(head[i], 0) + 1
        last[head[i]] = i
    number, first, lasts, counts, scores = {}, [], [], [], []
    for s in sorted(count):
        sc = f[last[s]] - (0 if pred[s] < 0 else f[pred[s]])
        if sc >= min_score and count[s] >= min_count:
            number[s] = len(first)
            first.append(s); lasts.append(last[s]); counts.append(count[s]); scores.append(sc)
    ch = [number.get(head[i], -1) for i in range(m)]
    return Chained(np.array(f, dtype=np.int32), np.array(pred, dtype=np.int32), np.array(ch, dtype=np.int32), np.array(first, dtype=np.uint32),
                   np.array(lasts, dtype=np.uint32), np.array(counts, dtype=np.uint32), np.array(scores, dtype=np.int32), g, best_child, start)


# ---- the synthetic case of the chaining tests: a random reference, a query cut from it with substitutions and a deletion, followed by
#      the reverse complement of another piece
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def synthetic_texts(n=20000, seed=1):
    import random
    rng = random.Random(seed)
    ref = "".join(rng.choice("ACGT") for _ in range(n))
    qa = list(ref[5000:7000])
    for p in (300, 900, 1500):
        qa[p] = COMP[qa[p]]
    del qa[1200:1203]
    return ref, "".join(qa) + revcomp(ref[12000:13000])


def all_window_anchors(ref, query, k):
    """(qpos, rpos, rev) of every canonical k-mer match, in query order and then ascending rpos -- the order of the index's anchors()"""
    def canon(s):
        t = revcomp(s)
        return (t, 1) if t < s else (s, 0)
    idx = {}
    for p in range(len(ref) - k + 1):
        c, b = canon(ref[p:p + k])
        idx.setdefault(c, []).append((p, b))
    q, r, rev = [], [], []
    for p in range(len(query) - k + 1):
        c, b = canon(query[p:p + k])
        for rp, rb in idx.get(c, []):
            q.append(p); r.append(rp); rev.append(b ^ rb)
    return q, r, rev
