"""TEST HELPER (not collected): the definition of kh_chain_select (include/kmerhash_amd.h) written out literally on Python integers.
Loops only; numpy carries the inputs in and the outputs out and takes no part in any decision."""
import numpy as np


def covers(cs, ce, ps, pe, mask_pct):
    """does p = [ps, pe) cover c = [cs, ce)?"""
    len_c, len_p = max(0, ce - cs), max(0, pe - ps)
    ov = max(0, min(ce, pe) - max(cs, ps))
    return 100 * ov >= mask_pct * min(len_c, len_p)


def mapq_of(s, sub, cnt):
    if s <= 0:
        return 0
    return min(60, (60 * (s - sub) * min(cnt, 10) * min(s, 100)) // (1000 * s))


def select_group(qs, qe, sc, cnt, mask_pct, pri_pct, best_n):
    """one group, lists of Python integers -> (parent, rank, mapq, flag, sub, nsub) as lists of local chain numbers / values, best"""
    n = len(qs)
    order = sorted(range(n), key=lambda c: (-sc[c], c))
    parent, rank, mapq, flag, sub, nsub = [0] * n, [0] * n, [0] * n, [0] * n, [0] * n, [0] * n
    primaries, seen, first_sub = [], {}, {}
    for r, c in enumerate(order):
        rank[c] = r
        par = None
        for p in primaries:                       # rank order: the first that covers is the covering primary of smallest rank
            if covers(qs[c], qe[c], qs[p], qe[p], mask_pct):
                par = p
                break
        if par is None:
            primaries.append(c)
            parent[c], flag[c], seen[c] = c, 3, 0
        else:
            parent[c] = par
            if seen[par] == 0:
                first_sub[par] = sc[c]
            if 100 * sc[c] >= pri_pct * sc[par] and seen[par] < best_n:
                flag[c] = 2
            seen[par] += 1
    for p in primaries:
        nsub[p] = seen[p]
        sub[p] = max(0, first_sub[p]) if seen[p] else 0
        mapq[p] = mapq_of(sc[p], sub[p], cnt[p])
    return parent, rank, mapq, flag, sub, nsub, (order[0] if n else -1)


def select_model(q_start, q_end, score, count, offsets=None, mask_pct=50, pri_pct=80, best_n=5):
    """-> (parent i32, rank u32, mapq u8, flag u8, sub i32, nsub u32, best i32) as numpy arrays"""
    qs, qe, sc, cn = ([int(x) for x in np.asarray(a).ravel()] for a in (q_start, q_end, score, count))
    n = len(qs)
    assert len(qe) == n and len(sc) == n and len(cn) == n
    offs = [0, n] if offsets is None else [int(x) for x in np.asarray(offsets).ravel()]
    assert offs[0] == 0 and offs[-1] == n and all(a <= b for a, b in zip(offs, offs[1:]))
    out = [[0] * n for _ in range(6)]
    best = []
    for a, b in zip(offs, offs[1:]):
        res = select_group(qs[a:b], qe[a:b], sc[a:b], cn[a:b], mask_pct, pri_pct, best_n)
        for i in range(b - a):
            out[0][a + i] = a + res[0][i]
            for f in range(1, 6):
                out[f][a + i] = res[f][i]
        best.append(a + res[6] if b > a else -1)
    dts = (np.int32, np.uint32, np.uint8, np.uint8, np.int32, np.uint32)
    return tuple(np.array(o, dtype=np.int64).astype(dt) for o, dt in zip(out, dts)) + (np.array(best, dtype=np.int64).astype(np.int32),)


NAMES = ("parent", "rank", "mapq", "flag", "sub", "nsub", "best")
