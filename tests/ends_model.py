"""TEST HELPER (not collected): the definition of kh_chain_ends (include/kmerhash_amd.h) written out literally on Python integers.

    extend(A, B, max_edits, clip_cost)   one end over two code strings that run away from the seed, B already cut to
                                         min(|A| + max_edits, what the reference has left) -> (q, r, e, clip, S, [(op, len), ...] as found)
    end_strings(...)                     (A, B) of one row as code lists, or None for a row that is not looked at
    end_model(...)                       (q, r, edits, clip, runs as stored) of one row
    chain_ends_model(...)                (q, r, edits, clip, offsets, ops) of a whole call
"""
import numpy as np

from cigar_model import DMAX, OP_D, OP_EQ, OP_I, OP_X, _codes, _merge
from edits_model import _match


def extend(A, B, max_edits, clip_cost):
    n, mB = len(A), len(B)

    def hi(d):
        return min(n, mB - d)

    def ext(v, d):
        while v < hi(d) and _match(A[v], B[v + d]):
            v += 1
        return v

    def rank(S, e, d):                       # greater is better: S, then the smaller e, then the smaller |d|, then d < 0
        return (S, -e, -abs(d), 1 if d < 0 else 0)

    F = {0: ext(0, 0)}
    levels = [None]                          # levels[e][d] = (move, pre, F)
    best, e = None, 0
    while True:
        for d, f in F.items():
            cand = rank(f - clip_cost * e, e, d)
            if best is None or cand > best[0]:
                best = (cand, e, d, f)
        if any(f == n for f in F.values()) or e == max_edits:
            break
        G, lev = {}, {}
        for d in range(-DMAX, DMAX + 1):
            cands = []
            if d in F:
                cands.append((OP_X, F[d] + 1))
            if d + 1 in F:
                cands.append((OP_I, F[d + 1] + 1))
            if d - 1 in F:
                cands.append((OP_D, F[d - 1]))
            cands = [(op, v) for op, v in cands if v <= hi(d) and v + d >= 0]      # an invalid candidate is dropped, not clamped
            if not cands:
                continue
            pre = max(v for _, v in cands)
            move = next(op for op, v in cands if v == pre)                       # the first of X, I, D that attains it
            G[d] = ext(pre, d)
            lev[d] = (move, pre, G[d])
        levels.append(lev)
        F = G
        e += 1
    (S, _, _, _), we, wd, wf = best
    back, d = [], wd
    for t in range(we, 0, -1):
        move, pre, f = levels[t][d]
        back.append((move, f - pre))
        d += {OP_X: 0, OP_I: 1, OP_D: -1}[move]
    assert d == 0
    runs = [(OP_EQ, ext(0, 0))]
    for move, eq in reversed(back):
        runs += [(move, 1), (OP_EQ, eq)]
    return wf, wf + wd, we, n - wf, S, _merge(runs)


def _comp(x):
    return 3 - x if x < 4 else 4


def end_strings(qc, rc, ref_base, qpos, rpos, rev, first, last, q_lo, q_hi, k, max_edits, row):
    c, head = row >> 1, row % 2 == 0
    a = int(first[c]) if head else int(last[c])
    if not 0 <= a < len(qpos):
        return None
    q, r, rv, lo, hi = int(qpos[a]), int(rpos[a]), int(rev[a]) & 1, int(q_lo[c]), int(q_hi[c])
    if q >= 2 ** 31 or r >= 2 ** 31:
        return None
    if hi > len(qc) or lo > q or q + k > hi:
        return None
    rr = r - ref_base
    if rr < 0 or rr + k > len(rc):
        return None
    n = q - lo if head else hi - (q + k)
    if n == 0 or n >= 2 ** 28:
        return None
    A = [int(qc[q - 1 - i]) for i in range(n)] if head else [int(x) for x in qc[q + k:hi]]
    down = head != bool(rv)                  # B runs towards the start of rtext: head-forward and tail-reverse
    nb = min(n + max_edits, rr if down else len(rc) - (rr + k))
    B = [int(rc[rr - 1 - j]) for j in range(nb)] if down else [int(rc[rr + k + j]) for j in range(nb)]
    if rv:
        B = [_comp(x) for x in B]
    return A, B


def end_model(qc, rc, ref_base, qpos, rpos, rev, first, last, q_lo, q_hi, k, max_edits, clip_cost, row):
    s = end_strings(qc, rc, ref_base, qpos, rpos, rev, first, last, q_lo, q_hi, k, max_edits, row)
    if s is None:
        return 0, 0, 0, 0, []
    A, B = s
    q, r, e, clip, _, runs = extend(A, B, max_edits, clip_cost)
    return q, r, e, clip, (runs[::-1] if row % 2 == 0 else runs)          # a head is stored in read order


def chain_ends_model(qtext, rtext, qpos, rpos, rev, first, last, q_lo, q_hi, k, ref_base=0, max_edits=31, clip_cost=4):
    """-> (q, r, edits, clip: uint32[2 n_chains]; offsets uint64[2 n_chains + 1]; ops uint32[total])"""
    qc, rc = _codes(qtext), _codes(rtext)
    rows = 2 * len(first)
    nums = np.zeros((4, rows), dtype=np.uint32)
    offsets, ops = np.zeros(rows + 1, dtype=np.uint64), []
    for row in range(rows):
        *four, runs = end_model(qc, rc, ref_base, qpos, rpos, rev, first, last, q_lo, q_hi, k, max_edits, clip_cost, row)
        nums[:, row] = four
        ops += [(n << 4) | op for op, n in runs]
        offsets[row + 1] = len(ops)
    return nums[0], nums[1], nums[2], nums[3], offsets, np.array(ops, dtype=np.uint32)
