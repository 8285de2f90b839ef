"""TEST HELPER (not collected): the definition of kh_mate_rescue (include/kmerhash_amd.h) written out literally on Python integers.

    pattern(qc, q_lo, q_hi, rev)         R as a code list: the mate as it stands, or its reverse complement
    scan(R, win)                         phase 1, the plain full matrix -> (d*, e, last)
    rescue_one(qc, rc, ...)              one request -> (edits, rs, re, span, runs in reference order)
    rescue_model(...)                    (edits, rs, re, span, offsets, ops) of a whole call
Phase 2 is ends_model.extend with clip_cost 0 -- the extension that never stops early: S = F, so the winner is the first level at
which a diagonal holds |A|, the smaller |d| first, then d < 0 -- and E == d* is asserted."""
import numpy as np

from cigar_model import _codes
from edits_model import _match
from ends_model import _comp, extend

NONE, OVER = -1, -2
MAX_READ, MAX_WINDOW = 512, 65536


def pattern(qc, q_lo, q_hi, rev):
    mate = [int(x) for x in qc[q_lo:q_hi]]
    return [_comp(x) for x in reversed(mate)] if rev & 1 else mate


def scan(R, win):
    """D[0][c] = 0, D[i][0] = i, unit costs -> (d* = min D[m][.], the smallest and the greatest column attaining it)"""
    m, W = len(R), len(win)
    prev = list(range(m + 1))                # column 0
    bottom = [prev[m]]
    for c in range(1, W + 1):
        cur = [0] * (m + 1)
        b = win[c - 1]
        for i in range(1, m + 1):
            cur[i] = min(prev[i - 1] + (0 if _match(R[i - 1], b) else 1), prev[i] + 1, cur[i - 1] + 1)
        bottom.append(cur[m])
        prev = cur
    d = min(bottom)
    cols = [c for c, v in enumerate(bottom) if v == d]
    return d, cols[0], cols[-1]


def rescue_one(qc, rc, ref_base, q_lo, q_hi, w_lo, w_hi, rev, max_edits):
    q_lo, q_hi, w_lo, w_hi = int(q_lo), int(q_hi), int(w_lo), int(w_hi)
    m, W = q_hi - q_lo, w_hi - w_lo
    if not (q_lo < q_hi <= len(qc) and 1 <= m <= MAX_READ and ref_base <= w_lo <= w_hi and w_hi - ref_base <= len(rc) and W <= MAX_WINDOW):
        return NONE, 0, 0, 0, []
    R = pattern(qc, q_lo, q_hi, int(rev))
    w0 = w_lo - ref_base
    win = [int(x) for x in rc[w0:w0 + W]]
    d, e, last = scan(R, win)
    if d > max_edits:
        return OVER, 0, 0, 0, []
    A = R[::-1]
    nb = min(m + max_edits, e)
    B = [win[e - 1 - t] for t in range(nb)]
    q, r, E, clip, _, runs = extend(A, B, max_edits, 0)
    assert q == m and clip == 0 and E == d, (q, clip, E, d)          # E == d* by construction
    return d, w_lo + e - r, w_lo + e, last - e, runs[::-1]


def rescue_model(qtext, rtext, q_lo, q_hi, w_lo, w_hi, rev, ref_base=0, max_edits=31):
    """-> (edits int32[n], rs, re, span uint32[n], offsets uint64[n + 1], ops uint32[total])"""
    qc, rc = _codes(qtext), _codes(rtext)
    n = len(q_lo)
    edits, nums = np.zeros(n, dtype=np.int32), np.zeros((3, n), dtype=np.uint32)
    offsets, ops = np.zeros(n + 1, dtype=np.uint64), []
    for j in range(n):
        d, rs, re, span, runs = rescue_one(qc, rc, int(ref_base), q_lo[j], q_hi[j], w_lo[j], w_hi[j], rev[j], int(max_edits))
        edits[j] = d
        nums[:, j] = (rs, re, span)
        ops += [(ln << 4) | op for op, ln in runs]
        offsets[j + 1] = len(ops)
    return edits, nums[0], nums[1], nums[2], offsets, np.array(ops, dtype=np.uint32)
