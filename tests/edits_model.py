"""TEST HELPER (not collected): the definition of kh_chain_edits (include/kmerhash_amd.h) written out literally on Python integers.

    code(b)                         A/a 0, C/c 1, G/g 2, T/t 3, anything else 4
    lev(A, B, rev)                  the full-matrix Levenshtein distance under the match rule (A: query codes, B: the reference stretch
                                    as it lies in rtext; rev: B is read as its reverse complement)
    lev_banded(A, B, rev, max_edits)  the same within the band |diagonal| <= max_edits + 1, OVER beyond max_edits: for long links
    link_model(...)                 out_link of one anchor
    chain_edits_model(...)          (link, edits, over) of a whole call
"""
import numpy as np

NOLINK, OVER = -1, -2
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i
    _CODE[ord(_c.lower())] = _i


def code(b):
    return int(_CODE[b])


def _oriented(B, rev):
    """B as A faces it: codes, reverse-complemented on the reverse strand (an invalid code stays invalid)"""
    B = [int(x) for x in B]
    return [(3 - x if x < 4 else 4) for x in reversed(B)] if rev else B


def _match(a, b):
    return a < 4 and a == b


def lev(A, B, rev=0):
    """textbook DP, (len(A) + 1) x (len(B) + 1) cells; A and B are sequences of codes"""
    A, B = [int(x) for x in A], _oriented(B, rev)
    prev = list(range(len(B) + 1))
    for i in range(1, len(A) + 1):
        cur = [i] + [0] * len(B)
        for j in range(1, len(B) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if _match(A[i - 1], B[j - 1]) else 1))
        prev = cur
    return prev[len(B)]


def lev_banded(A, B, rev, max_edits):
    """the distance if it is <= max_edits, else OVER: only the cells with |j - i| <= max_edits + 1 are filled (a path of at most
    max_edits edits never leaves |j - i| <= max_edits, and the cells beyond the band count as infinite).  Row i is kept by diagonal:
    cell (i, j) sits at t = j - i + w, so (i - 1, j) is the old row's t + 1 and (i - 1, j - 1) its t."""
    A, B = [int(x) for x in A], _oriented(B, rev)
    n, m, w, INF = len(A), len(B), max_edits + 1, 1 << 30
    if abs(n - m) > max_edits:
        return OVER
    prev = [INF] * (2 * w + 2)
    for j in range(0, min(m, w) + 1):
        prev[j + w] = j
    for i in range(1, n + 1):
        cur = [INF] * (2 * w + 2)
        a = A[i - 1]
        for t in range(max(0, w - i), min(2 * w, m - i + w) + 1):
            j = t + i - w
            best = prev[t + 1] + 1
            if j > 0:
                left, diag = cur[t - 1] + 1 if t > 0 else INF, prev[t] + (0 if a < 4 and a == B[j - 1] else 1)
                best = min(best, left, diag)
            cur[t] = best
        prev = cur
    d = prev[m - n + w]
    return d if d <= max_edits else OVER


def link_model(qc, rc, ref_base, qpos, rpos, rev, pred, chain, n_chains, k, max_edits, i, banded=False):
    """out_link[i]; qc / rc: the codes of the two texts"""
    c, p = int(chain[i]), int(pred[i])
    if not (0 <= c < n_chains and 0 <= p < i and int(chain[p]) == c):
        return NOLINK
    qi, qj, ri, rj, rv = int(qpos[i]), int(qpos[p]), int(rpos[i]), int(rpos[p]), int(rev[i]) & 1
    if max(qi, qj, ri, rj) >= 2 ** 31:
        return OVER
    dq, dr = qi - qj, (rj - ri if rv else ri - rj)
    lo, hi = (ri + k - ref_base, rj + k - ref_base) if rv else (rj - ref_base, ri - ref_base)
    if dq < 1 or dr < 1 or qi + k > len(qc) or not (0 <= lo <= len(rc) and 0 <= hi <= len(rc)):
        return OVER
    if abs(dq - dr) > max_edits:
        return OVER
    A, B = qc[qj:qi], rc[lo:hi]
    if banded:
        return lev_banded(A, B, rv, max_edits)
    d = lev(A, B, rv)
    return d if d <= max_edits else OVER


def chain_edits_model(qtext, rtext, qpos, rpos, rev, pred, chain, n_chains, k, ref_base=0, max_edits=31, banded=True):
    """-> (link int32[m], edits uint32[n_chains], over uint32[n_chains])"""
    qc = _CODE[np.frombuffer(bytes(qtext), dtype=np.uint8)] if isinstance(qtext, (bytes, bytearray)) else _CODE[np.asarray(qtext, dtype=np.uint8)]
    rc = _CODE[np.frombuffer(bytes(rtext), dtype=np.uint8)] if isinstance(rtext, (bytes, bytearray)) else _CODE[np.asarray(rtext, dtype=np.uint8)]
    m = len(qpos)
    link = np.zeros(m, dtype=np.int32)
    edits, over = np.zeros(n_chains, dtype=np.uint32), np.zeros(n_chains, dtype=np.uint32)
    for i in range(m):
        d = link_model(qc, rc, ref_base, qpos, rpos, rev, pred, chain, n_chains, k, max_edits, i, banded)
        link[i] = d
        if d >= 0:
            edits[int(chain[i])] += d
        elif d == OVER:
            over[int(chain[i])] += 1
    return link, edits, over
