"""TEST HELPER (not collected): the definition of kh_chain_cigars (include/kmerhash_amd.h) written out literally on Python integers.

    OP_I, OP_D, OP_EQ, OP_X          the BAM operation codes 1, 2, 7, 8; a run is (len << 4) | op
    canonical(A, B, bound)           the canonical alignment of two oriented code strings among the distances 0..bound
                                     -> (e, [(op, len), ...]) or None where the target is not reached by `bound`
    apply_ops(A, B, runs)            walks a row over A and B -> (consumed A, consumed B, X, I, D) or None where a run contradicts the texts
    row_model(...)                   the row of one anchor as a list of uint32
    chain_cigars_model(...)          (offsets, ops, ins, dels) of a whole call
    parse(text)                      "2=1I3=" -> [(7, 2), (1, 1), (7, 3)]
"""
import numpy as np

from edits_model import _CODE, _match, _oriented

OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
LETTER = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
DMAX = 31


def _merge(runs):
    out = []
    for op, n in runs:
        if n == 0:
            continue
        if out and out[-1][0] == op:
            out[-1] = (op, out[-1][1] + n)
        else:
            out.append((op, n))
    return out


def canonical(A, B, bound):
    """A, B: code sequences, B already oriented as A faces it"""
    n, mB = len(A), len(B)
    target = mB - n
    if abs(target) > DMAX:
        return None

    def hi(d):
        return min(n, mB - d)

    def ext(v, d):
        while v < hi(d) and _match(A[v], B[v + d]):
            v += 1
        return v

    F = {0: ext(0, 0)}
    levels = [None]                      # levels[e][d] = (move, pre, F)
    e = 0
    while True:
        if F.get(target) == n:
            break
        if e == bound:
            return None
        G, lev = {}, {}
        for d in range(-DMAX, DMAX + 1):
            cands = []
            if d in F:
                cands.append((OP_X, F[d] + 1))
            if d + 1 in F:
                cands.append((OP_I, F[d + 1] + 1))
            if d - 1 in F:
                cands.append((OP_D, F[d - 1]))
            cands = [(op, v) for op, v in cands if v <= hi(d) and v + d >= 0]
            if not cands:
                continue
            pre = max(v for _, v in cands)
            move = next(op for op, v in cands if v == pre)          # the first of X, I, D that attains it
            G[d] = ext(pre, d)
            lev[d] = (move, pre, G[d])
        levels.append(lev)
        F = G
        e += 1
    # traceback from (e, target) to (0, 0)
    back, d = [], target
    for t in range(e, 0, -1):
        move, pre, f = levels[t][d]
        back.append((move, f - pre))
        d += {OP_X: 0, OP_I: 1, OP_D: -1}[move]
    assert d == 0
    f0 = ext(0, 0)
    runs = [(OP_EQ, f0)]
    for move, eq in reversed(back):
        runs += [(move, 1), (OP_EQ, eq)]
    return e, _merge(runs)


def apply_ops(A, B, runs):
    i = j = x = ins = dels = 0
    for op, n in runs:
        if n < 1:
            return None
        if op == OP_I:
            i += n; ins += n
        elif op == OP_D:
            j += n; dels += n
        elif op in (OP_EQ, OP_X):
            if i + n > len(A) or j + n > len(B):
                return None
            for t in range(n):
                if _match(A[i + t], B[j + t]) != (op == OP_EQ):
                    return None
            i += n; j += n
            x += n if op == OP_X else 0
        else:
            return None
    return i, j, x, ins, dels


def row_model(qc, rc, ref_base, qpos, rpos, rev, pred, chain, n_chains, k, link, i):
    """-> (runs as (op, len) pairs, chain number)"""
    c, p = int(chain[i]), int(pred[i])
    if not (0 <= c < n_chains and 0 <= p < i and int(chain[p]) == c):
        return [], c
    qi, qj, ri, rj, rv = int(qpos[i]), int(qpos[p]), int(rpos[i]), int(rpos[p]), int(rev[i]) & 1
    if max(qi, qj, ri, rj) >= 2 ** 31:
        return [], c
    dq, dr = qi - qj, (rj - ri if rv else ri - rj)
    lo, hi = (ri + k - ref_base, rj + k - ref_base) if rv else (rj - ref_base, ri - ref_base)
    if dq < 1 or dr < 1 or qi + k > len(qc) or not (0 <= lo <= len(rc) and 0 <= hi <= len(rc)):
        return [], c
    e = int(link[i])
    if abs(dq - dr) > DMAX or not 0 <= e <= DMAX or dq >= 2 ** 28 or dr >= 2 ** 28:
        return [], c
    if e == 0:
        return ([(OP_EQ, dq)] if dq == dr else []), c
    got = canonical([int(x) for x in qc[qj:qi]], _oriented(rc[lo:hi], rv), e)
    return (got[1] if got else []), c


def _codes(t):
    return _CODE[np.frombuffer(bytes(t), dtype=np.uint8)] if isinstance(t, (bytes, bytearray)) else _CODE[np.asarray(t, dtype=np.uint8)]


def chain_cigars_model(qtext, rtext, qpos, rpos, rev, pred, chain, n_chains, k, link, ref_base=0):
    """-> (offsets uint64[m + 1], ops uint32[total], ins uint32[n_chains], dels uint32[n_chains])"""
    qc, rc = _codes(qtext), _codes(rtext)
    m = len(qpos)
    offsets, ops = np.zeros(m + 1, dtype=np.uint64), []
    ins, dels = np.zeros(n_chains, dtype=np.uint32), np.zeros(n_chains, dtype=np.uint32)
    for i in range(m):
        runs, c = row_model(qc, rc, ref_base, qpos, rpos, rev, pred, chain, n_chains, k, link, i)
        for op, n in runs:
            ops.append((n << 4) | op)
            if op == OP_I:
                ins[c] += n
            elif op == OP_D:
                dels[c] += n
        offsets[i + 1] = len(ops)
    return offsets, np.array(ops, dtype=np.uint32), ins, dels


def text(runs):
    return "".join("%d%s" % (n, LETTER[op]) for op, n in runs)


def parse(s):
    import re
    assert re.fullmatch(r"(\d+[ID=X])*", s), s
    back = {v: k for k, v in LETTER.items()}
    return [(back[o], int(n)) for n, o in re.findall(r"(\d+)([ID=X])", s)]
