"""TEST HELPER (not collected): kh_record_diffs on Python integers -- the definition of include/kmerhash_amd.h as loops, the yardstick the
kernels must equal bit for bit (ok, offsets, text)."""
CS, MD = 0, 1
OP_I, OP_D, OP_S, OP_EQ, OP_X = 1, 2, 4, 7, 8


def code(b):
    """A/a 0, C/c 1, G/g 2, T/t 3, any other byte 4"""
    return {0x41: 0, 0x43: 1, 0x47: 2, 0x54: 3}.get(b & 0xdf, 4)


def oriented(qtext, lo, hi, rev):
    """the codes of the oriented read O of a row"""
    if not rev & 1:
        return [code(qtext[lo + j]) for j in range(hi - lo)]
    out = []
    for j in range(hi - lo):
        c = code(qtext[hi - 1 - j])
        out.append(3 - c if c < 4 else 4)
    return out


def row_text(qtext, rtext, ref_base, runs, valid, rev, lo, hi, rs, kind):
    """one row -> its text as bytes, or None where the row is not good.  runs: the (len << 4) | op words of the row"""
    nq, nr = len(qtext), len(rtext)
    if not valid or not runs or not lo <= hi <= nq:
        return None
    L = hi - lo
    O = oriented(qtext, lo, hi, rev)
    lower, upper = "acgtn", "ACGTN"
    j, r, n, out = 0, rs, 0, []

    def R(x):
        return code(rtext[x - ref_base])

    for v in runs:
        op, l = v & 15, v >> 4
        if l == 0:
            continue
        if op not in (OP_I, OP_D, OP_S, OP_EQ, OP_X):
            return None
        if op in (OP_S, OP_EQ, OP_X, OP_I) and j + l > L:
            return None
        if op in (OP_EQ, OP_X, OP_D) and (r < ref_base or r + l > ref_base + nr):
            return None
        if op == OP_S:
            j += l
        elif op == OP_EQ:
            if kind == CS:
                out.append(":%d" % l)
            else:
                n = (n + l) & 0xFFFFFFFF
            j += l; r += l
        elif op == OP_X:
            for t in range(l):
                if kind == CS:
                    out.append("*" + lower[R(r + t)] + lower[O[j + t]])
                else:
                    out.append("%d%s" % (n, upper[R(r + t)]))
                    n = 0
            j += l; r += l
        elif op == OP_I:
            if kind == CS:
                out.append("+" + "".join(lower[O[j + t]] for t in range(l)))
            j += l
        else:
            if kind == CS:
                out.append("-" + "".join(lower[R(r + t)] for t in range(l)))
            else:
                out.append("%d^%s" % (n, "".join(upper[R(r + t)] for t in range(l))))
                n = 0
            r += l
    if j != L:
        return None
    if kind == MD:
        out.append("%d" % n)
    text = "".join(out).encode("ascii")
    return text if len(text) < 2 ** 32 else None


def record_diffs(qtext, rtext, ref_base, offsets, ops, valid, rev, q_lo, q_hi, rs, kind):
    """-> dict(ok, offsets, text): lists of integers and the text as bytes"""
    n_ops, ok, offs, parts = len(ops), [], [0], []
    for c in range(len(valid)):
        a, b = min(int(offsets[c]), n_ops), min(int(offsets[c + 1]), n_ops)
        runs = [int(v) for v in ops[a:b]] if b > a else []
        t = row_text(qtext, rtext, int(ref_base), runs, int(valid[c]), int(rev[c]), int(q_lo[c]), int(q_hi[c]), int(rs[c]), kind)
        ok.append(0 if t is None else 1)
        parts.append(t or b"")
        offs.append(offs[-1] + len(parts[-1]))
    return {"ok": ok, "offsets": offs, "text": b"".join(parts)}
