"""TEST HELPER (not collected): kh_chain_records and kh_cigar_text on Python integers and lists -- the definition of
include/kmerhash_amd.h restated, the yardstick of the kernels.  Everything is u32 / u64 arithmetic written out with masks."""
M32 = 0xFFFFFFFF
LEN_MASK = (1 << 28) - 1
OP_I, OP_D, OP_S, OP_EQ, OP_X = 1, 2, 4, 7, 8
ROW_MAX = 63
TEXT_OPS = "MIDNSHP=X"


def row(offsets, ops, i):
    """row i of a CSR: bounds clamped to the number of runs; empty where they descend or hold more than ROW_MAX runs"""
    n = len(ops)
    a, b = min(int(offsets[i]), n), min(int(offsets[i + 1]), n)
    return [int(v) for v in ops[a:b]] if a < b <= a + ROW_MAX else []


def feed(out, op, length):
    """the rule of a row: a zero run vanishes, a run of the op before it adds to it (mod 2^28), another starts a new run"""
    if not length:
        return
    if out and out[-1][0] == op:
        out[-1][1] = (out[-1][1] + length) & LEN_MASK
    else:
        out.append([op, length])


def records(qpos, rpos, rev, chain, lk_offsets, lk_ops, first, last, q_lo, q_hi, e_q, e_r, e_clip, en_offsets, en_ops, k, ref_order=0):
    """-> dict of lists: valid, qs, qe, rs, re, qlen, n_match, n_block, nm, offsets, ops"""
    m, nc = len(qpos), len(first)
    out = {key: [] for key in "valid qs qe rs re qlen n_match n_block nm".split()}
    out["offsets"], out["ops"] = [0], []
    for c in range(nc):
        f, l, lo, hi = int(first[c]), int(last[c]), int(q_lo[c]), int(q_hi[c])
        level = 0
        if f <= l < m and int(chain[f]) == c and int(chain[l]) == c:
            level = 1
            if lo <= int(qpos[f]) and int(qpos[l]) + k <= hi and ((hi - lo) & M32) < (1 << 28):
                level = 2
        qs = qe = rs = re = 0
        if level:
            rv = int(rev[f]) & 1
            hq, tq, hr, tr = int(e_q[2 * c]), int(e_q[2 * c + 1]), int(e_r[2 * c]), int(e_r[2 * c + 1])
            qs, qe = (int(qpos[f]) - hq - lo) & M32, (int(qpos[l]) + k + tq - lo) & M32
            rf, rl = int(rpos[f]), int(rpos[l])
            rs, re = (min(rf, rl) - (tr if rv else hr)) & M32, (max(rf, rl) + k + (hr if rv else tr)) & M32
        runs, ok = [], level == 2
        if ok:
            feed(runs, OP_S, int(e_clip[2 * c]) & LEN_MASK)
            for v in row(en_offsets, en_ops, 2 * c):
                feed(runs, v & 15, v >> 4)
            for i in range(f + 1, l + 1):
                if int(chain[i]) != c:
                    continue
                piece = row(lk_offsets, lk_ops, i)
                if not piece:
                    ok = False
                    break
                for v in piece:
                    feed(runs, v & 15, v >> 4)
        if ok:
            feed(runs, OP_EQ, k)
            for v in row(en_offsets, en_ops, 2 * c + 1):
                feed(runs, v & 15, v >> 4)
            feed(runs, OP_S, int(e_clip[2 * c + 1]) & LEN_MASK)
        else:
            runs = []
        # the sums are those of the runs as they were fed (u32); merging mod 2^28 does not touch them
        fed = []
        if ok:
            fed = [(v & 15, v >> 4) for v in row(en_offsets, en_ops, 2 * c)] + [(v & 15, v >> 4) for i in range(f + 1, l + 1) if int(chain[i]) == c for v in row(lk_offsets, lk_ops, i)]
            fed += [(OP_EQ, k)] + [(v & 15, v >> 4) for v in row(en_offsets, en_ops, 2 * c + 1)]
        out["valid"].append(1 if ok else 0)
        for key, v in (("qs", qs), ("qe", qe), ("rs", rs), ("re", re), ("qlen", (hi - lo) & M32)):
            out[key].append(v)
        out["n_match"].append(sum(n for o, n in fed if o == OP_EQ) & M32)
        out["n_block"].append(sum(n for o, n in fed if o in (OP_EQ, OP_X, OP_I, OP_D)) & M32)
        out["nm"].append(sum(n for o, n in fed if o in (OP_X, OP_I, OP_D)) & M32)
        if ref_order and level and int(rev[f]) & 1:
            runs = runs[::-1]
        out["ops"] += [((n << 4) | o) & M32 for o, n in runs]
        out["offsets"].append(len(out["ops"]))
    return out


def run_text(v):
    return "%d%s" % (v >> 4, TEXT_OPS[v & 15] if (v & 15) < 9 else "?")


def cigar_text(offsets, ops):
    """-> (text offsets, text as bytes): the bounds clamped as kh_cigar_text clamps them"""
    n = len(ops)
    o = [min(int(x), n) for x in offsets]
    if not o:
        return [], b""
    base = o[0]
    b = [max(x, base) for x in o]
    size = [len(run_text(int(v))) for v in ops]
    pre = [0]
    for s in size:
        pre.append(pre[-1] + s)
    text = "".join(run_text(int(v)) for v in ops[base:b[-1]])
    return [pre[x] - pre[base] for x in b], text.encode("ascii")
