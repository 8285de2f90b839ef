"""TEST HELPER (not collected): hand-made inputs of kh_chain_records.  The call reads no text, so a case is made of rows alone: per chain a
number of members, the runs of its link rows, of its head and tail, and its two clips; the positions are laid out so that they agree with
the rows (a link row moves the query by its '=', X and I bases and the reference by its '=', X and D bases, downwards on the reverse
strand) -- until a `broken` case rewrites an array.  cases() -> {name: Case}."""
import numpy as np

import records_model as RM

K = 15
EQ, X, I, D = RM.OP_EQ, RM.OP_X, RM.OP_I, RM.OP_D
FIELDS = "qpos rpos rev chain lk_offsets lk_ops first last q_lo q_hi e_q e_r e_clip en_offsets en_ops".split()


def qlen_of(runs):
    return sum(n for o, n in runs if o in (EQ, X, I))


def rlen_of(runs):
    return sum(n for o, n in runs if o in (EQ, X, D))


class Case:
    """arrays: the inputs in the order of FIELDS; consistent: positions and rows agree, so the identities of a valid row hold"""

    def __init__(self, arrays, k=K, consistent=True):
        self.a, self.k, self.consistent = arrays, k, consistent

    def args(self):
        return [self.a[f] for f in FIELDS]

    def model(self, ref_order):
        return RM.records(*self.args(), self.k, ref_order)


def chain(n, link=lambda j: [(EQ, 20)], head=(), tail=(), clip=(0, 0), rev=0):
    return dict(n=n, link=link, head=list(head), tail=list(tail), clip=clip, rev=rev)


def build(specs, order=None, k=K, stray=0):
    """order: the chain of every anchor in anchor order (default: chain after chain); stray: anchors of no chain put between them"""
    if order is None:
        order = [c for c, s in enumerate(specs) for _ in range(s["n"])]
    if stray:
        order = [x for c in order for x in ([c] + [-1] * stray)]
    qpos, rpos, rev, chn, lk_off, lk_ops = [], [], [], [], [0], []
    seen = [0] * len(specs)
    at = {}                                              # chain -> (q, r) of its latest member
    first, last = [0] * len(specs), [0] * len(specs)
    q_cursor = 7
    q_lo, q_hi = [0] * len(specs), [0] * len(specs)
    for i, c in enumerate(order):
        if c < 0:
            qpos.append(0); rpos.append(0); rev.append(0); chn.append(-1); lk_off.append(len(lk_ops))
            continue
        s, j = specs[c], seen[c]
        if j == 0:
            q_lo[c] = q_cursor
            q = q_cursor + s["clip"][0] + qlen_of(s["head"])
            r = 1000000 * (c + 1)
            total = sum(qlen_of(s["link"](x)) for x in range(1, s["n"]))
            q_hi[c] = q + total + k + qlen_of(s["tail"]) + s["clip"][1]
            q_cursor = q_hi[c] + 3
            first[c] = i
            runs = []
        else:
            runs = s["link"](j)
            q, r = at[c]
            q, r = q + qlen_of(runs), (r - rlen_of(runs) if s["rev"] else r + rlen_of(runs))
        at[c] = (q, r)
        last[c] = i
        seen[c] += 1
        qpos.append(q); rpos.append(r); rev.append(s["rev"]); chn.append(c)
        lk_ops += [(n << 4) | o for o, n in runs]
        lk_off.append(len(lk_ops))
    e_q, e_r, e_clip, en_off, en_ops = [], [], [], [0], []
    for s in specs:
        for runs, cl in ((s["head"], s["clip"][0]), (s["tail"], s["clip"][1])):
            e_q.append(qlen_of(runs)); e_r.append(rlen_of(runs)); e_clip.append(cl)
            en_ops += [(n << 4) | o for o, n in runs]
            en_off.append(len(en_ops))
    u32 = lambda x: np.array(x, dtype=np.uint32)      # noqa: E731
    vals = [u32(qpos), u32(rpos), np.array(rev, dtype=np.uint8), np.array(chn, dtype=np.int32), np.array(lk_off, dtype=np.uint64), u32(lk_ops), u32(first), u32(last),
            u32(q_lo), u32(q_hi), u32(e_q), u32(e_r), u32(e_clip), np.array(en_off, dtype=np.uint64), u32(en_ops)]
    return Case(dict(zip(FIELDS, vals)), k)


def round_robin(sizes):
    left, order = list(sizes), []
    while any(left):
        for c, n in enumerate(left):
            if n:
                order.append(c)
                left[c] -= 1
    return order


def broken(case, **changes):
    a = {f: v.copy() for f, v in case.a.items()}
    for f, fn in changes.items():
        fn(a[f])
    return Case(a, case.k, consistent=False)


def _set(i, v):
    def fn(arr):
        arr[i] = v
    return fn


def cases():
    out = {}
    mixed = lambda j: [[(EQ, 12), (X, 1), (EQ, 7)], [(EQ, 9), (I, 2), (EQ, 4)], [(D, 3), (EQ, 11)], [(EQ, 30)], [(X, 2)]][j % 5]      # noqa: E731
    alt = lambda j: [(EQ, 5)] if j & 1 else [(X, 1)]                                                                                     # noqa: E731
    for n in (1, 2, 63, 64, 65, 129, 200):
        out["members_%d_mixed" % n] = build([chain(n, mixed, head=[(EQ, 4), (X, 1), (EQ, 3)], tail=[(EQ, 6), (I, 1), (EQ, 2)], clip=(2, 5))])
        out["members_%d_cascade" % n] = build([chain(n, head=[(EQ, 9)], tail=[(EQ, 8)])])                  # every piece is one '=' run: one run in all
        out["members_%d_alternating" % n] = build([chain(n, alt, head=[(X, 1)] if n > 1 else [(D, 1)], tail=[(X, 2)])])       # nothing merges
    sizes = [70, 3, 131]
    three = [chain(sizes[0], mixed, clip=(1, 0)), chain(sizes[1], rev=1, tail=[(EQ, 5)]), chain(sizes[2], alt, head=[(EQ, 2)], rev=1, clip=(0, 4))]
    out["two_interleaved"] = build(three[:2], round_robin(sizes[:2]))
    out["three_interleaved"] = build(three, round_robin(sizes))
    out["three_interleaved_strays"] = build(three, round_robin(sizes), stray=2)
    out["head_and_tail_merge"] = build([chain(3, lambda j: [(X, 2), (EQ, 10), (I, 1)], head=[(EQ, 5), (X, 3)], tail=[(EQ, 4), (X, 1)])])      # X + X at the head; k '=' + '=' at the tail
    out["tail_merges_clip_not"] = build([chain(2, tail=[(EQ, 3), (I, 2)], clip=(0, 6)), chain(1, head=[(I, 1)], clip=(3, 0))])
    out["empty_ends_no_clip"] = build([chain(4, mixed), chain(1)])
    out["empty_ends_clip"] = build([chain(4, mixed, clip=(11, 13)), chain(1, clip=(1, 1), rev=1)])
    out["zero_runs_inside"] = build([chain(3, lambda j: [(EQ, 4), (X, 0), (EQ, 5), (I, 0)], head=[(EQ, 0)], tail=[(X, 0), (EQ, 2)])])
    out["one_empty_link_row"] = build([chain(5, lambda j: [] if j == 3 else [(EQ, 20)], head=[(EQ, 2)]), chain(2)])
    out["reverse_chains"] = build([chain(66, mixed, head=[(EQ, 3)], tail=[(X, 1), (EQ, 9)], clip=(4, 0), rev=1), chain(2, alt, rev=1, clip=(0, 2)), chain(3, mixed)])
    base = build([chain(6, mixed, head=[(EQ, 4)], tail=[(EQ, 6)], clip=(2, 5)), chain(3, alt, rev=1), chain(70)], round_robin([6, 3, 70]))
    m = len(base.a["qpos"])
    out["last_beyond_m"] = broken(base, last=_set(0, m))
    out["last_far_beyond_m"] = broken(base, last=_set(2, 0xFFFFFFFF))
    out["first_after_last"] = broken(base, first=_set(1, m - 1))
    out["chain_of_first_is_another"] = broken(base, chain=_set(int(base.a["first"][0]), 1))
    out["chain_numbers_garbage"] = broken(base, chain=lambda a: a.__setitem__(slice(5, 9), [-7, 2 ** 31 - 1, 0, -2 ** 31]))
    out["read_too_short"] = broken(base, q_hi=_set(0, int(base.a["qpos"][int(base.a["last"][0])]) + K - 1))
    out["seed_before_read"] = broken(base, q_lo=_set(2, int(base.a["qpos"][int(base.a["first"][2])]) + 1))
    out["read_of_2_28"] = broken(base, q_hi=_set(1, int(base.a["q_lo"][1]) + 2 ** 28))
    out["link_offsets_descend"] = broken(base, lk_offsets=lambda a: a.__setitem__(slice(10, 14), a[10:14][::-1].copy()))
    out["link_offsets_beyond"] = broken(base, lk_offsets=lambda a: a.__setitem__(slice(20, None), a[20:] + np.uint64(10 ** 12)))
    out["link_rows_63_and_64"] = build([chain(2, lambda j: [(EQ, 1), (X, 1)] * 31 + [(EQ, 1)]), chain(2, lambda j: [(EQ, 1), (X, 1)] * 32)])      # (more than 63 runs: an empty row)
    out["end_offsets_descend"] = broken(base, en_offsets=lambda a: a.__setitem__(slice(1, 3), a[1:3][::-1].copy()))
    out["end_offsets_beyond"] = broken(base, en_offsets=lambda a: a.__setitem__(slice(3, None), np.uint64(2 ** 63)))
    out["clip_of_2_31"] = broken(base, e_clip=_set(0, 2 ** 31 + 9))
    out["ops_garbage"] = broken(base, lk_ops=lambda a: a.__setitem__(slice(0, 12), np.arange(12, dtype=np.uint32) * np.uint32(0x1F3D5B79)))
    empty = build([chain(1), chain(1, clip=(2, 2))])
    out["no_anchors_with_chains"] = Case({f: (v[:0] if f in ("qpos", "rpos", "rev", "chain", "lk_ops") else v[:1] if f == "lk_offsets" else v) for f, v in empty.a.items()},
                                         consistent=False)
    out["no_chains"] = Case({f: (v[:0] if f in FIELDS[6:13] + ["en_ops"] else v[:1] if f == "en_offsets" else v) for f, v in base.a.items()}, consistent=False)
    return out
