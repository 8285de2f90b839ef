"""TEST HELPER (not collected): named inputs of kh_pair_chains, the hand-written outputs of the small ones, a random table and the planted
fragments the model must recover.  A chain is (rs, re, rev, score, tid, use, mapq_in); a case is a list of pairs (mate 1's chains, mate 2's
chains) and the parameters."""
import numpy as np

NONE = 0xFFFFFFFF
TOP, BOT = 2 ** 31 - 1, -2 ** 31
U32 = 2 ** 32 - 1


def c(rs, re, rev, score, tid=0, use=1, mq=0):
    return (rs, re, rev, score, tid, use, mq)


F, R = c(1000, 1100, 0, 90), c(1300, 1400, 1, 80)      # a forward and a reverse chain 400 bases apart: the plain proper pair


def build(pairs, with_tid=True, with_use=True, with_mapq=True, **params):
    """-> the keyword arguments of pair_model / kmers.pair_chains"""
    rows, offs = [], [0]
    for m1, m2 in pairs:
        for m in (m1, m2):
            rows += list(m)
            offs.append(len(rows))
    col = lambda i, dt: np.array([r[i] for r in rows], dtype=np.int64).astype(dt)      # noqa: E731
    return dict(rs=col(0, np.uint32), re=col(1, np.uint32), rev=col(2, np.uint8), score=col(3, np.int32), read_offsets=np.array(offs, dtype=np.uint64),
                tid=col(4, np.uint32) if with_tid else None, use=col(5, np.uint8) if with_use else None, mapq=col(6, np.uint8) if with_mapq else None,
                **{**dict(min_ins=0, max_ins=1000, unpaired_pen=17), **params})


def cut(n, partner_rank):
    """mate 1 has n candidates: n - 63 of score 50 first, then 63 of score 100 -- the 64th place is taken by the first 50 in chain order,
    a tie across the cut.  All but one are decoys far downstream; the one chain concordant with mate 2 is the first 50 (ranked 64th: in)
    or the second (ranked 65th: out)."""
    decoy = lambda i, s: c(100000 + 1000 * i, 100100 + 1000 * i, 0, s)      # noqa: E731
    m1 = [decoy(i, 50) for i in range(n - 63)] + [decoy(i, 100) for i in range(n - 63, n)]
    m1[partner_rank - 64] = c(1000, 1100, 0, 50)
    return build([(m1, [R])], unpaired_pen=50)


CASES = {
    "no_chains_pair": build([([], []), ([F], [R])]),
    "one_mate_empty": build([([c(1000, 1100, 0, 90, mq=33)], [])]),
    "use_all_zero": build([([c(1000, 1100, 0, 90, use=0)], [c(1300, 1400, 1, 80, use=0)])]),
    "cut_64_rank64": cut(64, 64),
    "cut_65_rank64": cut(65, 64),
    "cut_65_rank65": cut(65, 65),
    "cut_130_rank64": cut(130, 64),
    "cut_130_rank65": cut(130, 65),
    "same_strand": build([([c(1000, 1100, 0, 90, mq=11)], [c(1300, 1400, 0, 80, mq=22)])]),
    "reverse_forward": build([([c(1300, 1400, 0, 90)], [c(1000, 1100, 1, 80)])]),
    "re_f_gt_re_r": build([([c(1000, 1500, 0, 90)], [c(1200, 1400, 1, 80)])]),
    "frag_bounds": build([([F], [c(1200, 1300, 1, 80)]), ([F], [R]), ([F], [c(1301, 1401, 1, 80)])], min_ins=300, max_ins=400),
    "different_tid": build([([F], [c(1300, 1400, 1, 80, tid=1)])]),
    "tid_none": build([([c(1000, 1100, 0, 90, tid=NONE)], [c(1300, 1400, 1, 80, tid=NONE)])]),
    "tid_null": build([([F], [c(1300, 1400, 1, 80, tid=5)])], with_tid=False),
    "all_null": build([([F], [R])], with_tid=False, with_use=False, with_mapq=False),
    "ps_ties": build([([c(1000, 1100, 0, 50), c(1010, 1110, 0, 50)], [c(1300, 1400, 1, 50), c(1310, 1410, 1, 50)])]),
    "ps_ties_chain_order": build([([c(1000, 1100, 0, 40), c(5000, 5100, 0, 60, tid=1)], [c(1300, 1400, 1, 60), c(5300, 5400, 1, 40, tid=1)])], unpaired_pen=20),
    "pen_equal": build([([c(1000, 1100, 0, 50), c(9000, 9100, 0, 70)], [R])], unpaired_pen=20),
    "pen_below": build([([c(1000, 1100, 0, 50), c(9000, 9100, 0, 70)], [R])], unpaired_pen=19),
    "negative_scores": build([([c(1000, 1100, 0, -5)], [c(1300, 1400, 1, 30)])]),
    "ps_nonpositive": build([([c(1000, 1100, 0, -50, mq=7)], [c(1300, 1400, 1, 30, mq=9)])]),
    "big_scores": build([([c(1000, 1100, 0, TOP), c(1010, 1110, 0, TOP - 1)], [c(1300, 1400, 1, TOP)]), ([c(1000, 1100, 0, BOT)], [c(1300, 1400, 1, BOT)])]),
    "equal_rs": build([([c(1000, 1200, 1, 80)], [c(1000, 1100, 0, 90)])]),
    "re_max": build([([c(U32 - 1295, U32 - 1195, 0, 90)], [c(U32 - 100, U32, 1, 80)]), ([c(0, 100, 0, 50)], [c(U32 - 100, U32, 1, 50)])], max_ins=2000),
    "re_le_rs": build([([c(1000, 1000, 0, 99), c(1000, 1100, 0, 50)], [R, c(1500, 1400, 1, 99)])]),
}

# name -> (row, mapq, tlen, flag, score, nconc), written by hand from the definition
EXPECT = {
    "no_chains_pair": ([-1, -1, 0, 1], [0, 0, 60, 60], [0, 0, 400, -400], [0, 7], [0, 170], [0, 1]),
    "one_mate_empty": ([0, -1], [33, 0], [0, 0], [0], [0], [0]),
    "use_all_zero": ([-1, -1], [0, 0], [0, 0], [0], [0], [0]),
    "same_strand": ([0, 1], [11, 22], [400, -400], [6], [0], [0]),
    "reverse_forward": ([0, 1], [0, 0], [-400, 400], [6], [0], [0]),
    "re_f_gt_re_r": ([0, 1], [0, 0], [500, -500], [6], [0], [0]),
    "frag_bounds": ([0, 1, 2, 3, 4, 5], [60, 60, 60, 60, 0, 0], [300, -300, 400, -400, 401, -401], [7, 7, 6], [170, 170, 0], [1, 1, 0]),
    "different_tid": ([0, 1], [0, 0], [0, 0], [2], [0], [0]),
    "tid_none": ([0, 1], [0, 0], [0, 0], [2], [0], [0]),
    "tid_null": ([0, 1], [60, 60], [400, -400], [7], [170], [1]),
    "all_null": ([0, 1], [60, 60], [400, -400], [7], [170], [1]),
    "ps_ties": ([0, 2], [0, 0], [400, -400], [7], [100], [4]),
    "ps_ties_chain_order": ([0, 2], [0, 0], [400, -400], [7], [100], [2]),
    "pen_equal": ([0, 2], [60, 60], [400, -400], [7], [130], [1]),
    "pen_below": ([1, 2], [0, 0], [-7800, 7800], [6], [130], [1]),
    "negative_scores": ([0, 1], [60, 60], [400, -400], [7], [25], [1]),
    "ps_nonpositive": ([0, 1], [7, 9], [400, -400], [7], [-20], [1]),
    "big_scores": ([0, 2, 3, 4], [0, 60, 0, 0], [400, -400, 400, -400], [7, 7], [TOP, BOT], [2, 1]),
    "equal_rs": ([0, 1], [60, 60], [200, -200], [7], [170], [1]),
    "re_max": ([0, 1, 2, 3], [60, 60, 0, 0], [1295, -1295, TOP, -TOP], [7, 6], [170, 0], [1, 0]),
    "re_le_rs": ([1, 2], [60, 60], [400, -400], [7], [130], [1]),
    "cut_64_rank64": ([0, 64], [60, 60], [400, -400], [7], [130], [1]),
    "cut_65_rank64": ([0, 65], [60, 60], [400, -400], [7], [130], [1]),
    "cut_65_rank65": ([2, 65], [0, 0], [-100800, 100800], [6], [0], [0]),
    "cut_130_rank64": ([0, 130], [60, 60], [400, -400], [7], [130], [1]),
    "cut_130_rank65": ([67, 130], [0, 0], [-165800, 165800], [6], [0], [0]),
}

RANDOM_SIZES = (0, 1, 2, 5, 63, 64, 65, 200)


def random_table(n_pairs=2000, seed=5):
    """group sizes drawn from RANDOM_SIZES, chains within a few kilobases of each other on three targets and none, few distinct scores
    (many ties), some chains switched off, some with re <= rs"""
    rng = np.random.default_rng(seed)
    sizes = rng.choice(RANDOM_SIZES, size=2 * n_pairs, p=[0.1, 0.25, 0.25, 0.2, 0.03, 0.03, 0.04, 0.1])
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(offs[-1])
    rs = rng.integers(0, 3000, size=n).astype(np.uint32)
    ln = rng.integers(-20, 200, size=n)
    re = np.maximum(rs.astype(np.int64) + ln, 0).astype(np.uint32)
    tid = rng.choice(np.array([0, 1, 2, NONE], dtype=np.uint32), size=n, p=[0.5, 0.3, 0.15, 0.05])
    return dict(rs=rs, re=re, rev=rng.integers(0, 4, size=n).astype(np.uint8), score=rng.integers(-3, 12, size=n).astype(np.int32), read_offsets=offs, tid=tid,
                use=(rng.random(n) < 0.9).astype(np.uint8) * rng.integers(1, 255, size=n).astype(np.uint8), mapq=rng.integers(0, 61, size=n).astype(np.uint8),
                min_ins=100, max_ins=2500, unpaired_pen=3)


def planted_table(n_pairs=200, seed=11, genome=50_000):
    """fragments over a genome that holds an exact duplicate: per pair the two true rows (forward mate at the fragment's start, reverse
    mate at its end, score 100) planted at random places among decoy rows of lower score elsewhere; every tenth fragment lies in the
    duplicate, so both mates have a second true-looking row one copy further.  -> (arguments, truth): truth[p] = (row of mate 1, row of
    mate 2, fragment length, in the duplicate?)"""
    rng = np.random.default_rng(seed)
    dup_a, dup_b, dup_len = 10_000, 30_000, 1500
    pairs, truth, base = [], [], 0
    for p in range(n_pairs):
        frag = int(rng.integers(300, 501))
        in_dup = p % 10 == 0
        start = int(dup_a + rng.integers(0, dup_len - frag)) if in_dup else int(rng.integers(0, dup_a - frag))
        flip = bool(rng.integers(0, 2))      # which mate is the forward one
        fwd, rv = c(start, start + 100, 0, 100, mq=0 if in_dup else 60), c(start + frag - 100, start + frag, 1, 100, mq=0 if in_dup else 60)
        mates = []
        for true in ((rv, fwd) if flip else (fwd, rv)):
            rows = [true]
            if in_dup:      # the other copy
                rows.append(c(true[0] + dup_b - dup_a, true[1] + dup_b - dup_a, true[2], 100))
            for _ in range(int(rng.integers(0, 6))):
                at = int(rng.integers(0, genome - 100))
                rows.append(c(at, at + 100, int(rng.integers(0, 2)), int(rng.integers(40, 90))))
            order = rng.permutation(len(rows))
            mates.append([rows[i] for i in order])
            truth.append(base + int(np.flatnonzero(order == 0)[0]))
            base += len(rows)
        pairs.append(tuple(mates))
        truth[-2:] = [(truth[-2], truth[-1], frag, in_dup, flip)]
    return build(pairs, min_ins=200, max_ins=600), truth
