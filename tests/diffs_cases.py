"""TEST HELPER (not collected): inputs of kh_record_diffs.  A batch is a dict of the call's arrays (qtext, rtext, ref_base, offsets, ops,
valid, rev, q_lo, q_hi, rs).  cases() holds the hand-made rows -- every run count around the wave steps, the MD number carried across a
step and an insertion, edits at the ends and side by side, every digit count, rows that must be refused -- over random texts (the kernel
and the model do not care whether '=' really matches); planted() makes alignments that are true, for the checks that rebuild the
reference from a difference string."""
import random

import numpy as np

I, D, S, EQ, X, M = 1, 2, 4, 7, 8, 0
ALPHABET = b"ACGTACGTACGTacgtNn-*"


def run(op, l):
    return (l << 4) | op


class Batch:
    def __init__(self, seed, ref_base=0, nr=4000, alphabet=ALPHABET):
        self.rng = random.Random(seed)
        self.ref_base, self.alphabet = ref_base, alphabet
        self.rtext = bytes(self.rng.choice(alphabet) for _ in range(nr))
        self.q = bytearray(self._bases(3))          # (no read starts at byte 0)
        self.rows = []                              # (runs, valid, rev, lo, hi, rs)

    def _bases(self, n):
        return bytes(self.rng.choice(self.alphabet) for _ in range(n))

    def row(self, runs, rev=0, valid=1, dL=0, rs=None, pad=2, L=None):
        """a row of (op, length) runs over a fresh read of the length the runs consume + dL (or of length L) and a random reference start
        that fits (where anything fits)"""
        qlen = sum(l for o, l in runs if o in (S, EQ, X, I, M)) if L is None else L
        rlen = min(sum(l for o, l in runs if o in (EQ, X, D, M)), len(self.rtext))
        lo = len(self.q)
        self.q += self._bases(max(qlen + dL, 0) + pad)
        if rs is None:
            rs = self.ref_base + self.rng.randrange(0, len(self.rtext) - rlen + 1)
        self.rows.append(([run(o, l) for o, l in runs], valid, rev, lo, lo + max(qlen + dL, 0), rs))
        return self

    def arrays(self):
        offs, ops = [0], []
        for r in self.rows:
            ops += r[0]
            offs.append(len(ops))
        col = lambda i, dt: np.array([r[i] for r in self.rows], dtype=dt)      # noqa: E731
        return {"qtext": np.frombuffer(bytes(self.q), dtype=np.uint8).copy(), "rtext": np.frombuffer(self.rtext, dtype=np.uint8).copy(), "ref_base": self.ref_base,
                "offsets": np.array(offs, dtype=np.uint64), "ops": np.array(ops, dtype=np.uint32), "valid": col(1, np.uint8), "rev": col(2, np.uint8),
                "q_lo": col(3, np.uint32), "q_hi": col(4, np.uint32), "rs": col(5, np.uint32)}


def alternating(n):
    """n runs, no two neighbours alike: '=' between X, I and D in turn"""
    edits = [(X, 1), (I, 2), (D, 3), (X, 2), (D, 1), (I, 1)]
    return [(EQ, 1 + i % 7) if i % 2 == 0 else edits[(i // 2) % len(edits)] for i in range(n)]


def hand(rev):
    b = Batch(5 + rev, ref_base=1000, nr=6000)
    for n in (0, 1, 63, 64, 65, 128, 129):                       # around the wave steps (a row of 0 runs is not good)
        b.row(alternating(n), rev)
    # '=' at run 63, I at run 64, '=' at run 65, then X: the MD number crosses a wave step and an insertion
    b.row([(X, 1) if i % 2 else (EQ, 2) for i in range(63)] + [(EQ, 5), (I, 3), (EQ, 7), (X, 1), (EQ, 4)], rev)
    b.row([(X, 1), (EQ, 10)], rev)                               # starts with X
    b.row([(D, 2), (EQ, 10)], rev)                               # starts with D
    b.row([(EQ, 10), (X, 1)], rev)                               # ends with X
    b.row([(EQ, 5), (X, 1), (D, 3), (X, 2), (EQ, 5)], rev)       # X next to D next to X
    b.row([(EQ, 3), (X, 1), (EQ, 3), (X, 40), (EQ, 3)], rev)     # X runs of 1 and of 40
    for n in (9, 10, 99, 100):                                   # digit counts of an MD number and of a cs match
        b.row([(S, 2), (EQ, n), (X, 1), (EQ, n), (D, 1), (EQ, 1), (S, 1)], rev)
    b.row([(EQ, 4), (X, 0), (M, 0), (EQ, 5), (I, 0), (X, 1), (EQ, 2)], rev)      # runs of length 0, whatever their op, vanish
    b.row([(S, 5)], rev)                                         # clips alone: cs is empty and ok, MD is "0"
    b.row([(I, 4)], rev)
    b.row(alternating(9), rev, valid=0)                          # valid = 0
    b.row([(EQ, 4), (M, 3), (EQ, 4)], rev)                       # an M run spoils the row
    b.row([(EQ, 4), (3, 2), (EQ, 4)], rev)                       # so does N
    b.row(alternating(7), rev, dL=1)                             # j != L by one
    b.row(alternating(7), rev, dL=-1)
    b.row([(EQ, 8), (X, 1), (EQ, 8)], rev, rs=999)               # leaves the reference text by one below
    b.row([(EQ, 8), (X, 1), (EQ, 8)], rev, rs=1000 + 6000 - 16)  # ... and above
    b.row([(EQ, 8), (X, 1), (EQ, 8)], rev, rs=1000 + 6000 - 17)  # the last base of the text: good
    b.row([(EQ, 8), (X, 1), (EQ, 8)], rev, rs=1000)              # the first one: good
    b.row([(I, 3), (EQ, 8), (D, 8)], rev, rs=999 + 6000 - 15)    # a deletion that ends with the text
    b.row([(EQ, 6), (X, 2)], rev, pad=0)                         # the last read: ends with the text
    a = b.arrays()
    a["q_hi"][-1] = len(a["qtext"])
    return a


def q_beyond():
    """q_hi one beyond nq; q_lo > q_hi"""
    b = Batch(9)
    b.row([(EQ, 6), (X, 2)], pad=0).row([(EQ, 6), (X, 2)], pad=0)
    a = b.arrays()
    a["q_hi"][1] = len(a["qtext"]) + 1
    a["q_lo"][1] += 1
    a["q_lo"][0], a["q_hi"][0] = a["q_hi"][0], a["q_lo"][0]
    return a


def bad_offsets():
    """offsets that descend, and offsets beyond n_ops: clamped, empty rows are not good"""
    b = Batch(11)
    for n in (3, 5, 7, 9, 4):
        b.row(alternating(n), n & 1)
    a = b.arrays()
    a["offsets"] = np.array([0, 3, 8, 5, 2 ** 40, 2 ** 63], dtype=np.uint64)      # row 2 descends, row 3 is clamped to the end, row 4 is empty
    return a


def million():
    """a match of 10^6 bases: seven digits in cs and MD"""
    b = Batch(13, ref_base=7, nr=1_000_100, alphabet=b"ACGT")
    b.row([(X, 1), (EQ, 1_000_000), (X, 1)], 0, rs=7 + 50).row([(X, 1), (EQ, 1_000_000), (D, 2)], 1, rs=7 + 90)
    return b.arrays()


def garbage(seed, n_rows=200):
    """random rows: random run words (any op, lengths 0..40, now and then huge), intervals and starts that fit or do not"""
    rng = random.Random(seed)
    b = Batch(seed, ref_base=rng.choice([0, 333]), nr=3000)
    for _ in range(n_rows):
        runs = [(rng.choice([EQ, EQ, EQ, X, I, D, S, rng.randrange(16)]), rng.choice([0, 1, 1, 2, 3, 9, 10, 40, rng.randrange(1 << 28)])) for _ in range(rng.randrange(0, 9))]
        if rng.random() < 0.7:      # mostly rows that can be good
            runs = [(o if o in (EQ, X, I, D, S) else EQ, l % 50) for o, l in runs]
        qlen = sum(l for o, l in runs if o in (S, EQ, X, I, M))
        b.row(runs, rng.randrange(4), rng.choice([1, 1, 1, 0, 255]), rng.choice([0, 0, 0, 1, -1]), None if rng.random() < 0.8 else rng.randrange(0, 4000),
              L=None if qlen <= 2000 else rng.randrange(0, 300))
    return b.arrays()


def planted(seed, n_rows=200, max_len=300):
    """true alignments over A, C, G, T: the reference-oriented read is made from the reference run by run (X bases differ, '=' bases are
    equal), reverse-strand reads are stored reverse-complemented -> (batch, the reference span [rs, re) per row)"""
    rng = random.Random(seed)
    ref_base, nr = rng.choice([0, 17]), 5000
    rtext = bytes(rng.choice(b"ACGT") for _ in range(nr))
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    q, rows, spans = bytearray(b"NN"), [], []
    for _ in range(n_rows):
        rs = rng.randrange(0, nr - max_len - 100)
        r, o, runs = rs, bytearray(), []
        if rng.random() < 0.3:
            l = rng.randrange(1, 9); runs.append((S, l)); o += bytes(rng.choice(b"ACGT") for _ in range(l))
        last = None
        for t in range(rng.randrange(1, 12)):
            op = rng.choice([EQ, EQ, X, I, D]) if t else rng.choice([EQ, X, D, I])
            if op == last:
                op = EQ if op != EQ else X
            l = rng.randrange(1, 30) if op == EQ else rng.randrange(1, 4)
            if op == EQ:
                o += rtext[r:r + l]; r += l
            elif op == X:
                o += bytes(rng.choice([c for c in b"ACGT" if c != x]) for x in rtext[r:r + l]); r += l
            elif op == I:
                o += bytes(rng.choice(b"ACGT") for _ in range(l))
            else:
                r += l
            runs.append((op, l)); last = op
        if rng.random() < 0.3:
            l = rng.randrange(1, 9); runs.append((S, l)); o += bytes(rng.choice(b"ACGT") for _ in range(l))
        rev = rng.randrange(2)
        lo = len(q)
        q += (bytes(o).translate(comp)[::-1] if rev else bytes(o)) + b"\n"
        rows.append(([run(a, b) for a, b in runs], 1, rev, lo, lo + len(o), ref_base + rs))
        spans.append((ref_base + rs, ref_base + r))
    b = Batch.__new__(Batch)
    b.ref_base, b.rtext, b.q, b.rows = ref_base, rtext, q, rows
    return b.arrays(), spans


def cases():
    out = {"hand_fwd": hand(0), "hand_rev": hand(1), "q_beyond": q_beyond(), "bad_offsets": bad_offsets(), "million": million(), "garbage_1": garbage(1), "garbage_2": garbage(2)}
    out["planted"] = planted(3)[0]
    return out
