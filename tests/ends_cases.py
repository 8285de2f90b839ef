"""TEST HELPER (not collected): hand-made chain ends for the tests of kh_chain_ends.  One reference of random bases; every read is cut
around ONE seed of k bases at a chosen reference position and strand, with a head and a tail of chosen lengths that equal the reference
(as far as it reaches: beyond its ends the read goes on with random bases) until `mutate` rewrites them.  Each read is one chain whose
first and last anchor are that seed, unless add() is given a second seed."""
import random

import numpy as np

K = 15
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def bases(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def revcomp(s):
    return s.translate(COMP)[::-1]


def sub(s, *at):
    s = bytearray(s)
    for p in at:
        s[p] = b"ACGT"[(b"ACGT".index(s[p]) + 1) % 4] if s[p] in b"ACGT" else ord("A")
    return bytes(s)


class Ends:
    def __init__(self, seed, ref_len=4000, ref_base=0):
        self.rng = random.Random(seed)
        self.ref = bytearray(bases(self.rng, ref_len))
        self.ref_base = ref_base
        self.reads, self.qpos, self.rpos, self.rev, self.first, self.last, self.q_lo, self.q_hi = [], [], [], [], [], [], [], []
        self.nq = 0

    def add(self, r, h, t, rev=0, head=None, tail=None, gap=0):
        """a read with its seed at reference offset r (into the text): h bases before it and t behind it in read order; head / tail:
        functions that rewrite the piece (given in read order); gap: bytes of another read's text put in front of it"""
        ref, rng = bytes(self.ref), self.rng
        seed = ref[r:r + K]
        if rev:
            hp = revcomp(ref[r + K:r + K + h])
            hp = bases(rng, h - len(hp)) + hp
            tp = revcomp(ref[max(0, r - t):r])
            tp = tp + bases(rng, t - len(tp))
            seed = revcomp(seed)
        else:
            hp = ref[max(0, r - h):r]
            hp = bases(rng, h - len(hp)) + hp
            tp = ref[r + K:r + K + t]
            tp = tp + bases(rng, t - len(tp))
        hp, tp = (head(hp) if head else hp), (tail(tp) if tail else tp)
        read = bases(rng, gap) + hp + seed + tp
        lo = self.nq + gap
        self.reads.append(read)
        self.qpos.append(lo + len(hp)); self.rpos.append(r + self.ref_base); self.rev.append(rev)
        self.first.append(len(self.qpos) - 1); self.last.append(len(self.qpos) - 1)
        self.q_lo.append(lo); self.q_hi.append(lo + len(hp) + K + len(tp))
        self.nq += len(read)
        return len(self.first) - 1

    def arrays(self):
        """-> qtext, rtext, qpos, rpos, rev, first, last, q_lo, q_hi"""
        u32 = lambda x: np.array(x, dtype=np.uint32)      # noqa: E731
        return (np.frombuffer(b"".join(self.reads), dtype=np.uint8).copy(), np.frombuffer(bytes(self.ref), dtype=np.uint8).copy(), u32(self.qpos), u32(self.rpos),
                np.array(self.rev, dtype=np.uint8), u32(self.first), u32(self.last), u32(self.q_lo), u32(self.q_hi))
