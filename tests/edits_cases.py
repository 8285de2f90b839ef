"""TEST HELPER (not collected): hand-made chains for the tests of kh_chain_edits -- random bases, planted substitutions, and a batch that
lays (A, B) string pairs out in a query text and a reference text with the anchors, pred and chain arrays that name them as links."""
import random

import numpy as np

K = 15
COMP = {65: 84, 67: 71, 71: 67, 84: 65, 97: 116, 99: 103, 103: 99, 116: 97}


def revcomp(s):
    return bytes(COMP.get(b, b) for b in reversed(s))


def bases(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def other(rng, b):
    return rng.choice([c for c in b"ACGT" if c != (b & 0xDF)])


def sub(rng, s, positions):
    s = bytearray(s)
    for p in positions:
        s[p] = other(rng, s[p])
    return bytes(s)


class Batch:
    """texts and anchors of hand-made chains: a chain is a list of (A, B) string pairs, one per link, laid out so that link t of the
    chain has exactly A_t in the query and B_t (forward) or its reverse complement (reverse strand) in the reference"""

    def __init__(self, seed, k=K, ref_base=0):
        self.rng, self.k, self.ref_base = random.Random(seed), k, ref_base
        self.q, self.r = bytearray(), bytearray()
        self.qpos, self.rpos, self.rev, self.pred, self.chain, self.n_chains = [], [], [], [], [], 0

    def add(self, pairs, rev=0, pad=True):
        """-> the anchor index of the chain's first link"""
        k, rng = self.k, self.rng
        if pad:
            self.q += bases(rng, rng.randrange(1, 5)); self.r += bases(rng, rng.randrange(1, 5))
        q0, r0, first = len(self.q), len(self.r), len(self.qpos)
        seed = bases(rng, k)
        self.q += b"".join(a for a, _ in pairs) + seed
        if rev:
            self.r += revcomp(seed) + b"".join(revcomp(b) for _, b in reversed(pairs))
            rp = r0 + sum(len(b) for _, b in pairs)
        else:
            self.r += b"".join(b for _, b in pairs) + seed
            rp = r0
        qp = q0
        for t in range(len(pairs) + 1):
            self.qpos.append(qp); self.rpos.append(rp + self.ref_base); self.rev.append(rev)
            self.pred.append(first + t - 1 if t else -1); self.chain.append(self.n_chains)
            if t < len(pairs):
                qp += len(pairs[t][0]); rp += -len(pairs[t][1]) if rev else len(pairs[t][1])
        self.n_chains += 1
        return first + 1

    def arrays(self):
        return (np.frombuffer(bytes(self.q), dtype=np.uint8).copy(), np.frombuffer(bytes(self.r), dtype=np.uint8).copy(), np.array(self.qpos, dtype=np.uint32),
                np.array(self.rpos, dtype=np.uint32), np.array(self.rev, dtype=np.uint8), np.array(self.pred, dtype=np.int32), np.array(self.chain, dtype=np.int32))
