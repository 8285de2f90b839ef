"""Cases for kh_anchor_targets, shared by the model test (CPU) and the kernel test (GPU): a Case holds the call's inputs as numpy arrays
and model() is what tests/targets_model.py makes of them."""
from collections import namedtuple

import numpy as np

import targets_model as TM

STAGED_MAX = 8192                                   # KH_TARGETS_STAGED_MAX
N_T = (1, 2, 64, 65, STAGED_MAX, STAGED_MAX + 1)
SIZES = (0, 1, 63, 64, 65, 129, 300)                # anchors per segment: empty, one, around a wavefront, several tiles
FIELDS = "qpos rpos rev seg t_start t_end".split()


class Case(namedtuple("Case", FIELDS + ["k"])):
    def model(self):
        return TM.anchor_targets(self.qpos, self.rpos, self.rev, self.seg, self.t_start, self.t_end, self.k)


def table(n_t, rng, spacer=32):
    """n_t targets of 70..260 bases, `spacer` apart, from coordinate 0"""
    lengths = rng.randint(70, 261, size=n_t).astype(np.int64)
    ends = np.cumsum(lengths) + spacer * np.arange(n_t)
    return (ends - lengths).astype(np.uint32), ends.astype(np.uint32)


def special_positions(ts, te, k, rng, n):
    """n positions cycling through: a target's first base, the last place a seed fits, one past it (NONE), a spacer byte (NONE), a place
    inside, >= 2^31 (NONE), beyond the last target (NONE)"""
    t = rng.randint(0, len(ts), size=n)
    a, b = ts[t].astype(np.int64), te[t].astype(np.int64)
    kinds = np.arange(n) % 7
    inside = a + (rng.randint(0, 1 << 30, size=n) % np.maximum(b - a - k + 1, 1))
    pos = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3, kinds == 4, kinds == 5],
                    [a, b - k, b - k + 1, b + rng.randint(0, 32, size=n), inside, (1 << 31) + rng.randint(0, 1 << 31, size=n)], int(te[-1]) + rng.randint(0, 99, size=n))
    return pos.astype(np.uint32)


def batch(n_t, k, seed, sizes=SIZES, seg=True):
    rng = np.random.RandomState(seed)
    ts, te = table(n_t, rng)
    m = int(sum(sizes))
    rpos = special_positions(ts, te, k, rng, m)
    rng.shuffle(rpos)
    qpos = rng.randint(0, 1 << 20, size=m).astype(np.uint32)
    rev = rng.randint(0, 256, size=m).astype(np.uint8)      # all eight bits travel
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64) if seg else None
    return Case(qpos, rpos, rev, offs, ts, te, k)


def cases():
    out = {}
    for n_t in N_T:
        out["sizes_nt%d" % n_t] = batch(n_t, 15, 100 + n_t)
    out["sizes_k63"] = batch(65, 63, 7)
    out["sizes_k1"] = batch(64, 1, 8)
    out["no_segments"] = batch(65, 15, 9, seg=False)        # seg_offsets == NULL: one segment of 622 anchors
    # a read whose 65 anchors hit 65 different targets, in descending order of target; then a read of one anchor
    rng = np.random.RandomState(11)
    ts, te = table(80, rng)
    order = np.arange(64, -1, -1)
    out["65_targets"] = Case(np.arange(66, dtype=np.uint32), np.concatenate([ts[order] + 3, ts[70:71]]).astype(np.uint32), np.zeros(66, dtype=np.uint8),
                             np.array([0, 65, 66], dtype=np.uint64), ts, te, 15)
    # reads whose anchors all hit one target: the regrouping is the identity
    r = np.concatenate([ts[5] + rng.randint(0, 50, size=100), ts[9] + rng.randint(0, 50, size=64), ts[0] + rng.randint(0, 50, size=3)]).astype(np.uint32)
    out["identity"] = Case(rng.randint(0, 999, size=167).astype(np.uint32), r, rng.randint(0, 2, size=167).astype(np.uint8),
                           np.array([0, 100, 100, 164, 167], dtype=np.uint64), ts, te, 15)
    # a garbage table (descending): the ids are the loop's, whatever they mean
    c = batch(65, 15, 12)
    out["descending_table"] = c._replace(t_start=c.t_start[::-1].copy(), t_end=c.t_end[::-1].copy())
    c = batch(STAGED_MAX + 1, 15, 13, sizes=(5, 70))
    out["descending_table_large"] = c._replace(t_start=c.t_start[::-1].copy(), t_end=c.t_end[::-1].copy())
    return out


def broken_offsets(m):
    """segment offsets over m >= 8 anchors that do not ascend from 0 to m"""
    return {"first_not_0": [1, 4, m], "last_not_m": [0, 4, m - 1], "beyond_m": [0, m + 3, m], "descending": [0, 6, 2, m], "huge": [0, 1 << 40, m],
            "last_beyond": [0, 4, m + 1]}
