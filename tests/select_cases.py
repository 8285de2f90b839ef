"""TEST HELPER (not collected): chains for the tests of kh_chain_select -- group layouts, score distributions and interval shapes, all
from one seeded generator.  A case is (q_start u32, q_end u32, score i32, count u32, offsets u64)."""
import numpy as np

TILE = 2048                      # KSEL_TILE of kmerhash_amd/csrc/kh_kernels_select.h: groups beyond it are sorted and swept over scratch
BIG = 5000                       # > TILE: the radix path
SIZES = (0, 1, 2, 3, 63, 64, 65, 200, BIG, 0)            # wave path up to 64, LDS tile path, scratch path, a trailing empty group
SMALL_SIZES = (0, 1, 2, 3, 63, 64, 65, 200, 0)

SCORES = ("equal", "descending", "ascending", "ties", "nonpositive", "huge")
SHAPES = ("disjoint", "identical", "nested", "staircase", "random")


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def scores(kind, n, rng):
    i = np.arange(n, dtype=np.int64)
    if kind == "equal":
        s = np.full(n, 77, dtype=np.int64)
    elif kind == "descending":
        s = 10 * n - 3 * i
    elif kind == "ascending":
        s = 40 + 3 * i
    elif kind == "ties":
        s = rng.integers(30, 45, n)
    elif kind == "nonpositive":
        s = rng.integers(-50, 3, n)
    elif kind == "huge":
        s = rng.choice([2 ** 30, 2 ** 30 - 1, -2 ** 30, 2 ** 30 - 7, -(2 ** 30) + 1], n) + rng.integers(-2, 3, n)
    else:
        raise ValueError(kind)
    return s.astype(np.int32)


def intervals(kind, n, rng):
    """-> (q_start, q_end) of n chains of one group"""
    i = np.arange(n, dtype=np.int64)
    if kind == "disjoint":
        order = rng.permutation(n)
        qs = 100 * order
        qe = qs + 60
    elif kind == "identical":
        qs, qe = np.full(n, 500, dtype=np.int64), np.full(n, 900, dtype=np.int64)
    elif kind == "nested":
        order = rng.permutation(n)
        qs = 1000 + order
        qe = 1000 + 4 * n + 10 - order
    elif kind == "staircase":
        # length 100, step 50: neighbours overlap by exactly 50 = 50 % of the shorter; every third step is one short of it
        qs = 50 * i + (i % 3 == 2)
        qe = 50 * i + 100
    elif kind == "random":
        qs = rng.integers(0, 3000, n)
        qe = qs + rng.integers(-5, 400, n)          # a few inverted and empty ones
        qe = np.maximum(qe, 0)
    else:
        raise ValueError(kind)
    return qs.astype(np.uint32), qe.astype(np.uint32)


def batch(sizes, score_kind, shape_kind, seed=1):
    rng = np.random.default_rng(seed)
    qs, qe, sc = [], [], []
    for n in sizes:
        a, b = intervals(shape_kind, n, rng)
        qs.append(a); qe.append(b); sc.append(scores(score_kind, n, rng))
    qs, qe, sc = np.concatenate(qs), np.concatenate(qe), np.concatenate(sc)
    cnt = rng.integers(1, 16, len(qs)).astype(np.uint32)
    return qs, qe, sc, cnt, offsets_of(sizes)
