"""CPU: the model of kh_chain_select (tests/select_model.py) against hand-worked cases -- the expected numbers stand here -- and against
the properties the rank order implies, on random input."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import select_cases as SC  # noqa: E402
from select_model import covers, mapq_of, select_model  # noqa: E402


def run(qs, qe, sc, cnt, offs=None, **kw):
    return [x.tolist() for x in select_model(np.array(qs, dtype=np.uint32), np.array(qe, dtype=np.uint32), np.array(sc, dtype=np.int32),
                                             np.array(cnt, dtype=np.uint32), offs, **kw)]


def test_two_identical_intervals():
    parent, rank, mapq, flag, sub, nsub, best = run([100, 100], [300, 300], [90, 60], [12, 12])
    assert 60 * 30 * 10 * 90 // 90000 == 18
    assert (parent, rank, mapq, sub, nsub, best) == ([0, 0], [0, 1], [18, 0], [60, 0], [1, 0], [0])
    assert flag == [3, 0]                                  # 100 * 60 < 80 * 90: not kept
    assert run([100, 100], [300, 300], [90, 72], [12, 12])[3] == [3, 2]      # 7200 >= 7200: kept


def test_lone_chains():
    assert run([0], [50], [200], [10])[2] == [60]
    assert 60 * 50 * 3 * 50 // 50000 == 9
    assert run([0], [50], [50], [3])[2] == [9]
    assert run([0], [50], [0], [10])[2] == [0] and run([0], [50], [-5], [10])[2] == [0]
    assert mapq_of(2 ** 31 - 1, 0, 2 ** 32 - 1) == 60 and 60 * (2 ** 31) * 10 * 100 < 2 ** 47


def test_ties_go_to_the_smaller_chain_number():
    parent, rank, mapq, flag, sub, nsub, best = run([0, 0, 0], [10, 10, 10], [5, 7, 7], [3, 3, 3])
    assert rank == [2, 0, 1] and parent == [1, 1, 1] and best == [1] and nsub == [0, 2, 0] and sub == [0, 7, 0]
    assert mapq == [0, 0, 0]                               # the gap to the best secondary is 0


def test_the_boundary_covers_and_one_below_does_not():
    # c = [0, 100), p = [50, 250): ov = 50, min length 100: 100 * 50 == 50 * 100
    assert covers(0, 100, 50, 250, 50) and not covers(0, 100, 51, 250, 50)
    assert run([50, 0], [250, 100], [9, 8], [3, 3])[0] == [0, 0]
    assert run([51, 0], [250, 100], [9, 8], [3, 3])[0] == [0, 1]


def test_a_secondary_never_becomes_a_parent():
    # A = [0, 100) covers B = [40, 140) (ov 60); B would cover C = [90, 190) (ov 50) but A does not (ov 10)
    parent, rank, mapq, flag, sub, nsub, best = run([0, 40, 90], [100, 140, 190], [30, 20, 10], [5, 5, 5])
    assert parent == [0, 0, 2] and flag == [3, 0, 3] and nsub == [1, 0, 0]


def test_mask_pct_0_and_100():
    qs, qe, sc, cnt = [0, 1000, 0], [100, 1100, 50], [9, 8, 7], [3, 3, 3]
    assert run(qs, qe, sc, cnt, mask_pct=0)[0] == [0, 0, 0]            # one primary per read, disjoint or not
    assert run(qs, qe, sc, cnt, mask_pct=100)[0] == [0, 1, 0]          # [0, 50) lies wholly inside [0, 100)
    assert run([0, 1], [100, 101], [9, 8], [3, 3], mask_pct=100)[0] == [0, 1]


def test_zero_length_and_inverted_intervals_are_covered_by_anything():
    parent = run([0, 5000, 7000], [100, 5000, 6000], [9, 8, 7], [3, 3, 3])[0]
    assert parent == [0, 0, 0]
    # ... and as a primary they cover everything that comes later
    assert run([5000, 0], [5000, 100], [9, 8], [3, 3])[0] == [0, 0]


def test_pri_pct_and_best_n():
    qs, qe, sc, cnt = [0] * 4, [100] * 4, [100, 90, 80, 10], [5] * 4
    assert run(qs, qe, sc, cnt)[3] == [3, 2, 2, 0]
    assert run(qs, qe, sc, cnt, pri_pct=0)[3] == [3, 2, 2, 2]
    assert run(qs, qe, sc, cnt, pri_pct=100)[3] == [3, 0, 0, 0]
    assert run(qs, qe, [100, 100, 80, 10], cnt, pri_pct=100)[3] == [3, 2, 0, 0]
    assert run(qs, qe, sc, cnt, best_n=0)[3] == [3, 0, 0, 0]
    assert run(qs, qe, sc, cnt, best_n=1)[3] == [3, 2, 0, 0]
    # the ordinal counts every earlier secondary of the parent, kept or not, and a negative parent keeps what 100 s >= pri s_p keeps
    assert run(qs, qe, [-10, -11, -12, -13], cnt, pri_pct=100, best_n=2)[3] == [3, 0, 0, 0]
    assert run(qs, qe, [-10, -11, -12, -13], cnt, pri_pct=0, best_n=2)[3] == [3, 0, 0, 0]
    assert run(qs, qe, [10, -1, -2, -3], cnt, pri_pct=0, best_n=2)[3] == [3, 0, 0, 0]
    assert run(qs, qe, [10, 0, 0, 0], cnt, pri_pct=0, best_n=2)[3] == [3, 2, 2, 0]


def test_groups_and_the_empty_group():
    offs = np.array([0, 0, 2, 2, 3], dtype=np.uint64)
    parent, rank, mapq, flag, sub, nsub, best = run([0, 0, 0], [10, 10, 10], [5, 9, 4], [10, 10, 10], offs)
    assert best == [-1, 1, -1, 2] and parent == [1, 1, 2] and rank == [1, 0, 0]
    assert sub == [0, 5, 0] and nsub == [0, 1, 0]
    assert mapq == [0, 60 * 4 * 10 * 9 // 9000, 60 * 4 * 10 * 4 // 4000]
    assert [len(x) for x in run([], [], [], [])] == [0] * 6 + [1] and run([], [], [], [])[6] == [-1]


@pytest.mark.parametrize("score_kind", SC.SCORES)
@pytest.mark.parametrize("shape_kind", SC.SHAPES)
def test_rank_based_properties(score_kind, shape_kind):
    qs, qe, sc, cnt, offs = SC.batch((0, 1, 2, 7, 40, 90, 0), score_kind, shape_kind, seed=5)
    for kw in ({}, {"mask_pct": 0, "best_n": 1}, {"mask_pct": 100, "pri_pct": 0}, {"mask_pct": 30, "pri_pct": 100, "best_n": 3}):
        mask, pri, bn = kw.get("mask_pct", 50), kw.get("pri_pct", 80), kw.get("best_n", 5)
        parent, rank, mapq, flag, sub, nsub, best = select_model(qs, qe, sc, cnt, offs, **kw)
        for g in range(len(offs) - 1):
            a, b = int(offs[g]), int(offs[g + 1])
            if a == b:
                assert best[g] == -1
                continue
            ids = sorted(range(a, b), key=lambda c: int(rank[c]))
            assert [int(rank[c]) for c in ids] == list(range(b - a)) and best[g] == ids[0]
            assert all((int(sc[x]), -x) > (int(sc[y]), -y) for x, y in zip(ids, ids[1:]))
            prim = [c for c in ids if flag[c] & 1]
            for c in ids:
                p = int(parent[c])
                assert a <= p < b and flag[p] & 1 and rank[p] <= rank[c] and (p == c) == bool(flag[c] & 1)
                if p != c:
                    assert covers(int(qs[c]), int(qe[c]), int(qs[p]), int(qe[p]), mask)
                    assert not any(covers(int(qs[c]), int(qe[c]), int(qs[x]), int(qe[x]), mask) for x in prim if rank[x] < rank[p])
                    assert mapq[c] == 0 and sub[c] == 0 and nsub[c] == 0
            for i, x in enumerate(prim):                 # a primary is covered by no earlier primary
                assert not any(covers(int(qs[x]), int(qe[x]), int(qs[y]), int(qe[y]), mask) for y in prim[:i])
                subs = [c for c in ids if parent[c] == x and c != x]
                assert nsub[x] == len(subs) and sub[x] == (max(0, int(sc[subs[0]])) if subs else 0) and flag[x] == 3
                assert 0 <= mapq[x] <= 60 and sub[x] <= max(0, int(sc[x]))
                kept = [bool(flag[c] & 2) for c in subs]
                assert kept == sorted(kept, reverse=True) and sum(kept) <= bn      # a prefix of its secondaries in rank order
                assert all(100 * int(sc[c]) >= pri * int(sc[x]) for c, k in zip(subs, kept) if k)
