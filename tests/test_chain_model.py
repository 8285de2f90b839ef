"""CPU: the chaining model (tests/chain_model.py) against itself -- the properties the definition in include/kmerhash_amd.h promises,
checked on random anchor lists, and the synthetic two-locus case with its known answer."""
import random

import numpy as np
import pytest

import chain_model as CM


def random_anchors(rng, m, k=15, noise=0.3):
    """a noisy diagonal on each strand plus random hits, in query order"""
    q, r, v = [], [], []
    for i in range(m):
        if rng.random() < noise:
            q.append(rng.randrange(0, 4 * m)); r.append(rng.randrange(0, 4 * m)); v.append(rng.randrange(2))
        else:
            s = rng.randrange(2)
            p = 3 * i + rng.randrange(0, 3)
            q.append(p); r.append(1000 + p + rng.randrange(-2, 3) if s == 0 else 100000 - p + rng.randrange(-2, 3)); v.append(s)
    order = sorted(range(m), key=lambda i: (q[i], r[i]))
    return [q[i] for i in order], [r[i] for i in order], [v[i] for i in order]


CASES = [(seed, m, h) for seed, m, h in ((1, 300, 64), (2, 500, 8), (3, 257, 64), (4, 64, 3))]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "seed%d-m%d-h%d" % c)
def case(request):
    seed, m, h = request.param
    q, r, v = random_anchors(random.Random(seed), m)
    segs = [0, m // 3, m // 3, m]
    return q, r, v, segs, CM.chain(q, r, v, 15, segs, lookback=h, max_gap=200, band=50, min_score=20, min_count=2)


def members(res, m):
    """start anchor -> the anchors of its chain, ascending"""
    head, out = [0] * m, {}
    for i in range(m):
        head[i] = i if res.start[i] else head[res.pred[i]]
        out.setdefault(head[i], []).append(i)
    return out


def test_chains_partition_the_anchors(case):
    q, r, v, segs, res = case
    m = len(q)
    mem = members(res, m)
    assert sorted(i for c in mem.values() for i in c) == list(range(m))
    kept = [s for s in sorted(mem) if res.chain[s] >= 0]
    assert [int(res.chain[s]) for s in kept] == list(range(len(kept))) == list(range(len(res.first)))
    assert res.first.tolist() == kept
    for s, c in mem.items():
        assert len({int(res.chain[i]) for i in c}) == 1
    assert int(res.count.sum()) == int((res.chain >= 0).sum())
    assert len(kept) > 1 and len(kept) < len(mem)           # (the filter keeps some and drops some)


def test_each_chain_is_a_pred_path_inside_one_segment(case):
    q, r, v, segs, res = case
    seg_of = [0] * len(q)
    for s in range(len(segs) - 1):
        for i in range(segs[s], segs[s + 1]):
            seg_of[i] = s
    for s, c in members(res, len(q)).items():
        assert c[0] == s and c == sorted(c)
        for x, y in zip(c, c[1:]):
            assert res.pred[y] == x and res.best_child[x] == y
        assert len({seg_of[i] for i in c}) == 1
        if res.pred[s] >= 0:
            assert seg_of[res.pred[s]] == seg_of[s]


def test_score_identities(case):
    q, r, v, segs, res = case
    mem = members(res, len(q))
    for n, s in enumerate(res.first.tolist()):
        c = mem[s]
        assert res.last[n] == c[-1] and res.count[n] == len(c)
        base = 0 if res.pred[s] < 0 else int(res.score[res.pred[s]])
        assert res.cscore[n] == res.score[c[-1]] - base
        if res.pred[s] < 0:
            assert res.cscore[n] == res.score[c[-1]]
        assert res.cscore[n] >= 20 and res.count[n] >= 2
    for s, c in mem.items():                                # a dropped chain fails the filter
        if res.chain[s] < 0:
            sc = int(res.score[c[-1]]) - (0 if res.pred[s] < 0 else int(res.score[res.pred[s]]))
            assert sc < 20 or len(c) < 2


def test_g_of_a_root_is_the_maximum_f_of_its_tree(case):
    q, r, v, segs, res = case
    m = len(q)
    root, best = [0] * m, {}
    for i in range(m):
        root[i] = i if res.pred[i] < 0 else root[res.pred[i]]
        best[root[i]] = max(best.get(root[i], 0), int(res.score[i]))
    assert len(best) < m
    for t, b in best.items():
        assert res.g[t] == b
    for i in range(m):                                      # f grows along a link, and g never lies below f
        assert res.g[i] >= res.score[i] >= 15
        if res.pred[i] >= 0:
            assert res.score[i] > 15 and 0 < i - res.pred[i] <= 64


def test_lookback_one_links_only_neighbours():
    q, r, v = random_anchors(random.Random(7), 400, noise=0.1)
    res = CM.chain(q, r, v, 15, None, lookback=1, max_gap=200, band=50)
    linked = [i for i in range(400) if res.pred[i] >= 0]
    assert linked and all(res.pred[i] == i - 1 for i in linked)
    wide = CM.chain(q, r, v, 15, None, lookback=64, max_gap=200, band=50)
    assert any(wide.pred[i] >= 0 and wide.pred[i] != i - 1 for i in range(400))


def test_cost_and_invalid_positions():
    assert [CM.cost(15, d) for d in (0, 1, 2, 3, 4, 9, 128)] == [0, 0, 0, 0, 1, 2, 18]
    assert CM.cost(64, 2 ** 31 - 1) == ((64 * (2 ** 31 - 1)) >> 7) + 15
    q = [0, 10, 20, CM.POS_INVALID, 30, 2 ** 31, 40]
    r = [0, 10, 20, CM.POS_INVALID, 30, 35, 2 ** 31 + 5]
    res = CM.chain(q, r, [0, 2, 4, 0, 0, 0, 0], 15, None, min_score=0, min_count=1)     # (only bit 0 of rev counts)
    assert res.score.tolist() == [15, 25, 35, 15, 45, 15, 15] and res.pred.tolist() == [-1, 0, 1, -1, 2, -1, -1]
    assert res.count.tolist() == [4, 1, 1, 1]


@pytest.fixture(scope="module")
def synthetic():
    ref, query = CM.synthetic_texts()
    return CM.all_window_anchors(ref, query, 15)


def test_the_synthetic_case_gives_its_two_chains(synthetic):
    q, r, v = synthetic
    assert len(q) == 2911
    res = CM.chain(q, r, v, 15, None, lookback=64, max_gap=5000, band=500, min_score=40, min_count=3)
    assert res.count.tolist() == [1925, 986] and res.cscore.tolist() == [1994, 1000]
    assert [v[i] for i in res.first.tolist()] == [0, 1]
    assert abs(r[res.first[0]] - 5000) <= 15 and abs(r[res.last[0]] + 15 - 7000) <= 15
    assert abs(r[res.last[1]] - 12000) <= 15 and abs(r[res.first[1]] + 15 - 13000) <= 15


def test_a_segment_boundary_splits_a_collinear_run():
    q = list(range(0, 400, 4))
    r = [1000 + x for x in q]
    v = [0] * len(q)
    one = CM.chain(q, r, v, 15, [0, 100], min_score=40, min_count=3)
    two = CM.chain(q, r, v, 15, [0, 50, 100], min_score=40, min_count=3)
    assert one.count.tolist() == [100] and two.count.tolist() == [50, 50]
    assert two.first.tolist() == [0, 50] and two.pred[50] == -1 and one.pred[50] == 49
    assert two.cscore.tolist() == [15 + 4 * 49] * 2 and one.cscore.tolist() == [15 + 4 * 99]
    assert np.array_equal(two.chain, np.repeat([0, 1], 50))
