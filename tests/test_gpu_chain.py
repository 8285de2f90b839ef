"""GPU: kh_chain_anchors against the Python-integer model of tests/chain_model.py -- exact equality of all seven outputs (score, pred,
chain per anchor; first, last, count, score per kept chain), for host and for device memory.  The shapes sit on the edges of the
kernels' 64-anchor ring and tile, the rule cases on each side of every comparison of the definition; then many segments per wave,
the filter and the table's capacity, the refusals, broken segment offsets, and the index's chains() end to end."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
import chain_model as CM  # noqa: E402
from chain_cases import arrays, assert_same, check, collinear, segment_list, to_dev  # noqa: E402

INV = CM.POS_INVALID
LOOSE = dict(min_score=0, min_count=1)          # keep every chain: the table then shows the whole partition


# ---- ring and tile edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookback", [1, 2, 63, 64])
def test_segment_lengths_around_the_ring(lookback):
    rng = np.random.default_rng(lookback)
    q, r, v, seg = segment_list(rng, [0, 1, 2, 63, 64, 65, 128, 129, 200, 0], noise=0.1)
    exp = check(q, r, v, 15, seg, lookback=lookback, max_gap=200, band=50, min_score=30, min_count=2)
    assert len(exp.first) >= 6 and (exp.pred >= 0).sum() > 400
    if lookback > 1:
        assert (np.arange(len(q)) - exp.pred)[exp.pred >= 0].max() > 1


def lone_pair(gap, lead=0, tail=3):
    """a segment whose only two valid anchors are `gap` places apart and collinear; every other anchor is KH_POS_INVALID"""
    n = lead + gap + 1 + tail
    q, r = [INV] * n, [INV] * n
    q[lead], r[lead], q[lead + gap], r[lead + gap] = 100, 1100, 130, 1130
    return q, r, [0] * n


@pytest.mark.parametrize("lead", [0, 5, 63, 64, 100])
def test_the_candidate_at_64_counts_and_the_one_at_65_does_not(lead):
    q1, r1, v1 = lone_pair(64, lead)
    q2, r2, v2 = lone_pair(65, lead)
    q3, r3, v3 = lone_pair(63, lead)
    seg = [0, len(q1), len(q1) + len(q2), len(q1) + len(q2) + len(q3)]
    exp = check(q1 + q2 + q3, r1 + r2 + r3, v1 + v2 + v3, 15, seg, lookback=64, **LOOSE)
    assert exp.pred[lead + 64] == lead and exp.score[lead + 64] == 30
    assert exp.pred[seg[1] + lead + 65] == -1 and exp.score[seg[1] + lead + 65] == 15
    assert exp.pred[seg[2] + lead + 63] == seg[2] + lead
    exp = check(q1 + q2 + q3, r1 + r2 + r3, v1 + v2 + v3, 15, seg, lookback=63, **LOOSE)
    assert exp.pred[lead + 64] == -1 and exp.pred[seg[2] + lead + 63] == seg[2] + lead


@pytest.mark.parametrize("cut", [1, 30, 64, 65, 128])
def test_a_candidate_before_the_segment_start_is_ignored(cut):
    q, r, v = collinear(np.random.default_rng(cut), 140, jitter=0)
    exp = check(q, r, v, 15, [0, cut, 140], **LOOSE)
    one = check(q, r, v, 15, None, **LOOSE)
    assert exp.pred[cut] == -1 and one.pred[cut] == cut - 1 and exp.first.tolist() == [0, cut] and one.first.tolist() == [0]


# ---- rule edges ----------------------------------------------------------------------------------------------
G, B = 100, 10
RULES = {
    "dq=G": ([0, G], [0, G], [0, 0], [-1, 0]),
    "dq=G+1": ([0, G + 1], [0, G + 1], [0, 0], [-1, -1]),
    "dr=G": ([0, G - 5], [0, G], [0, 0], [-1, 0]),
    "dr=G+1": ([0, G - 4], [0, G + 1], [0, 0], [-1, -1]),
    "dr=G-rev": ([0, G - 5], [G, 0], [1, 1], [-1, 0]),
    "dr=G+1-rev": ([0, G - 4], [G + 1, 0], [1, 1], [-1, -1]),
    "dd=B": ([0, 50], [0, 50 + B], [0, 0], [-1, 0]),
    "dd=B+1": ([0, 50], [0, 50 + B + 1], [0, 0], [-1, -1]),
    "dd=B-other-side": ([0, 50 + B], [0, 50], [0, 0], [-1, 0]),
    "dd=B+1-other-side": ([0, 50 + B + 1], [0, 50], [0, 0], [-1, -1]),
    "dd=0..4": ([0, 50, 0, 50, 0, 50, 0, 50, 0, 50], [0, 50, 200, 251, 400, 452, 600, 653, 800, 854], [0] * 10, None),
    "dq=0": ([10, 10, 10, 20, 20, 20, 30], [100, 200, 300, 110, 210, 310, 120], [0] * 7, [-1, -1, -1, 0, 1, 2, 3]),
    "dr=0": ([10, 20], [100, 100], [0, 0], [-1, -1]),
    "backwards": ([20, 10], [120, 110], [0, 0], [-1, -1]),
    "rev-wrong-way": ([10, 20], [110, 120], [1, 1], [-1, -1]),
    "other-strand-nearest": ([10, 12, 14, 16, 18, 20], [100, 500, 498, 496, 494, 110], [0, 1, 1, 1, 1, 0], [-1, -1, 1, 2, 3, 0]),
    "rev-high-bits": ([10, 20, 30, 40], [100, 110, 500, 490], [0xFE, 2, 0xFF, 3], [-1, 0, -1, 2]),
    "equal-cand": ([0, 0, 20], [0, 0, 20], [0, 0, 0], [-1, -1, 1]),
    "equal-cand-3": ([0, 5, 5, 0, 40], [0, 5, 5, 0, 40], [0] * 5, [-1, 0, 0, -1, 2]),
    "cand=k": ([0, 1], [0, 5], [0, 0], [-1, -1]),
    "cand=k+1": ([0, 2], [0, 6], [0, 0], [-1, 0]),
    "invalid": ([0, 10, INV, 20, 2 ** 31, 30, 40, 2 ** 31 - 1], [0, 10, INV, 20, 25, 2 ** 31, 40, 2 ** 31 - 1], [0] * 8, [-1, 0, -1, 1, -1, -1, 3, -1]),
    "top-of-range": ([2 ** 31 - 60, 2 ** 31 - 30, 2 ** 31 - 1], [2 ** 31 - 50, 2 ** 31 - 20, 2 ** 31 - 1], [0] * 3, None),
}


@pytest.mark.parametrize("name", sorted(RULES))
def test_rule_edges(name):
    q, r, v, pred = RULES[name]
    exp = check(q, r, v, 15, None, max_gap=G, band=B, **LOOSE)
    if pred is not None:
        assert exp.pred.tolist() == pred
    # the same anchors behind a full tile of another strand's, so that they straddle the ring's wrap
    pq, pr, pv = collinear(np.random.default_rng(1), 61, rev=1, q0=5000, r0=90000)
    if all(x & 1 == 0 for x in v):
        check(pq + q, pr + r, pv + v, 15, None, max_gap=G, band=B, **LOOSE)


def test_equal_g_goes_to_the_smallest_child_and_a_higher_g_wins_the_prefix():
    # parent 0 with two children of equal g: the first is the best child, the second starts a chain whose score is counted from the parent
    exp = check([0, 10, 10], [0, 10, 10], [0, 0, 0], 15, None, **LOOSE)
    assert exp.pred.tolist() == [-1, 0, 0] and exp.chain.tolist() == [0, 0, 1]
    assert exp.first.tolist() == [0, 2] and exp.count.tolist() == [2, 1] and exp.cscore.tolist() == [25, 10]
    # child 1 has the greater f (29 against 25), child 2 the greater g (40, through anchor 3): 2 continues the parent's chain
    exp = check([0, 15, 10, 30], [0, 23, 10, 30], [0] * 4, 15, None, **LOOSE)
    assert exp.score.tolist() == [15, 29, 25, 40] and exp.pred.tolist() == [-1, 0, 0, 2]
    assert exp.chain.tolist() == [0, 1, 0, 0] and exp.first.tolist() == [0, 1] and exp.cscore.tolist() == [40, 14]
    assert exp.g[:2] == [40, 29] and exp.best_child[0] == 2


@pytest.mark.parametrize("k", [1, 15, 64])
def test_k(k):
    rng = np.random.default_rng(k)
    q, r, v, seg = segment_list(rng, [150, 70], noise=0.15)
    exp = check(q, r, v, k, seg, max_gap=300, band=100, min_score=2 * k, min_count=2)
    assert len(exp.first) >= 2
    # a wide band at k = 64: the gap cost's product passes 2^31 >> 7 per unit of k
    check([0, 50, 2 ** 30 + 100], [0, 2 ** 30, 2 ** 30 + 50], [0] * 3, k, None, max_gap=2 ** 31 - 1, band=2 ** 31 - 1, **LOOSE)


# ---- scheduling ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many():
    rng = np.random.default_rng(5)
    lengths = rng.integers(0, 201, 2800).tolist()
    lengths[0] = lengths[17] = lengths[18] = lengths[-1] = 0
    q, r, v, seg = segment_list(rng, lengths, noise=0.25, shuffle=set(range(1, 2800, 2)))
    assert 2 * 10 ** 5 < len(q) < 3 * 10 ** 5
    return q, r, v, seg


def test_many_segments_sorted_and_shuffled(many):
    q, r, v, seg = many
    exp = check(q, r, v, 15, seg, lookback=8, max_gap=300, band=60, min_score=40, min_count=3)     # (a short look-back keeps the model to seconds)
    assert len(exp.first) > 2000 and (exp.chain < 0).any()
    assert np.array_equal(np.searchsorted(seg, exp.first, side="right"), np.searchsorted(seg, exp.last, side="right"))


def test_no_offsets_is_one_segment():
    rng = np.random.default_rng(9)
    q, r, v, seg = segment_list(rng, [90, 0, 130, 64, 1], noise=0.2)
    a = check(q, r, v, 15, None, max_gap=300, band=60, **LOOSE)
    b = check(q, r, v, 15, [0, len(q)], max_gap=300, band=60, **LOOSE)
    assert_same(a, b)
    c = check(q, r, v, 15, seg, max_gap=300, band=60, **LOOSE)
    assert len(c.first) >= len(a.first)


# ---- filter and capacity (the C call itself, device and host memory) --------------------------------------------------------
def raw_call(q, r, v, seg, k=15, h=64, G_=5000, B_=500, min_score=40, min_count=3, where="device", table=True, cap=None, fill=-7):
    """kh_chain_anchors with pre-filled outputs -> (status, n_chains, [score, pred, chain], [first, last, count, cscore]) as numpy"""
    aq, ar, av, aseg = arrays(q, r, v, seg)
    m = len(aq)
    cap = m if cap is None else cap
    per = [np.full(m, fill, dtype=np.int32) for _ in range(3)]
    tab = [np.full(max(cap, 1), fill, dtype=np.int32) for _ in range(4)]
    ins = [aq, ar, av] + ([aseg] if aseg is not None else [])
    if where == "device":
        ins, per, tab = [to_dev(a) for a in ins], [to_dev(a) for a in per], [to_dev(a) for a in tab]
        ptr = lambda t: t.data_ptr()
        kind = K.KH_MEM_DEVICE
    else:
        ptr = lambda a: a.ctypes.data
        kind = K.KH_MEM_HOST
    n = C.c_uint64(12345)
    st = K.lib().kh_chain_anchors(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), m, ptr(ins[3]) if aseg is not None else None, 0 if aseg is None else len(aseg) - 1,
                                  k, h, G_, B_, min_score, min_count, kind, *[ptr(t) for t in per], *([ptr(t) for t in tab] if table else [None] * 4),
                                  cap, C.byref(n), 0, None)
    host = lambda t: t.cpu().numpy() if where == "device" else t
    return st, n.value, [host(t) for t in per], [host(t) for t in tab]


@pytest.fixture(scope="module")
def two_runs():
    q = list(range(0, 400, 4))
    return q, [1000 + x for x in q], [0] * 100, [0, 50, 100]          # two chains of 50 anchors, score 15 + 4 * 49 = 211 each


@pytest.mark.parametrize("where", ["device", "host"])
def test_filter_at_below_and_above_a_chains_values(two_runs, where):
    q, r, v, seg = two_runs
    for kw, n_exp in ((dict(min_score=211), 2), (dict(min_score=210), 2), (dict(min_score=212), 0), (dict(min_count=50), 2), (dict(min_count=49), 2),
                      (dict(min_count=51), 0), (dict(min_score=211, min_count=50), 2), (dict(min_score=-5, min_count=0), 2)):
        exp = CM.chain(q, r, v, 15, seg, **kw)
        st, n, per, tab = raw_call(q, r, v, seg, where=where, **kw)
        assert (st, n) == (K.KH_OK, n_exp) and len(exp.first) == n_exp, kw
        assert np.array_equal(per[0], exp.score) and np.array_equal(per[1], exp.pred) and np.array_equal(per[2], exp.chain), kw
        for t, e in zip(tab, (exp.first, exp.last, exp.count, exp.cscore)):
            assert np.array_equal(t[:n].view(e.dtype), e) and (t[n:] == -7).all(), kw
    check(q, r, v, 15, seg, min_score=211, min_count=50)


@pytest.mark.parametrize("where", ["device", "host"])
def test_capacity_and_no_table(two_runs, where):
    q, r, v, seg = two_runs
    exp = CM.chain(q, r, v, 15, seg)
    st, n, per, tab = raw_call(q, r, v, seg, where=where, table=False)
    assert (st, n) == (K.KH_OK, 2) and np.array_equal(per[2], exp.chain) and all((t == -7).all() for t in tab)
    st, n, per, tab = raw_call(q, r, v, seg, where=where, cap=2)
    assert (st, n) == (K.KH_OK, 2) and tab[0].view(np.uint32).tolist() == [0, 50]
    st, n, per, tab = raw_call(q, r, v, seg, where=where, cap=1)                  # one row short
    assert (st, n) == (K.KH_ERR_INVALID, 2)
    assert np.array_equal(per[0], exp.score) and np.array_equal(per[1], exp.pred) and np.array_equal(per[2], exp.chain)
    assert all((t == -7).all() for t in tab)
    st, n, per, tab = raw_call(q, r, v, seg, where=where, cap=0)
    assert (st, n) == (K.KH_ERR_INVALID, 2) and all((t == -7).all() for t in tab)


@pytest.mark.parametrize("where", ["device", "host"])
def test_empty_and_refused_calls_leave_the_outputs_alone(two_runs, where):
    q, r, v, seg = two_runs
    st, n, per, tab = raw_call([], [], [], None, where=where)
    assert (st, n) == (K.KH_OK, 0)
    st, n, per, tab = raw_call([], [], [], [0, 0, 0], where=where)
    assert (st, n) == (K.KH_OK, 0)
    for kw in (dict(k=0), dict(k=65), dict(h=0), dict(h=65), dict(G_=0), dict(G_=2 ** 31), dict(B_=2 ** 31)):
        st, n, per, tab = raw_call(q, r, v, seg, where=where, **kw)
        assert (st, n) == (K.KH_ERR_INVALID, 12345), kw
        assert all((t == -7).all() for t in per + tab), kw
    c = kh.chain_anchors(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8), 15)
    assert [len(x) for x in c] == [0] * 7


BROKEN = {"descending": [0, 200, 100, 300], "past-the-end": [0, 150, 350, 300], "all-past-the-end": [0, 340, 350, 300], "not-from-0": [5, 100, 300],
          "not-to-m": [0, 100, 290], "ends-past-m": [0, 100, 364]}


@pytest.mark.parametrize("name", sorted(BROKEN))
def test_broken_offsets_are_refused_and_touch_nothing_else(name):
    """Every array of the call lies inside one allocation between guard bands of 4096 elements, wider than any offset here overshoots.
    The kernels clamp each segment to [0, m) where they read it and range-check every index they take from memory (kch_segment,
    kch_pred_ok and the h < m / l < m tests of k_chain_emit), so a correct build reads and writes the arrays alone."""
    m, pad = 300, 4096
    q, r, v = collinear(np.random.default_rng(3), m)
    aq, ar, av, aseg = arrays(q, r, v, BROKEN[name])
    assert max(BROKEN[name]) < m + pad
    words = torch.full((9 * (m + pad) + pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    part = [words[pad + j * (m + pad): pad + j * (m + pad) + m] for j in range(9)]      # q r rev(bytes in words) score pred chain + 3 spare
    part[0].copy_(to_dev(aq)); part[1].copy_(to_dev(ar))
    rev = part[2].view(torch.uint8)[:m]
    rev.copy_(to_dev(av))
    tabs = torch.full((4, m), -7, dtype=torch.int32, device="cuda")
    seg = to_dev(aseg)
    before = words.clone()
    n = C.c_uint64(12345)
    st = K.lib().kh_chain_anchors(part[0].data_ptr(), part[1].data_ptr(), rev.data_ptr(), m, seg.data_ptr(), len(aseg) - 1, 15, 64, 5000, 500, 40, 3,
                                  K.KH_MEM_DEVICE, part[3].data_ptr(), part[4].data_ptr(), part[5].data_ptr(), *[tabs[j].data_ptr() for j in range(4)], m,
                                  C.byref(n), 0, None)
    assert (st, n.value) == (K.KH_ERR_INVALID, 0)
    keep = torch.ones_like(words, dtype=torch.bool)
    for j in (3, 4, 5):
        keep[pad + j * (m + pad): pad + j * (m + pad) + m] = False
    assert torch.equal(words[keep], before[keep])            # inputs and every guard band are as they were
    with pytest.raises(kh.KhError):
        kh.chain_anchors(aq, ar, av, 15, aseg)
    # and the same anchors with sound offsets
    check(q, r, v, 15, [0, 100, 300])


# ---- end to end ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def texts():
    ref, query = CM.synthetic_texts()
    return np.frombuffer(ref.encode(), dtype=np.uint8).copy(), np.frombuffer(query.encode(), dtype=np.uint8).copy()


INDEXES = {"all-windows": lambda: kh.KmerPositionIndex(k=15, stranded=True), "syncmers": lambda: kh.KmerPositionIndex(k=15, s=11, stranded=True),
           "wide-syncmers": lambda: kh.WideKmerPositionIndex(k=63, s=31, stranded=True)}


@pytest.mark.parametrize("name", sorted(INDEXES))
def test_chains_end_to_end(texts, name):
    ref, query = texts
    ix = INDEXES[name]()
    k = ix.k
    try:
        ix.build_sequences(ref)
        q, r, v = ix.anchors(query)
        exp = CM.chain(q, r, v, k)
        for dev in (False, True):
            t = ix.chains(to_dev(query) if dev else query)
            host = (lambda x: x.cpu().numpy()) if dev else (lambda x: x)
            aq, ar, av = (host(x) for x in t.anchors)
            assert np.array_equal(aq.view(np.uint32), q) and np.array_equal(ar.view(np.uint32), r) and np.array_equal(av, v)
            assert np.array_equal(host(t.chain), exp.chain)
            assert np.array_equal(host(t.count).view(np.uint32), exp.count) and np.array_equal(host(t.score), exp.cscore)
            f, l = exp.first.astype(np.int64), exp.last.astype(np.int64)
            assert np.array_equal(host(t.seg), np.zeros(len(f))) and np.array_equal(host(t.rev), v[f])
            assert np.array_equal(host(t.q_start).view(np.uint32), q[f]) and np.array_equal(host(t.q_end).view(np.uint32), q[l] + k)
            assert np.array_equal(host(t.r_start).view(np.uint32), np.minimum(r[f], r[l]))
            assert np.array_equal(host(t.r_end).view(np.uint32), np.maximum(r[f], r[l]) + k)
        t = ix.chains(query)
        if name == "all-windows":
            assert len(q) == 2911 and t.count.tolist() == [1925, 986] and t.score.tolist() == [1994, 1000]
        # the two loci: the best chain of each strand
        for strand, lo, hi in ((0, 5000, 7000), (1, 12000, 13000)):
            rows = np.flatnonzero(t.rev == strand)
            assert rows.size, (name, strand)
            b = rows[np.argmax(t.score[rows])]
            assert abs(int(t.r_start[b]) - lo) <= k and abs(int(t.r_end[b]) - hi) <= k, (name, strand, t.r_start[b], t.r_end[b])
        # the same reads twice: the chains twice, never across the boundary
        n = len(query)
        two = ix.chains(np.concatenate([query, query]), read_starts=[0, n])
        c = len(t.count)
        assert len(two.count) == 2 * c and two.seg.tolist() == [0] * c + [1] * c
        for name_ in ("rev", "r_start", "r_end", "count", "score"):
            assert np.array_equal(getattr(two, name_)[:c], getattr(t, name_)) and np.array_equal(getattr(two, name_)[c:], getattr(t, name_)), name_
        assert np.array_equal(two.q_start[:c], t.q_start) and np.array_equal(two.q_start[c:], t.q_start + np.uint32(n))
        assert (two.q_end[:c] <= n).all() and (two.q_start[c:] >= n).all()
        assert np.array_equal(two.chain[len(q):][two.chain[len(q):] >= 0], t.chain[t.chain >= 0] + c)
    finally:
        ix.close()


def test_chains_needs_a_stranded_index():
    ix = kh.KmerPositionIndex(k=15)
    try:
        with pytest.raises(ValueError, match="stranded=True"):
            ix.chains(b"ACGTACGTACGTACGTACGT")
        with pytest.raises(ValueError, match="read_starts"):
            sx = kh.KmerPositionIndex(k=15, stranded=True)
            try:
                sx.build_sequences(np.frombuffer(b"ACGTTGCAAGCTAGCTAGGATCGATCGATTTACG", dtype=np.uint8))
                sx.chains(b"ACGTTGCAAGCTAGCTAGGATCG", read_starts=[3, 10])
            finally:
                sx.close()
    finally:
        ix.close()
