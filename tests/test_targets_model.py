"""CPU: tests/targets_model.py, the definition of kh_anchor_targets in Python integers, against a brute-force version that knows no
binary search and no running offsets: a dict from every coordinate to its target, and one sort of (segment, id, index) tuples."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import targets_cases as TC  # noqa: E402
import targets_model as TM  # noqa: E402

CASES = TC.cases()
WELL_FORMED = [n for n in sorted(CASES) if "descending" not in n]


def brute(case):
    """the expected result of a case with a well-formed table and offsets"""
    where = {}
    for t, (a, b) in enumerate(zip(case.t_start.tolist(), case.t_end.tolist())):
        for x in range(a, b - case.k + 1):                       # the places where a seed of k bases fits into target t
            where[x] = t
    m = len(case.qpos)
    seg = [0, m] if case.seg is None else case.seg.tolist()
    rows = sorted((s, where.get(int(case.rpos[i]), TM.NONE), i) for s in range(len(seg) - 1) for i in range(seg[s], seg[s + 1]))
    src = [i for _, _, i in rows]
    keys = [(s, t) for s, t, _ in rows]
    first = [j for j in range(m) if j == 0 or keys[j] != keys[j - 1]]
    return dict(ok=True, q=case.qpos[src].tolist(), r=[TM.NONE if t == TM.NONE else int(case.rpos[i]) for _, t, i in rows], v=case.rev[src].tolist(),
                tid=[t for _, t, _ in rows], src=src, g_off=first + [m], g_seg=[keys[j][0] for j in first], g_tid=[keys[j][1] for j in first])


@pytest.mark.parametrize("name", WELL_FORMED)
def test_model_equals_brute_force(name):
    case = CASES[name]
    got, exp = case.model(), brute(case)
    for f in exp:
        assert got[f] == exp[f], f


def test_the_cases_cover_what_they_claim():
    for n_t in TC.N_T:
        c = CASES["sizes_nt%d" % n_t]
        assert len(c.t_start) == n_t and np.diff(c.seg.astype(np.int64)).tolist() == list(TC.SIZES)
        r, ts, te = c.rpos.astype(np.int64), c.t_start.astype(np.int64), c.t_end.astype(np.int64)
        assert np.isin(r, ts).any() and np.isin(r, te - c.k).any() and np.isin(r, te - c.k + 1).any() and (r >= 1 << 31).any()
        t = np.searchsorted(ts, r, side="right") - 1
        assert ((r >= te[t]) & (r < te[t] + 32) & (t < n_t - 1)).any() or n_t == 1      # inside a spacer
        m = c.model()
        assert TM.NONE in m["tid"] and any(t != TM.NONE for t in m["tid"])
    m = CASES["65_targets"].model()
    assert m["g_tid"][:65] == list(range(65)) and m["g_seg"] == [0] * 65 + [1] and m["src"][:65] == list(range(64, -1, -1))
    m = CASES["identity"].model()
    assert m["src"] == list(range(167)) and m["g_off"] == [0, 100, 164, 167] and m["g_seg"] == [0, 2, 3] and m["g_tid"] == [5, 9, 0]
    assert CASES["no_segments"].seg is None and set(CASES["no_segments"].model()["g_seg"]) == {0}


def test_search_loop_on_any_table():
    # the loop is the definition for a garbage table too: the id it gives is always inside the table or NONE
    rng = np.random.RandomState(5)
    for _ in range(200):
        n = rng.randint(1, 9)
        ts, te = rng.randint(0, 50, size=n).tolist(), rng.randint(0, 80, size=n).tolist()
        for r in range(0, 60):
            t = TM.target_of(r, ts, te, 3)
            assert t == TM.NONE or (0 <= t < n and ts[t] <= r and r + 3 <= te[t])
    assert TM.target_of((1 << 31) - 1, [0], [1 << 31], 1) == 0 and TM.target_of(1 << 31, [0], [0xFFFFFFFF], 1) == TM.NONE
    assert TM.target_of(5, [6], [99], 1) == TM.NONE and TM.target_of(6, [6], [7], 1) == 0 and TM.target_of(6, [6], [7], 2) == TM.NONE


def test_segments_and_status():
    m = 9
    q = np.arange(m)
    for name, offs in TC.broken_offsets(m).items():
        assert TM.anchor_targets(q, q, q, offs, [0], [100], 3) == dict(ok=False), name
    assert TM.segments(5, [0, 9, 2, 5]) == ([(0, 5), (5, 5), (2, 5)], False)      # clamped as the chain kernels clamp
    assert TM.segments(5, None) == ([(0, 5)], True) and TM.segments(5, [0, 0, 5, 5]) == ([(0, 0), (0, 5), (5, 5)], True)
    e = TM.anchor_targets([], [], [], [0, 0, 0], [0], [9], 3)
    assert e["ok"] and e["g_off"] == [0] and e["g_seg"] == []
    # a segment without anchors has no group; NONE stands last in its segment and its rpos is invalid
    r = TM.anchor_targets([7, 8, 9], [50, 200, 3], [1, 0, 1], [0, 0, 3, 3], [0, 40], [30, 90], 5)
    assert r["src"] == [2, 0, 1] and r["tid"] == [0, 1, TM.NONE] and r["r"] == [3, 50, TM.NONE] and r["q"] == [9, 7, 8] and r["v"] == [1, 1, 0]
    assert r["g_off"] == [0, 1, 2, 3] and r["g_seg"] == [1, 1, 1] and r["g_tid"] == [0, 1, TM.NONE]
