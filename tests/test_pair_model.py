"""CPU: the model of kh_pair_chains (tests/pair_model.py) gives the hand-written outputs of the named cases, and on planted fragments --
200 pairs whose two true rows stand at known places among decoy rows, every tenth fragment inside an exact duplicate -- it recovers
each planted combination: proper, the planted rows, the planted fragment length as template length, quality 60 outside the duplicate and
0 inside it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pair_cases import CASES, EXPECT, planted_table  # noqa: E402
from pair_model import NAMES, pair_model  # noqa: E402


def run(a):
    a = dict(a)
    return pair_model(a.pop("rs"), a.pop("re"), a.pop("rev"), a.pop("score"), a.pop("read_offsets"), a.pop("tid"), a.pop("use"), a.pop("mapq"), **a)


def test_every_case_has_an_expectation():
    assert set(CASES) == set(EXPECT)


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_case(name):
    got = run(CASES[name])
    for field, g, want in zip(NAMES, got, EXPECT[name]):
        assert [int(x) for x in g] == list(want), (name, field)


def test_output_types():
    got = run(CASES["no_chains_pair"])
    assert [g.dtype for g in got] == [np.int32, np.uint8, np.int32, np.uint8, np.int32, np.uint32]
    assert [len(g) for g in got] == [4, 4, 4, 2, 2, 2]


def test_planted_fragments_are_recovered():
    args, truth = planted_table()
    assert len(truth) == 200 and sum(1 for t in truth if t[3]) == 20
    row, mapq, tlen, flag, score, nconc = run(args)
    for p, (r1, r2, frag, in_dup, flip) in enumerate(truth):
        assert flag[p] == 7 and score[p] == 200, p
        sign = -1 if flip else 1      # (flip: mate 1 is the reverse one, downstream)
        if in_dup:
            # both copies hold the whole fragment with the same score: the smaller chain numbers win, and nothing tells them apart
            assert nconc[p] >= 2 and (mapq[2 * p], mapq[2 * p + 1]) == (0, 0), p
            assert abs(int(tlen[2 * p])) == frag and tlen[2 * p] == -tlen[2 * p + 1], p
        else:
            assert (row[2 * p], row[2 * p + 1]) == (r1, r2) and nconc[p] >= 1, p
            assert (tlen[2 * p], tlen[2 * p + 1]) == (sign * frag, -sign * frag), p
            assert (mapq[2 * p], mapq[2 * p + 1]) == (60, 60), p
