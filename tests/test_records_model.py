"""CPU: tests/records_model.py, the yardstick of kh_chain_records and kh_cigar_text, against hand-worked rows and against the host helpers
that existed before it -- kmers.read_cigar and kmers.extended_intervals -- on inputs the other CPU models produce (chain_model,
edits_model, cigar_model, ends_model) from a synthetic query with substitutions, a deletion and a reverse-complemented piece; the text
model prints what "%d%s" prints."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import chain_model as HM  # noqa: E402
import cigar_model as CM  # noqa: E402
import edits_model as DM  # noqa: E402
import ends_model as EM  # noqa: E402
import records_cases as RC  # noqa: E402
import records_model as RM  # noqa: E402
from kmerhash_amd import kmers  # noqa: E402

EQ, X, I, D, S = RM.OP_EQ, RM.OP_X, RM.OP_I, RM.OP_D, RM.OP_S
run = lambda o, n: (n << 4) | o      # noqa: E731


def test_a_hand_worked_chain():
    # two members; link row 5= 1X 4=; head 2X 3=; tail 6= 1I; clips 4 and 0; k = 10
    a = dict(qpos=[9, 19], rpos=[105, 115], rev=[0, 0], chain=[0, 0], lk_offsets=[0, 0, 3], lk_ops=[run(EQ, 5), run(X, 1), run(EQ, 4)], first=[0], last=[1], q_lo=[0],
             q_hi=[36], e_q=[5, 7], e_r=[5, 6], e_clip=[4, 0], en_offsets=[0, 2, 4], en_ops=[run(X, 2), run(EQ, 3), run(EQ, 6), run(I, 1)])
    r = RM.records(*[a[f] for f in RC.FIELDS], 10)
    assert r["ops"] == [run(S, 4), run(X, 2), run(EQ, 8), run(X, 1), run(EQ, 20), run(I, 1)]      # 3= + 5=, then 4= + 10= + 6=
    assert (r["valid"], r["qs"], r["qe"], r["rs"], r["re"], r["qlen"]) == ([1], [4], [36], [100], [131], [36])
    assert (r["n_match"], r["n_block"], r["nm"]) == ([28], [32], [4])
    assert RM.cigar_text(r["offsets"], r["ops"]) == ([0, 13], b"4S2X8=1X20=1I")
    # the reverse strand: the head extends the reference interval upwards, the tail downwards; ref_order turns the row round
    a.update(rev=[1, 1], rpos=[115, 105])
    r1 = RM.records(*[a[f] for f in RC.FIELDS], 10, 1)
    assert (r1["rs"], r1["re"]) == ([105 - 6], [115 + 10 + 5]) and r1["ops"] == r["ops"][::-1]
    assert RM.records(*[a[f] for f in RC.FIELDS], 10, 0)["ops"] == r["ops"]
    # an empty link row: no whole alignment, an empty row, the intervals stay
    a["lk_offsets"] = [0, 0, 0]
    r2 = RM.records(*[a[f] for f in RC.FIELDS], 10, 1)
    assert (r2["valid"], r2["ops"], r2["offsets"], r2["n_block"], r2["qs"], r2["re"]) == ([0], [], [0, 0], [0], [4], [130])


def test_the_cascade_and_the_carry_of_the_merge_rule():
    out = []
    for o, n in [(EQ, 3), (EQ, 0), (EQ, 4), (X, 0), (EQ, 1), (X, 2), (X, (1 << 28) - 1)]:
        RM.feed(out, o, n)
    assert out == [[EQ, 8], [X, 1]]                                       # zero runs vanish between equal neighbours; lengths add mod 2^28
    assert RM.row([0, 64], list(range(64)), 0) == [] and len(RM.row([0, 63], list(range(64)), 0)) == 63 and RM.row([5, 2], [1] * 9, 0) == []
    assert RM.row([7, 99], [1] * 9, 0) == [1, 1]                          # bounds clamped to the runs


def test_text_model():
    ops = [run(o, n) for n in (0, 1, 9, 10, 99, 100, 12345, 10 ** 8, 2 ** 28 - 1) for o in range(16)]
    offs = [0, 3, 3, len(ops)]
    eo, et = RM.cigar_text(offs, ops)
    want = ["%d%s" % (v >> 4, ("MIDNSHP=X" + "?" * 7)[v & 15]) for v in ops]
    assert et.decode() == "".join(want) and eo == [0, len("".join(want[:3])), len("".join(want[:3])), len(et)]
    assert RM.cigar_text([2, 1, 999], ops)[0] == [0, 0, len("".join(want[2:]))]      # a bound below the first is lifted to it, one beyond is clamped


Table = collections.namedtuple("Table", "seg rev q_start q_end r_start r_end count score anchors chain")


def test_agrees_with_read_cigar_and_extended_intervals_on_model_inputs():
    k = 15
    ref, query = HM.synthetic_texts()
    ref = ref[4000:14000]
    q, r, v = HM.all_window_anchors(ref, query, k)
    c = HM.chain(q, r, v, k)
    nc = len(c[3])
    assert nc >= 2
    qt, rt = query.encode(), ref.encode()
    link, edits, over = DM.chain_edits_model(qt, rt, q, r, v, c[1], c[2], nc, k)
    cig = CM.chain_cigars_model(qt, rt, q, r, v, c[1], c[2], nc, k, link)
    lo, hi = [0] * nc, [len(query)] * nc
    ends = EM.chain_ends_model(qt, rt, q, r, v, c[3], c[4], lo, hi, k)
    qa, ra = np.array(q, dtype=np.uint32), np.array(r, dtype=np.uint32)
    f, l = c[3].astype(np.int64), c[4].astype(np.int64)
    table = Table(np.zeros(nc, dtype=np.uint32), np.array(v, dtype=np.uint8)[f], qa[f], qa[l] + np.uint32(k), np.minimum(ra[f], ra[l]), np.maximum(ra[f], ra[l]) + np.uint32(k),
                  c[5], c[6], (qa, ra, np.array(v, dtype=np.uint8)), c[2])
    cigars, cends = kmers.ChainCigars(*cig), kmers.ChainEnds(*ends)
    rec = RM.records(q, r, v, c[2], cig[0], cig[1], c[3], c[4], lo, hi, ends[0], ends[1], ends[3], ends[4], ends[5], k, 0)
    toff, text = RM.cigar_text(rec["offsets"], rec["ops"])
    q0, q1, r0, r1 = kmers.extended_intervals(table, cends)
    strands = set()
    for row in range(nc):
        s = kmers.read_cigar(cigars, cends, table, row, k)
        assert bool(rec["valid"][row]) == (s is not None)
        assert text[toff[row]:toff[row + 1]].decode() == (s or "")
        assert (rec["qs"][row], rec["qe"][row], rec["rs"][row], rec["re"][row]) == (int(q0[row]), int(q1[row]), int(r0[row]), int(r1[row]))
        if s is not None:
            assert rec["nm"][row] == int(edits[row]) + int(ends[2][2 * row]) + int(ends[2][2 * row + 1])
            strands.add(int(table.rev[row]))
    assert strands == {0, 1} and sum(rec["valid"]) >= 2
