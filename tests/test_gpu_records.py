"""GPU: kh_chain_records against its model (tests/records_model.py) on the hand-made cases of tests/records_cases.py: chains of 1 to 200
members (the carry across 64-anchor steps), interleaved chains, rows that collapse into one run and rows of which nothing merges, empty
ends, clips, an empty link row, first / last / chain numbers / offsets that are garbage, both strands with ref_order 0 and 1, no chains,
no anchors.  Host and device memory give the model's bits in every output, two calls give identical bits, the count-only call agrees
with the full one, a short out_ops is refused with *n_ops set, and on consistent valid rows the run sums equal the intervals."""
import ctypes as C
import os
import sys
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
import records_model as RM  # noqa: E402
import records_cases as RC  # noqa: E402
from stream_checks import to_dev  # noqa: E402

CASES = RC.cases()
OUT = "valid qs qe rs re qlen n_match n_block nm offsets ops".split()
Cig = namedtuple("Cig", "offsets ops")
End = namedtuple("End", "q r clip offsets ops")


@pytest.fixture(scope="module")
def models():
    return {(name, ro): case.model(ro) for name, case in CASES.items() for ro in (0, 1)}


def call(case, ref_order, dev):
    a = {f: (to_dev(v) if dev else v) for f, v in case.a.items()}
    rec = kh.chain_records(a["qpos"], a["rpos"], a["rev"], a["chain"], Cig(a["lk_offsets"], a["lk_ops"]), a["first"], a["last"], a["q_lo"], a["q_hi"],
                           End(a["e_q"], a["e_r"], a["e_clip"], a["en_offsets"], a["en_ops"]), case.k, bool(ref_order))
    if dev:
        torch.cuda.synchronize()
        assert rec.valid.dtype == torch.uint8 and rec.offsets.dtype == torch.int64 and all(getattr(rec, f).dtype == torch.int32 for f in OUT[1:9] + ["ops"])
        return [x.cpu().numpy() for x in rec]
    return list(rec)


def as_model(got):
    return {f: [int(v) for v in np.asarray(x).view(np.uint8 if f == "valid" else np.uint64 if f == "offsets" else np.uint32)] for f, x in zip(OUT, got)}


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("ref_order", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_model_bit_for_bit(models, name, ref_order, dev):
    case, exp = CASES[name], models[(name, ref_order)]
    got = call(case, ref_order, dev)
    g = as_model(got)
    for f in OUT:
        assert g[f] == exp[f], (name, f)
    again = call(case, ref_order, dev)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bits"


def test_the_cases_cover_what_they_claim(models):
    one = models[("members_200_cascade", 0)]
    assert one["valid"] == [1] and len(one["ops"]) == 1 and one["ops"][0] == ((9 + 199 * 20 + RC.K + 8) << 4) | RM.OP_EQ      # one run across all steps
    alt = models[("members_129_alternating", 0)]
    assert alt["valid"] == [1] and len(alt["ops"]) == 1 + 128 + 1 + 1                       # head, 128 links, the seed, the tail: nothing merges
    assert models[("one_empty_link_row", 0)]["valid"] == [0, 1]
    assert models[("three_interleaved", 0)]["valid"] == [1, 1, 1]
    assert models[("link_rows_63_and_64", 0)]["valid"] == [1, 0]
    for name in ("last_beyond_m", "chain_of_first_is_another", "read_too_short"):
        assert 0 in models[(name, 0)]["valid"] and 1 in models[(name, 0)]["valid"], name
    rev0, rev1 = models[("reverse_chains", 0)], models[("reverse_chains", 1)]
    o = rev0["offsets"]
    assert rev0["ops"] != rev1["ops"] and rev0["ops"][o[2]:] == rev1["ops"][o[2]:] and rev0["ops"][:o[1]] == rev1["ops"][:o[1]][::-1]


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c.consistent))
def test_run_sums_equal_the_intervals_on_valid_rows(name):
    case = CASES[name]
    g = as_model(call(case, 1, True))
    checked = 0
    for c, ok in enumerate(g["valid"]):
        if not ok:
            continue
        runs = [(v & 15, v >> 4) for v in g["ops"][g["offsets"][c]:g["offsets"][c + 1]]]
        assert sum(n for o, n in runs if o in (RM.OP_S, RM.OP_EQ, RM.OP_X, RM.OP_I)) == g["qlen"][c], (name, c)
        assert g["qe"][c] - g["qs"][c] == sum(n for o, n in runs if o in (RM.OP_EQ, RM.OP_X, RM.OP_I)), (name, c)
        assert g["re"][c] - g["rs"][c] == sum(n for o, n in runs if o in (RM.OP_EQ, RM.OP_X, RM.OP_D)), (name, c)
        assert g["n_block"][c] == g["n_match"][c] + g["nm"][c] == sum(n for o, n in runs if o != RM.OP_S)
        checked += 1
    assert checked >= 1


def raw_call(case, ref_order, dev, cap, with_ops=True):
    """the C entry point itself -> (status, n_ops, outputs as numpy, ops as numpy)"""
    mk = to_dev if dev else (lambda x: x)
    a = {f: mk(v) for f, v in case.a.items()}
    ptr = lambda x: (x.data_ptr() if dev else x.ctypes.data) if len(x) else None      # noqa: E731
    nc, m = len(case.a["first"]), len(case.a["qpos"])
    new = lambda n, dt: (torch.full((n,), 0x55, dtype={np.uint8: torch.uint8, np.uint32: torch.int32, np.uint64: torch.int64}[dt], device="cuda") if dev      # noqa: E731
                         else np.full(n, 0x55, dtype=dt))
    outs = [new(nc, np.uint8)] + [new(nc, np.uint32) for _ in range(8)] + [new(nc + 1, np.uint64)]
    ops = new(max(cap, 1), np.uint32)
    n = C.c_uint64(12345)
    st = K.lib().kh_chain_records(ptr(a["qpos"]), ptr(a["rpos"]), ptr(a["rev"]), ptr(a["chain"]), m, ptr(a["lk_offsets"]), ptr(a["lk_ops"]), len(case.a["lk_ops"]),
                                  ptr(a["first"]), ptr(a["last"]), ptr(a["q_lo"]), ptr(a["q_hi"]), nc, ptr(a["e_q"]), ptr(a["e_r"]), ptr(a["e_clip"]), ptr(a["en_offsets"]),
                                  ptr(a["en_ops"]), len(case.a["en_ops"]), case.k, ref_order, K.KH_MEM_DEVICE if dev else K.KH_MEM_HOST, *(ptr(x) for x in outs),
                                  ptr(ops) if with_ops else None, cap, C.byref(n), 0, None)
    if dev:
        torch.cuda.synchronize()
    host = lambda x: x.cpu().numpy() if dev else x      # noqa: E731
    return st, n.value, [host(x) for x in outs], host(ops)


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("name", ["three_interleaved", "members_65_mixed", "link_offsets_descend"])
def test_count_only_short_and_exact_capacity(models, name, dev):
    case, exp = CASES[name], models[(name, 1)]
    total = len(exp["ops"])
    assert total >= 3
    st, n, outs, ops = raw_call(case, 1, dev, 0, with_ops=False)                       # count only
    assert (st, n) == (K.KH_OK, total)
    counted = as_model(outs + [np.zeros(0, dtype=np.uint32)])
    for f in OUT[:10]:
        assert counted[f] == exp[f], (name, f)
    st, n, outs, ops = raw_call(case, 1, dev, total - 1)                               # one run short: refused, *n_ops set, out_ops untouched
    assert (st, n) == (K.KH_ERR_INVALID, total)
    assert (ops == 0x55).all()
    short = as_model(outs + [np.zeros(0, dtype=np.uint32)])
    for f in OUT[:10]:
        assert short[f] == exp[f], (name, f)
    st, n, outs, ops = raw_call(case, 1, dev, total)
    assert (st, n) == (K.KH_OK, total) and [int(v) for v in ops.view(np.uint32)[:total]] == exp["ops"]
