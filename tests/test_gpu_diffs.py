"""GPU: kh_record_diffs against its model (tests/diffs_model.py) bit for bit -- ok, offsets and text -- on the cases of
tests/diffs_cases.py: both kinds, host and device memory; a cap_text one byte short is refused with the count and the offsets written and
the text untouched; the count-only pass writes what the full pass writes."""
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
import diffs_cases as DC  # noqa: E402
import diffs_model as DM  # noqa: E402
from stream_checks import to_dev  # noqa: E402

Rec = namedtuple("Rec", "valid rs offsets ops")
KINDS = {"cs": DM.CS, "md": DM.MD}


@pytest.fixture(scope="module")
def cases():
    return DC.cases()


@pytest.fixture(scope="module")
def expected(cases):
    return {(name, kind): DM.record_diffs(a["qtext"], a["rtext"], a["ref_base"], a["offsets"], a["ops"], a["valid"], a["rev"], a["q_lo"], a["q_hi"], a["rs"], KINDS[kind])
            for name, a in cases.items() for kind in KINDS}


def call(a, kind, dev):
    mk = to_dev if dev else (lambda x: x)
    got = kh.record_diffs(mk(a["qtext"]), mk(a["rtext"]), Rec(mk(a["valid"]), mk(a["rs"]), mk(a["offsets"]), mk(a["ops"])), mk(a["rev"]), mk(a["q_lo"]), mk(a["q_hi"]),
                          kind, a["ref_base"])
    if dev:
        torch.cuda.synchronize()
        got = [x.cpu().numpy() for x in got]
    return [int(v) for v in got[0]], [int(v) for v in np.asarray(got[1]).view(np.uint64)], np.asarray(got[2]).tobytes()


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", ["hand_fwd", "hand_rev", "q_beyond", "bad_offsets", "million", "garbage_1", "garbage_2", "planted"])
def test_equals_the_model(cases, expected, name, kind, dev):
    ok, offs, text = call(cases[name], kind, dev)
    exp = expected[name, kind]
    assert ok == exp["ok"]
    assert offs == exp["offsets"]
    assert text == exp["text"]


def test_the_hand_rows_hold_what_they_are_there_for(expected):
    """the cases are not vacuous: good rows and refused ones, an MD number carried across a wave step, seven digits"""
    e = expected["hand_fwd", "md"]
    rows = [e["text"][e["offsets"][i]:e["offsets"][i + 1]].decode() for i in range(len(e["ok"]))]
    assert e["ok"][:8] == [0, 1, 1, 1, 1, 1, 1, 1] and rows[8].startswith("0") and rows[10].endswith("0")
    assert rows[7][-5:-4] in "ACGTN" and rows[7][-4:-2] == "14" and rows[7][-1] == "4"      # 2 + 5 + 7 matches around the step and the insertion
    assert 0 in e["ok"][8:] and sum(e["ok"]) > 20
    assert b"1000000" in expected["million", "md"]["text"] and b":1000000" in expected["million", "cs"]["text"]


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_short_cap_is_refused_with_the_count(cases, expected, kind, dev):
    a, exp = cases["hand_rev"], expected["hand_rev", kind]
    total = len(exp["text"])
    mk = to_dev if dev else (lambda x: x)
    arrs = {f: mk(a[f]) for f in ("qtext", "rtext", "offsets", "ops", "valid", "rev", "q_lo", "q_hi", "rs")}
    ptr = (lambda t: t.data_ptr()) if dev else (lambda t: t.ctypes.data)
    rows = len(a["valid"])
    ok, offs, text = mk(np.full(rows, 7, dtype=np.uint8)), mk(np.full(rows + 1, 7, dtype=np.uint64)), mk(np.full(total, 0x55, dtype=np.uint8))
    n = C.c_uint64(99)
    args = [ptr(arrs["qtext"]), len(a["qtext"]), ptr(arrs["rtext"]), len(a["rtext"]), a["ref_base"], ptr(arrs["offsets"]), ptr(arrs["ops"]), len(a["ops"]), ptr(arrs["valid"]),
            ptr(arrs["rev"]), ptr(arrs["q_lo"]), ptr(arrs["q_hi"]), ptr(arrs["rs"]), rows, KINDS[kind], K.KH_MEM_DEVICE if dev else K.KH_MEM_HOST, ptr(ok), ptr(offs)]
    st = K.lib().kh_record_diffs(*args, ptr(text), total - 1, C.byref(n), 0, None)
    if dev:
        torch.cuda.synchronize()
    host = (lambda t: t.cpu().numpy()) if dev else (lambda t: t)
    assert st == K.KH_ERR_INVALID and n.value == total
    assert [int(v) for v in host(ok)] == exp["ok"] and [int(v) for v in host(offs).view(np.uint64)] == exp["offsets"]
    assert (host(text) == 0x55).all(), "the text was touched"
    # count only: the same numbers, no text
    ok2, offs2 = mk(np.full(rows, 7, dtype=np.uint8)), mk(np.full(rows + 1, 7, dtype=np.uint64))
    st = K.lib().kh_record_diffs(*args[:-2], ptr(ok2), ptr(offs2), None, 0, C.byref(n), 0, None)
    if dev:
        torch.cuda.synchronize()
    assert st == K.KH_OK and n.value == total
    assert host(ok2).tobytes() == host(ok).tobytes() and host(offs2).tobytes() == host(offs).tobytes()
    # the exact cap
    st = K.lib().kh_record_diffs(*args, ptr(text), total, C.byref(n), 0, None)
    if dev:
        torch.cuda.synchronize()
    assert st == K.KH_OK and host(text).tobytes() == exp["text"]
