"""GPU: stream order of kh_record_diffs and kh_oriented_rows, with the helpers of tests/stream_checks.py: the runs and the reference text
(the row bounds and the text of the copy) are decoys until a side stream has drained a delay and copied the real ones in, so a call whose
count pass, scan or emit pass runs on any other stream works on the decoy.  Device memory; the calls wait for their own stream once per
pass; the caller never waits.  The side stream's results equal those of the default stream and the model, and a second call gives
identical bits."""
import os
import sys
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import diffs_cases as DC  # noqa: E402
import diffs_model as DM  # noqa: E402
import orient_model as OM  # noqa: E402
from stream_checks import assert_busy, consume_on, late_inputs, side_stream, to_dev  # noqa: E402

Rec = namedtuple("Rec", "valid rs offsets ops")


@pytest.mark.parametrize("kind", ["cs", "md"])
def test_record_diffs_reads_its_late_inputs_on_the_callers_stream(kind):
    a, _ = DC.planted(7, n_rows=120)
    op = a["ops"] & np.uint32(15)
    decoy_ops = np.where(op == 7, a["ops"] + np.uint32(1), np.where(op == 8, a["ops"] - np.uint32(1), a["ops"])).astype(np.uint32)      # '=' <-> X
    decoy_ref = np.roll(a["rtext"], 1)
    model = lambda ops, rt: DM.record_diffs(a["qtext"], rt, a["ref_base"], a["offsets"], ops, a["valid"], a["rev"], a["q_lo"], a["q_hi"], a["rs"], DM.CS if kind == "cs" else DM.MD)  # noqa: E731
    exp = model(a["ops"], a["rtext"])
    assert all(exp["ok"]) and model(decoy_ops, a["rtext"])["offsets"] != exp["offsets"] and model(a["ops"], decoy_ref)["text"] != exp["text"]
    d = {f: to_dev(v) for f, v in a.items() if f != "ref_base"}
    call = lambda ops, rt: kh.record_diffs(d["qtext"], rt, Rec(d["valid"], d["rs"], d["offsets"], ops), d["rev"], d["q_lo"], d["q_hi"], kind, a["ref_base"])  # noqa: E731
    default = [x.cpu().numpy() for x in call(d["ops"], d["rtext"])]
    s = side_stream()
    try:
        with torch.cuda.stream(s):            # once before on the decoys: the scratch blocks of the real call are then at hand in the pool
            call(to_dev(decoy_ops), to_dev(decoy_ref))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            late_ops, late_ref = late_inputs(s, (a["ops"], decoy_ops), (a["rtext"], decoy_ref))
            assert_busy(s)
            got = consume_on(s, *call(late_ops, late_ref))
            again = consume_on(s, *call(late_ops, late_ref))
        assert [int(v) for v in got[0]] == exp["ok"] and [int(v) for v in got[1].view(np.uint64)] == exp["offsets"] and got[2].tobytes() == exp["text"]
        assert all(g.tobytes() == x.tobytes() for g, x in zip(got, default)), "side stream and default stream differ"
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bits"
    finally:
        s.synchronize()


@pytest.mark.parametrize("complement", [True, False])
def test_oriented_rows_reads_its_late_inputs_on_the_callers_stream(complement):
    rng = np.random.RandomState(5)
    text = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.randint(0, 9, size=40000)].copy()
    lo = rng.randint(0, 39000, size=400).astype(np.uint32)
    hi = (lo + rng.randint(0, 300, size=400)).astype(np.uint32)
    rev = rng.randint(0, 2, size=400).astype(np.uint8)
    decoy_text, decoy_lo = text[::-1].copy(), (lo + np.uint32(1)).astype(np.uint32)
    eo, et = OM.oriented_rows(text, lo, hi, rev, complement)
    assert OM.oriented_rows(text, decoy_lo, hi, rev, complement)[0] != eo and OM.oriented_rows(decoy_text, lo, hi, rev, complement)[1] != et
    dhi, drev = to_dev(hi), to_dev(rev)
    default = [x.cpu().numpy() for x in kh.oriented_rows(to_dev(text), to_dev(lo), dhi, drev, complement)]
    s = side_stream()
    try:
        with torch.cuda.stream(s):
            kh.oriented_rows(to_dev(decoy_text), to_dev(decoy_lo), dhi, drev, complement)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            late_text, late_lo = late_inputs(s, (text, decoy_text), (lo, decoy_lo))
            assert_busy(s)
            got = consume_on(s, *kh.oriented_rows(late_text, late_lo, dhi, drev, complement))
            again = consume_on(s, *kh.oriented_rows(late_text, late_lo, dhi, drev, complement))
        assert [int(v) for v in got[0].view(np.uint64)] == eo and got[1].tobytes() == et
        assert all(g.tobytes() == x.tobytes() for g, x in zip(got, default)), "side stream and default stream differ"
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bits"
    finally:
        s.synchronize()
