"""GPU: stream order of kh_chain_records and kh_cigar_text, with the helpers of tests/stream_checks.py: the link rows (the runs of the
text call) are a decoy until a side stream has drained a delay and copied the real ones in, so a call whose kernels, or whose zeroing
of the output row, run on any other stream works on the decoy.  Device memory; the calls wait for their own stream once per pass; the
caller never waits.  The side stream's results equal those of the default stream and the model, and a second call gives identical bits."""
import os
import sys
from collections import namedtuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import records_model as RM  # noqa: E402
import records_cases as RC  # noqa: E402
from stream_checks import assert_busy, consume_on, late_inputs, side_stream, to_dev  # noqa: E402

Cig = namedtuple("Cig", "offsets ops")
End = namedtuple("End", "q r clip offsets ops")
OUT = "valid qs qe rs re qlen n_match n_block nm offsets ops".split()


def records(a, lk_ops, k):
    return kh.chain_records(a["qpos"], a["rpos"], a["rev"], a["chain"], Cig(a["lk_offsets"], lk_ops), a["first"], a["last"], a["q_lo"], a["q_hi"],
                            End(a["e_q"], a["e_r"], a["e_clip"], a["en_offsets"], a["en_ops"]), k, True)


def test_chain_records_reads_its_late_inputs_on_the_callers_stream():
    case = RC.cases()["three_interleaved"]
    decoy = case.a["lk_ops"] ^ np.uint32(0xF)                     # '=' becomes X and X becomes '=': other merges, other sums
    exp = case.model(1)
    wrong = RM.records(*[decoy if f == "lk_ops" else case.a[f] for f in RC.FIELDS], case.k, 1)
    assert exp["ops"] != wrong["ops"] and exp["n_match"] != wrong["n_match"]
    fixed = {f: to_dev(v) for f, v in case.a.items()}
    default = [x.cpu().numpy() for x in records(fixed, fixed["lk_ops"], case.k)]
    s = side_stream()
    try:
        with torch.cuda.stream(s):            # once before on the decoy: the scratch blocks of the real call are then at hand in the pool
            records(fixed, to_dev(decoy), case.k)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            (late,) = late_inputs(s, (case.a["lk_ops"], decoy))
            assert_busy(s)
            got = consume_on(s, *records(fixed, late, case.k))
            again = consume_on(s, *records(fixed, late, case.k))
        for name, g, d in zip(OUT, got, default):
            assert [int(v) for v in g.view(np.uint8 if name == "valid" else np.uint64 if name == "offsets" else np.uint32)] == exp[name], "side stream: %s" % name
            assert g.tobytes() == d.tobytes(), "side stream and default stream differ: %s" % name
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bits"
    finally:
        s.synchronize()


def test_cigar_text_reads_its_late_inputs_on_the_callers_stream():
    rng = np.random.RandomState(3)
    ops = rng.randint(0, 2 ** 32, size=5000, dtype=np.uint64).astype(np.uint32)
    decoy = (ops >> np.uint32(3)) | np.uint32(1 << 31)
    offs = np.arange(0, 5001, 4, dtype=np.uint64)
    eo, et = RM.cigar_text(offs, ops)
    assert RM.cigar_text(offs, decoy)[1] != et
    doffs = to_dev(offs)
    default = [x.cpu().numpy() for x in kh.cigar_text(doffs, to_dev(ops))]
    s = side_stream()
    try:
        with torch.cuda.stream(s):
            kh.cigar_text(doffs, to_dev(decoy))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            (late,) = late_inputs(s, (ops, decoy))
            assert_busy(s)
            got = consume_on(s, *kh.cigar_text(doffs, late))
            again = consume_on(s, *kh.cigar_text(doffs, late))
        assert [int(v) for v in got[0].view(np.uint64)] == eo and got[1].tobytes() == et
        assert all(g.tobytes() == d.tobytes() for g, d in zip(got, default)), "side stream and default stream differ"
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bits"
    finally:
        s.synchronize()
