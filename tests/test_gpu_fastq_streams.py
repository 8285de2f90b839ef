"""GPU: stream order of kh_fastq_records, kh_pack_rows and read_fastq, with the helpers of tests/stream_checks.py: the text is a
decoy -- the same bytes rotated by one, so every line starts elsewhere -- until a side stream has drained a delay and copied the real
one in, so a call whose kernels run on any other stream works on the decoy.  Device memory.  fastq_records and read_fastq wait for their
own stream (once per pass; once more for the totals); pack_rows returns no count and never waits: the delay on the side stream is
still running AFTER it has returned.  The side stream's results equal those of the default stream and the model, and a second call
gives identical bits."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import fastq_cases as FC  # noqa: E402
import fastq_model as FM  # noqa: E402
from stream_checks import assert_busy, consume_on, late_inputs, side_stream, to_dev  # noqa: E402

RAW = FC.CASES["many"].text
REAL = np.frombuffer(RAW, dtype=np.uint8)
DECOY = np.roll(REAL, 1)


def columns(r):
    return [x for x in r if isinstance(x, torch.Tensor)]


def test_fastq_records_reads_its_late_text_on_the_callers_stream():
    rows = FM.fastq_records(RAW)[0]
    assert FM.fastq_records(DECOY.tobytes())[0] != rows
    default = [x.cpu().numpy() for x in columns(kh.fastq_records(to_dev(REAL)))]
    s = side_stream()
    try:
        with torch.cuda.stream(s):            # once before on the decoy: the scratch blocks of the real call are then at hand in the pool
            kh.fastq_records(to_dev(DECOY))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            (late,) = late_inputs(s, (REAL, DECOY))
            assert_busy(s)
            got = consume_on(s, *columns(kh.fastq_records(late)))
            again = consume_on(s, *columns(kh.fastq_records(late)))
        assert list(zip(*(g.view(np.uint32 if g.dtype == np.int32 else g.dtype).tolist() for g in got))) == rows
        assert all(g.tobytes() == d.tobytes() for g, d in zip(got, default)), "side stream and default stream differ"
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bits"
    finally:
        s.synchronize()


def test_pack_rows_reads_its_late_text_on_the_callers_stream_and_does_not_wait():
    rows = FM.fastq_records(RAW)[0]
    lo, hi = (np.array([r[i] for r in rows], dtype=np.uint32) for i in (2, 3))
    dst = np.concatenate([[0], np.cumsum(hi.astype(np.int64) - lo + 1)]).astype(np.uint64)
    out_len = int(dst[-1])
    want = FM.read_fastq([RAW])["seq"]
    assert bytes(FM.pack_rows(DECOY.tobytes(), lo.tolist(), hi.tolist(), dst[:-1].tolist(), 10, bytearray(out_len))) != want
    dlo, dhi, ddst = to_dev(lo), to_dev(hi), to_dev(dst[:-1])
    call = lambda text: kh.pack_rows(text, dlo, dhi, ddst, out_len, sep=10)      # noqa: E731
    default = call(to_dev(REAL)).cpu().numpy()
    s = side_stream()
    try:
        with torch.cuda.stream(s):
            call(to_dev(DECOY))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            (late,) = late_inputs(s, (REAL, DECOY))
            assert_busy(s)
            res = call(late)
            assert_busy(s)                    # the call has returned and the delay still runs: it did not wait for its stream
            res2 = call(late)
            assert_busy(s)
            got, again = consume_on(s, res), consume_on(s, res2)
        assert got.tobytes() == want and got.tobytes() == default.tobytes() and got.tobytes() == again.tobytes()
    finally:
        s.synchronize()


def test_read_fastq_reads_its_late_text_on_the_callers_stream():
    want = FM.read_fastq([RAW])
    flat = lambda r: [r.seq, r.qual, r.read_starts, r.read_ends, r.names[0], r.names[1], r.status]      # noqa: E731
    default = [x.cpu().numpy() for x in flat(kh.read_fastq(to_dev(REAL)))]
    s = side_stream()
    try:
        with torch.cuda.stream(s):
            kh.read_fastq(to_dev(DECOY), strict=False)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            (late,) = late_inputs(s, (REAL, DECOY))
            assert_busy(s)
            got = consume_on(s, *flat(kh.read_fastq(late)))
            again = consume_on(s, *flat(kh.read_fastq(late)))
        assert got[0].tobytes() == want["seq"] and got[1].tobytes() == want["qual"] and got[2].tolist() == want["read_starts"] and got[5].tobytes() == want["names"][1]
        assert all(g.tobytes() == d.tobytes() for g, d in zip(got, default)), "side stream and default stream differ"
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bits"
    finally:
        s.synchronize()
