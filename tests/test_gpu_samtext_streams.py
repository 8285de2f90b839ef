"""GPU: stream order of kh_sam_lines, with the helpers of tests/stream_checks.py: the SEQ text and the FLAG column are decoys until a
side stream has drained a delay and copied the real ones in, and so are the SEQ offsets, on which the lengths of the lines depend -- so
a call whose count pass, scan or emit pass runs on any other stream works on a decoy.  Device memory; the call waits for its own stream
once per pass; the caller never waits.  The side stream's result equals that of the default stream and the model, and a second call
gives identical bits."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import samtext_cases as SC  # noqa: E402
import samtext_model as SM  # noqa: E402
from stream_checks import assert_busy, consume_on, late_inputs, side_stream, to_dev  # noqa: E402


def test_sam_lines_reads_its_late_inputs_on_the_callers_stream():
    csrs, cols = SC.lines(257, 31)
    h = lambda pair: ([int(x) for x in pair[0]], pair[1].tobytes())      # noqa: E731
    model = lambda seq_off, seq_text, flag: SM.sam_lines(*(h((seq_off, seq_text)) if x == "seq" else h(csrs[x]) for x in SC.CSRS), dict(cols, flag=flag))  # noqa: E731
    seq_off, seq_text = csrs["seq"]
    decoy_off = np.minimum(seq_off, seq_off[5]).astype(np.uint64)      # rows beyond the fifth are empty: other line lengths
    decoy_text = np.roll(seq_text, 1)
    decoy_flag = (cols["flag"] ^ np.uint32(0x10)).astype(np.uint32)
    eo, et = model(seq_off, seq_text, cols["flag"])
    assert model(decoy_off, seq_text, cols["flag"])[0] != eo and model(seq_off, decoy_text, cols["flag"])[1] != et and model(seq_off, seq_text, decoy_flag)[1] != et
    d = {x: tuple(to_dev(a) for a in csrs[x]) for x in SC.CSRS}
    dc = {c: to_dev(cols[c]) for c in SC.COLUMNS}
    call = lambda so, st, fl: kh.sam_lines_text(*((so, st) if x == "seq" else d[x] for x in SC.CSRS), [fl if c == "flag" else dc[c] for c in SC.COLUMNS])  # noqa: E731
    default = [x.cpu().numpy() for x in call(d["seq"][0], d["seq"][1], dc["flag"])]
    s = side_stream()
    try:
        with torch.cuda.stream(s):            # once before on the decoys: the scratch blocks of the real call are then at hand in the pool
            call(to_dev(decoy_off), to_dev(decoy_text), to_dev(decoy_flag))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            late_off, late_text, late_flag = late_inputs(s, (seq_off, decoy_off), (seq_text, decoy_text), (cols["flag"], decoy_flag))
            assert_busy(s)
            got = consume_on(s, *call(late_off, late_text, late_flag))
            again = consume_on(s, *call(late_off, late_text, late_flag))
        assert [int(v) for v in got[0].view(np.uint64)] == eo and got[1].tobytes() == et
        assert all(g.tobytes() == x.tobytes() for g, x in zip(got, default)), "side stream and default stream differ"
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bits"
    finally:
        s.synchronize()
