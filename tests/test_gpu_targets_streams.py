"""GPU: stream order of kh_anchor_targets, with the helpers of tests/stream_checks.py: rpos is a decoy until a side stream has drained
a delay and copied the real positions in, so a call whose kernels run on any other stream groups the anchors by the decoy's targets.
Device memory; the call waits for its own stream once; the caller never waits.  The side stream's results equal those of the default
stream and the model, and a second call gives identical bytes."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import targets_cases as TC  # noqa: E402
from stream_checks import assert_busy, consume_on, late_inputs, side_stream, to_dev  # noqa: E402

OUT = (("qpos", "q", np.uint32), ("rpos", "r", np.uint32), ("rev", "v", np.uint8), ("tid", "tid", np.uint32), ("src", "src", np.uint32),
       ("offsets", "g_off", np.uint64), ("seg", "g_seg", np.uint32), ("target", "g_tid", np.uint32))


def test_group_anchors_reads_its_late_input_on_the_callers_stream():
    case = TC.batch(65, 15, 21)
    decoy = case.rpos[::-1].copy()                                # the same positions on other anchors: other groups
    exp, wrong = case.model(), case._replace(rpos=decoy).model()
    assert exp["src"] != wrong["src"] and exp["g_off"] != wrong["g_off"]
    q, v, seg, tab = to_dev(case.qpos), to_dev(case.rev), to_dev(case.seg), (to_dev(case.t_start), to_dev(case.t_end))
    default = [x.cpu().numpy() for x in kh.group_anchors(q, to_dev(case.rpos), v, tab, case.k, seg)]
    s = side_stream()
    try:
        with torch.cuda.stream(s):            # once before on the decoy: the scratch block of the real call is then at hand in the pool
            kh.group_anchors(q, to_dev(decoy), v, tab, case.k, seg)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            (late,) = late_inputs(s, (case.rpos, decoy))
            assert_busy(s)
            got = consume_on(s, *kh.group_anchors(q, late, v, tab, case.k, seg))
            again = consume_on(s, *kh.group_anchors(q, late, v, tab, case.k, seg))
        for (name, mf, dt), g, d in zip(OUT, got, default):
            assert g.view(dt).tolist() == exp[mf], "side stream: %s" % name
            assert g.tobytes() == d.tobytes(), "side stream and default stream differ: %s" % name
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bytes"
    finally:
        s.synchronize()
