"""GPU: stream order of kh_chain_anchors, with the helpers of tests/stream_checks.py: the anchors are a decoy until a side stream has
drained a delay and copied the real ones in, so a call whose kernels run on any other stream, or are not ordered behind the producer of
the anchors on that stream, chains the decoy.  Device memory; the results are read in the order of the caller's stream."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import chain_model as CM  # noqa: E402
from chain_cases import arrays, assert_same, segment_list  # noqa: E402
from stream_checks import assert_busy, consume_on, late_inputs, side_stream, to_dev  # noqa: E402


def test_chain_anchors_reads_its_late_anchors():
    lengths = [130, 0, 64, 200, 65]
    q, r, v, seg = segment_list(np.random.default_rng(1), lengths, noise=0.1)
    dq, dr, dv, _ = segment_list(np.random.default_rng(2), lengths, noise=0.1)
    params = dict(max_gap=300, band=60, min_score=30, min_count=2)
    exp, wrong = CM.chain(q, r, v, 15, seg, **params), CM.chain(dq, dr, dv, 15, seg, **params)
    assert len(exp.first) >= 4 and not np.array_equal(exp.score, wrong.score)
    (aq, ar, av, aseg), (bq, br, bv, _) = arrays(q, r, v, seg), arrays(dq, dr, dv, seg)
    s = side_stream()
    try:
        dseg = to_dev(aseg)
        with torch.cuda.stream(s):            # once before on the decoys: the allocations of the real call are then served from memory at hand
            kh.chain_anchors(to_dev(bq), to_dev(br), to_dev(bv), 15, dseg, **params)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            lq, lr, lv = late_inputs(s, (aq, bq), (ar, br), (av, bv))
            assert_busy(s)
            got = kh.chain_anchors(lq, lr, lv, 15, dseg, **params)      # (waits for its own stream: the count of the chains)
            got = type(got)(*consume_on(s, *got))
        assert_same(got, exp, "side stream")
    finally:
        s.synchronize()
