"""GPU: stream order of kh_chain_ends, with the helpers of tests/stream_checks.py: the reference text is a decoy until a side stream has
drained a delay and copied the real one in, so a call whose kernels run on any other stream, or are not ordered behind the producer of
its inputs on that stream, extends against the decoy.  Device memory; the call waits for its own stream once per pass (it returns a
count); the caller never waits: the results are read in the order of the caller's stream.  The side stream's results equal those of
the default stream and the model, and a second call over the same inputs gives identical bits."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import ends_model as EM  # noqa: E402
from ends_cases import Ends, K, sub  # noqa: E402
from stream_checks import assert_busy, consume_on, late_inputs, side_stream, to_dev  # noqa: E402


def make():
    B = Ends(3, 3000)
    for t in range(60):
        B.add(100 + 45 * t, 5 + t % 30, 3 + (7 * t) % 40, t & 1, head=(lambda s: sub(s, len(s) // 2)) if t % 3 == 0 else None)
    return B


def test_chain_ends_reads_its_late_inputs_on_the_callers_stream():
    B = make()
    ra = B.arrays()
    decoy_ref = ra[1].copy()
    for p in range(20, len(decoy_ref), 37):                      # the decoy: the same text with a base changed every 37
        decoy_ref[p] = sub(bytes(decoy_ref[p:p + 1]), 0)[0]
    da = (ra[0], decoy_ref) + ra[2:]
    exp, wrong = EM.chain_ends_model(*ra, K), EM.chain_ends_model(*da, K)
    assert not np.array_equal(exp[0], wrong[0]) and not np.array_equal(exp[4], wrong[4]) and len(exp[5]) > 100
    fixed = [to_dev(a) for a in ra]
    default = [x.cpu().numpy() for x in kh.chain_ends(*fixed, K)]      # the default stream, everything in place
    s = side_stream()
    try:
        with torch.cuda.stream(s):            # once before on the decoy: the scratch blocks of the real call are then at hand in the pool
            kh.chain_ends(fixed[0], to_dev(da[1]), *fixed[2:], K)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            (late_ref,) = late_inputs(s, (ra[1], da[1]))
            assert_busy(s)
            got = consume_on(s, *kh.chain_ends(fixed[0], late_ref, *fixed[2:], K))
            again = consume_on(s, *kh.chain_ends(fixed[0], late_ref, *fixed[2:], K))
        for name, g, d, e in zip(("q", "r", "edits", "clip", "offsets", "ops"), got, default, exp):
            assert np.array_equal(g.view(e.dtype), e), "side stream: %s" % name
            assert g.tobytes() == d.tobytes(), "side stream and default stream differ: %s" % name
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bits"
    finally:
        s.synchronize()
