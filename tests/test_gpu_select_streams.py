"""GPU: stream order of kh_chain_select, with the helpers of tests/stream_checks.py: the scores are a decoy until a side stream has
drained a delay and copied the real ones in, so a call whose kernels run on any other stream, or are not ordered behind the producer of
its inputs on that stream, ranks the decoy.  Device memory.  The call returns no count and therefore never waits: the delay on the side
stream is still running AFTER select_chains has returned -- the chain calls that wait once per pass cannot pass that assertion.  The
side stream's results equal those of the default stream and the model, and a second call over the same inputs gives identical bits."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import select_cases as SC  # noqa: E402
from select_model import NAMES, select_model  # noqa: E402
from stream_checks import assert_busy, consume_on, late_inputs, side_stream, to_dev  # noqa: E402


def test_select_chains_reads_its_late_inputs_on_the_callers_stream_and_does_not_wait():
    qs, qe, sc, cnt, offs = SC.batch((0, 3, 64, 65, 200, 2100, 0), "ties", "random", seed=21)      # both kernels, both sorts
    decoy = sc[::-1].copy()
    exp, wrong = select_model(qs, qe, sc, cnt, offs), select_model(qs, qe, decoy, cnt, offs)
    assert not np.array_equal(exp[0], wrong[0]) and not np.array_equal(exp[2], wrong[2]) and not np.array_equal(exp[6], wrong[6])
    fixed = [to_dev(a) for a in (qs, qe, sc, cnt, offs)]
    default = [x.cpu().numpy() for x in kh.select_chains(*fixed)]      # the default stream, everything in place
    s = side_stream()
    try:
        with torch.cuda.stream(s):            # twice before on the decoy: the scratch blocks of the two real calls are then at hand in the pool
            dd = to_dev(decoy)
            kh.select_chains(fixed[0], fixed[1], dd, fixed[3], fixed[4])
            kh.select_chains(fixed[0], fixed[1], dd, fixed[3], fixed[4])
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            (late_score,) = late_inputs(s, (sc, decoy))
            assert_busy(s)
            res = kh.select_chains(fixed[0], fixed[1], late_score, fixed[3], fixed[4])
            assert_busy(s)                    # the call has returned and the delay still runs: it did not wait for its stream
            res2 = kh.select_chains(fixed[0], fixed[1], late_score, fixed[3], fixed[4])
            assert_busy(s)
            got, again = consume_on(s, *res), consume_on(s, *res2)
        for name, g, d, e in zip(NAMES, got, default, exp):
            assert np.array_equal(g.view(e.dtype), e), "side stream: %s" % name
            assert g.tobytes() == d.tobytes(), "side stream and default stream differ: %s" % name
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bits"
    finally:
        s.synchronize()
