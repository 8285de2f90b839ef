"""GPU: stream order of kh_pair_chains, with the helpers of tests/stream_checks.py: the scores are a decoy until a side stream has
drained a delay and copied the real ones in, so a call whose kernel runs on any other stream, or is not ordered behind the producer of
its inputs on that stream, pairs the decoy.  Device memory.  The call returns no count and therefore never waits: the delay on the side
stream is still running AFTER pair_chains has returned.  The side stream's results equal those of the default stream and the model, and
a second call over the same inputs gives identical bits."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from pair_cases import random_table  # noqa: E402
from pair_model import NAMES, pair_model  # noqa: E402
from stream_checks import assert_busy, consume_on, late_inputs, side_stream, to_dev  # noqa: E402


def test_pair_chains_reads_its_late_inputs_on_the_callers_stream_and_does_not_wait():
    a = random_table(n_pairs=300, seed=9)
    params = dict(min_ins=a.pop("min_ins"), max_ins=a.pop("max_ins"), unpaired_pen=a.pop("unpaired_pen"))
    order = ("rs", "re", "rev", "score", "read_offsets", "tid", "use", "mapq")
    decoy = a["score"][::-1].copy()
    exp = pair_model(*(a[k] for k in order), **params)
    wrong = pair_model(*(decoy if k == "score" else a[k] for k in order), **params)
    assert not np.array_equal(exp[0], wrong[0]) and not np.array_equal(exp[1], wrong[1]) and not np.array_equal(exp[4], wrong[4])
    fixed = {k: to_dev(a[k]) for k in order}
    call = lambda score: kh.pair_chains(*(score if k == "score" else fixed[k] for k in order), **params)      # noqa: E731
    default = [x.cpu().numpy() for x in call(fixed["score"])]      # the default stream, everything in place
    s = side_stream()
    try:
        with torch.cuda.stream(s):
            dd = to_dev(decoy)
            call(dd)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            (late_score,) = late_inputs(s, (a["score"], decoy))
            assert_busy(s)
            res = call(late_score)
            assert_busy(s)                    # the call has returned and the delay still runs: it did not wait for its stream
            res2 = call(late_score)
            assert_busy(s)
            got, again = consume_on(s, *res), consume_on(s, *res2)
        for name, g, d, e in zip(NAMES, got, default, exp):
            assert np.array_equal(g.view(e.dtype), e), "side stream: %s" % name
            assert g.tobytes() == d.tobytes(), "side stream and default stream differ: %s" % name
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bits"
    finally:
        s.synchronize()
