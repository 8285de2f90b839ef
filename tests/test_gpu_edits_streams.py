"""GPU: stream order of kh_chain_edits, with the helpers of tests/stream_checks.py: the query text and the anchor positions are decoys
until a side stream has drained a delay and copied the real ones in, so a call whose kernels run on any other stream, or are not ordered
behind the producer of its inputs on that stream, verifies the decoy.  Device memory; the call returns while the delay still runs -- it
does not wait on the host -- and the results are read in the order of the caller's stream."""
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import edits_model as EM  # noqa: E402
from stream_checks import assert_busy, consume_on, late_inputs, side_stream, to_dev  # noqa: E402
from edits_cases import Batch, bases, sub  # noqa: E402


def make(seed, edits):
    B = Batch(7)                                                 # the same layout both times; the planted edits differ
    rng = random.Random(seed)
    for t in range(300):
        a = bases(B.rng, 10 + t % 40)
        b = sub(rng, a, rng.sample(range(len(a)), min(len(a), edits[t % len(edits)])))
        B.add([(a, b), (a, a)], rev=t & 1)
    return B


def test_chain_edits_reads_its_late_inputs_and_does_not_wait():
    real, decoy = make(1, [0, 1, 2, 5]), make(2, [1, 0, 3, 0])
    ra, da = real.arrays(), decoy.arrays()
    assert np.array_equal(ra[0], da[0]) and all(np.array_equal(x, y) for x, y in zip(ra[2:], da[2:])) and not np.array_equal(ra[1], da[1])
    exp, wrong = EM.chain_edits_model(*ra, real.n_chains, 15), EM.chain_edits_model(*da, decoy.n_chains, 15)
    assert not np.array_equal(exp[0], wrong[0]) and not np.array_equal(exp[1], wrong[1])
    s = side_stream()
    try:
        fixed = [to_dev(a) for a in ra]
        with torch.cuda.stream(s):            # once before on the decoy: the scratch block of the real call is then at hand in the pool
            kh.chain_edits(fixed[0], to_dev(da[1]), *fixed[2:], real.n_chains, 15)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            (late_ref,) = late_inputs(s, (ra[1], da[1]))
            assert_busy(s)
            got = kh.chain_edits(fixed[0], late_ref, *fixed[2:], real.n_chains, 15)
            assert_busy(s)                    # back while the delay still runs: the call queued its work and did not wait for the stream
            link, edits, over = consume_on(s, *got)
        assert np.array_equal(link, exp[0]), "side stream: links"
        assert np.array_equal(edits.view(np.uint32), exp[1]) and np.array_equal(over.view(np.uint32), exp[2]), "side stream: chain sums"
    finally:
        s.synchronize()
