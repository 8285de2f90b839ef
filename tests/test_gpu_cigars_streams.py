"""GPU: stream order of kh_chain_cigars, with the helpers of tests/stream_checks.py: the reference text is a decoy until a side stream has
drained a delay and copied the real one in, so a call whose kernels run on any other stream, or are not ordered behind the producer of
its inputs on that stream, aligns the decoy.  Device memory; the call waits for its own stream once per pass (it returns a count), so
unlike kh_chain_edits it is not back before the delay ends; the results are read in the order of the caller's stream.  A second call over
the same inputs gives identical bits."""
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import cigar_model as CM  # noqa: E402
import edits_model as EM  # noqa: E402
from stream_checks import assert_busy, consume_on, late_inputs, side_stream, to_dev  # noqa: E402
from edits_cases import Batch, bases, sub  # noqa: E402


def make(seed, edits):
    B = Batch(7)                                                 # the same layout both times; the planted edits differ
    rng = random.Random(seed)
    for t in range(100):
        a = bases(B.rng, 10 + t % 40)
        b = sub(rng, a, rng.sample(range(len(a)), min(len(a), edits[t % len(edits)])))
        B.add([(a, b), (a, a)], rev=t & 1)
    return B


def test_chain_cigars_reads_its_late_inputs_on_the_callers_stream():
    real, decoy = make(1, [0, 1, 2, 5]), make(2, [1, 0, 3, 0])
    ra, da = real.arrays(), decoy.arrays()
    assert np.array_equal(ra[0], da[0]) and all(np.array_equal(x, y) for x, y in zip(ra[2:], da[2:])) and not np.array_equal(ra[1], da[1])
    # one link array for both: 5 everywhere a link exists, so that the rows depend on the text alone
    link = np.where(EM.chain_edits_model(*ra, real.n_chains, 15)[0] >= 0, 5, -1).astype(np.int32)
    exp, wrong = CM.chain_cigars_model(*ra, real.n_chains, 15, link), CM.chain_cigars_model(*da, decoy.n_chains, 15, link)
    assert not np.array_equal(exp[0], wrong[0]) and len(exp[1]) > 100
    s = side_stream()
    try:
        fixed = [to_dev(a) for a in ra]
        dlink = to_dev(link)
        with torch.cuda.stream(s):            # once before on the decoy: the scratch blocks of the real call are then at hand in the pool
            kh.chain_cigars(fixed[0], to_dev(da[1]), *fixed[2:], real.n_chains, 15, dlink)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            (late_ref,) = late_inputs(s, (ra[1], da[1]))
            assert_busy(s)
            got = kh.chain_cigars(fixed[0], late_ref, *fixed[2:], real.n_chains, 15, dlink)
            offsets, ops, ins, dels = consume_on(s, *got)
            again = consume_on(s, *kh.chain_cigars(fixed[0], late_ref, *fixed[2:], real.n_chains, 15, dlink))
        assert np.array_equal(offsets.view(np.uint64), exp[0]), "side stream: offsets"
        assert np.array_equal(ops.view(np.uint32), exp[1]), "side stream: ops"
        assert np.array_equal(ins.view(np.uint32), exp[2]) and np.array_equal(dels.view(np.uint32), exp[3]), "side stream: chain sums"
        assert all(x.tobytes() == y.tobytes() for x, y in zip((offsets, ops, ins, dels), again)), "a second call gives other bits"
    finally:
        s.synchronize()
