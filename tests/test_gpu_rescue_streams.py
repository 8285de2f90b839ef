"""GPU: stream order of kh_mate_rescue, with the helpers of tests/stream_checks.py: the reference text is a decoy until a side stream has
drained a delay and copied the real one in, so a call whose kernels run on any other stream, or are not ordered behind the producer of
its inputs on that stream, scans the decoy.  Device memory; the call waits for its own stream once per pass (it returns a count); the
caller never waits: the results are read in the order of the caller's stream.  The side stream's results equal those of the default
stream and the model, and a second call over the same inputs gives identical bits."""
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import rescue_model as RM  # noqa: E402
from stream_checks import assert_busy, consume_on, late_inputs, side_stream, to_dev  # noqa: E402

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def make():
    rng = random.Random(3)
    ref = bytes(rng.choice(b"ACGT") for _ in range(6000))
    q, req = bytearray(), []
    for t in range(60):
        m, at = 40 + (t * 13) % 120, 50 + 95 * t
        frag = bytearray(ref[at:at + m])
        for p in range(7, m, 23):
            frag[p] = b"ACGT"[(b"ACGT".index(frag[p]) + 1) % 4]
        mate = bytes(reversed(bytes(frag).translate(COMP))) if t & 1 else bytes(frag)
        req.append((len(q), len(q) + m, at - 30, at + m + 40, t & 1))
        q += mate + b"N"
    cols = list(zip(*req))
    return (np.frombuffer(bytes(q), dtype=np.uint8).copy(), np.frombuffer(ref, dtype=np.uint8).copy(), *(np.array(c, dtype=np.uint32) for c in cols[:4]),
            np.array(cols[4], dtype=np.uint8))


def test_rescue_mates_reads_its_late_inputs_on_the_callers_stream():
    ra = make()
    decoy_ref = ra[1].copy()
    for p in range(20, len(decoy_ref), 37):                      # the decoy: the same text with a base changed every 37
        decoy_ref[p] = b"ACGT"[(b"ACGT".index(bytes(decoy_ref[p:p + 1])) + 2) % 4]
    da = (ra[0], decoy_ref) + ra[2:]
    exp, wrong = RM.rescue_model(*ra), RM.rescue_model(*da)
    assert not np.array_equal(exp[0], wrong[0]) and not np.array_equal(exp[4], wrong[4]) and len(exp[5]) > 100
    fixed = [to_dev(a) for a in ra]
    fields = lambda r: (r.edits, r.rs, r.re, r.span, r.offsets, r.ops)      # noqa: E731
    default = [x.cpu().numpy() for x in fields(kh.rescue_mates(*fixed))]      # the default stream, everything in place
    s = side_stream()
    try:
        with torch.cuda.stream(s):            # once before on the decoy: the scratch blocks of the real call are then at hand in the pool
            kh.rescue_mates(fixed[0], to_dev(da[1]), *fixed[2:])
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            (late_ref,) = late_inputs(s, (ra[1], da[1]))
            assert_busy(s)
            got = consume_on(s, *fields(kh.rescue_mates(fixed[0], late_ref, *fixed[2:])))
            again = consume_on(s, *fields(kh.rescue_mates(fixed[0], late_ref, *fixed[2:])))
        for name, g, d, e in zip(("edits", "rs", "re", "span", "offsets", "ops"), got, default, exp):
            assert np.array_equal(g.view(e.dtype), e), "side stream: %s" % name
            assert g.tobytes() == d.tobytes(), "side stream and default stream differ: %s" % name
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), "a second call gives other bits"
    finally:
        s.synchronize()
