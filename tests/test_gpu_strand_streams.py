"""GPU: stream order of the strand entry points, with the helpers of tests/stream_checks.py: the input of each call is a decoy until a
side stream has drained a delay, so a call issued on any other stream, or not ordered behind its input, stamps the decoy text.
stamp_strand over device input (queued only: its result is read in the order of the caller's stream), a stranded build_sequences from a
device text, and anchors() of a device query."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from index_model import IndexModel  # noqa: E402
from stream_checks import assert_busy, consume_on, late_input, late_inputs, side_stream, to_dev  # noqa: E402
from strand_model import np_stamp, revcomp_text  # noqa: E402
from syncmer_model import np_syncmers  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
K, S = 15, 11


def random_text(n, seed):
    return BASES[np.random.default_rng(seed).integers(0, 4, n)].copy()


TEXT, TEXT_DECOY = random_text(6000, 1), random_text(6000, 2)


@pytest.fixture()
def s():
    st = side_stream()
    yield st
    st.synchronize()


def rehearse(stream, call):
    """the call once before under the same stream on decoys, so that the allocations of the real call are served from memory at hand"""
    with torch.cuda.stream(stream):
        call()
    torch.cuda.synchronize()


def u32(t):
    return np.ascontiguousarray(t).view(np.uint32)


def test_stamp_strand_reads_its_late_text_and_positions(s):
    rng = np.random.default_rng(3)
    pos = rng.integers(0, len(TEXT) - K + 1, 4000).astype(np.uint32)
    pos_decoy = rng.integers(0, len(TEXT) - K + 1, 4000).astype(np.uint32)
    exp = np_stamp(TEXT, pos, K, 100)
    assert not np.array_equal(exp, np_stamp(TEXT_DECOY, pos, K, 100)) and not np.array_equal(exp, np_stamp(TEXT, pos_decoy, K, 100))
    rehearse(s, lambda: kh.stamp_strand(to_dev(TEXT_DECOY), to_dev(pos_decoy), K, 100))
    with torch.cuda.stream(s):
        bt, bp = late_inputs(s, (TEXT, TEXT_DECOY), (pos, pos_decoy))
        assert_busy(s)
        got = consume_on(s, kh.stamp_strand(bt, bp, K, 100))
    assert np.array_equal(u32(got), exp)
    # with the count: the call waits for its own stream
    with torch.cuda.stream(s):
        bt, bp = late_inputs(s, (TEXT, TEXT_DECOY), (pos, pos_decoy))
        assert_busy(s)
        out, bad = kh.stamp_strand(bt, bp, K, 100, count_invalid=True)
    assert bad == 0 and np.array_equal(u32(out.cpu().numpy()), exp)


def test_stranded_build_sequences_from_a_late_device_text(s):
    km, pos = np_syncmers(TEXT, K, S, True, "murmur", 42)
    model = IndexModel(km, np_stamp(TEXT, pos, K))
    twin = kh.KmerPositionIndex(k=K, s=S, stranded=True)
    rehearse(s, lambda: twin.build_sequences(to_dev(TEXT_DECOY)))
    twin.close()
    ix = kh.KmerPositionIndex(k=K, s=S, stranded=True)
    try:
        with torch.cuda.stream(s):
            bt = late_input(s, TEXT, TEXT_DECOY)
            assert_busy(s)
            assert ix.build_sequences(bt) == len(pos)
        keys, offs, stamped = ix.export()
        eo, ep = model.export_in_key_order(keys)
        assert np.array_equal(offs, eo) and np.array_equal(stamped, ep)
    finally:
        ix.close()


def test_anchors_of_a_late_device_query(s):
    query = np.concatenate([TEXT[1000:1600], revcomp_text(TEXT[3000:3600])])
    decoy = np.concatenate([TEXT[2000:2600], revcomp_text(TEXT[4000:4600])])
    ix = kh.KmerPositionIndex(k=K, s=S, stranded=True)
    try:
        ix.build_sequences(TEXT)
        exp = ix.anchors(query)                              # host path, null stream (pinned against the model in test_gpu_strand_index.py)
        assert len(exp[0]) > 100 and (exp[2] == 0).any() and (exp[2] == 1).any()
        wrong = ix.anchors(decoy)
        assert not (len(wrong[1]) == len(exp[1]) and np.array_equal(wrong[1], exp[1]))
        rehearse(s, lambda: ix.anchors(to_dev(decoy)))
        with torch.cuda.stream(s):
            bq = late_input(s, query, decoy)
            assert_busy(s)
            qpos, rpos, rev = consume_on(s, *ix.anchors(bq))
        assert np.array_equal(u32(qpos), exp[0]) and np.array_equal(u32(rpos), exp[1]) and np.array_equal(rev, exp[2])
    finally:
        ix.close()
