"""GPU: kh_csr_unpermute against the numpy model of tests/csr_model.py, bit for bit.  The shapes follow the scan tile of the index
(2 048 entries) and the span of one workgroup of the move (256 output elements): one entry past a tile, several tiles and a ragged
tail, a segment longer than a workgroup's span, a segment that is the whole output, and the degenerate batches."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from csr_model import np_csr_unpermute  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402

SENTINEL = 0x5A5A5A5A


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype).view({4: np.int32, 8: np.int64}[np.dtype(dtype).itemsize]).copy()).cuda()


def unpermute(counts_perm, pos_perm, origin, counts=True, offsets=True, positions=True, cap=None, inputs=None):
    """-> (status, n_out, counts | None, offsets | None, positions buffer | None) as numpy arrays
    inputs: the three device buffers to pass instead of copies of the arrays (which then only give the sizes)"""
    n, total = len(counts_perm), len(pos_perm)
    cap = total if cap is None else cap
    dc, dp, do = inputs if inputs is not None else (dev(counts_perm, np.uint32), dev(pos_perm, np.uint32), dev(origin, np.uint32))
    oc = torch.full((max(n, 1),), SENTINEL, dtype=torch.int32, device="cuda") if counts else None
    oo = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda") if offsets else None
    op = torch.full((max(cap, 1),), SENTINEL, dtype=torch.int32, device="cuda") if positions else None
    n_out = C.c_uint64(12345)
    st = K.lib().kh_csr_unpermute(dc.data_ptr(), dp.data_ptr(), do.data_ptr(), n, oc.data_ptr() if counts else None,
                                  oo.data_ptr() if offsets else None, op.data_ptr() if positions else None, cap, C.byref(n_out), 0,
                                  torch.cuda.current_stream(0).cuda_stream)
    torch.cuda.synchronize()
    back = lambda t, dt: None if t is None else t.cpu().numpy().view(dt)
    return st, n_out.value, back(oc, np.uint32), back(oo, np.uint64), back(op, np.uint32)


def check(counts_perm, origin, **kw):
    counts_perm = np.asarray(counts_perm, dtype=np.uint32)
    total = int(counts_perm.sum())
    pos_perm = np.random.default_rng(total + len(counts_perm)).integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)
    ec, eo, ep = np_csr_unpermute(counts_perm, pos_perm, origin)
    st, n_out, c, o, p = unpermute(counts_perm, pos_perm, origin, **kw)
    assert st == K.KH_OK and n_out == total
    if c is not None:
        assert np.array_equal(c[: len(ec)], ec)
    if o is not None:
        assert np.array_equal(o, eo)
    if p is not None:
        assert np.array_equal(p[:total], ep) and (p[total:] == SENTINEL).all()
    return ec, eo, ep


def test_empty_batch():
    st, n_out, _, o, p = unpermute(np.zeros(0), np.zeros(0), np.zeros(0))
    assert st == K.KH_OK and n_out == 0 and o.tolist() == [0] and p.tolist() == [SENTINEL]


@pytest.mark.parametrize("hits", [0, 5000])       # 5 000: longer than one workgroup's span of the move
def test_one_query(hits):
    check([hits], [0])


@pytest.mark.parametrize("n", [2049, 5000])       # one entry past a scan tile; several tiles and a ragged tail
@pytest.mark.parametrize("order", ["random", "identity", "reversed"])
def test_scan_tiles(n, order):
    rng = np.random.default_rng(n)
    counts = rng.integers(0, 6, n)
    counts[rng.integers(0, n, 3)] = 700           # a few segments longer than a workgroup's span
    origin = {"random": rng.permutation(n), "identity": np.arange(n), "reversed": np.arange(n)[::-1]}[order]
    ec, _, _ = check(counts, origin)
    assert (ec == 0).any() and (ec == 700).any()


def test_all_counts_zero():
    ec, eo, ep = check(np.zeros(5000), np.random.default_rng(1).permutation(5000))
    assert eo[-1] == 0 and len(ep) == 0


def test_one_query_holds_everything():
    counts = np.zeros(5000, dtype=np.uint32)
    counts[1234] = 100_000
    check(counts, np.random.default_rng(2).permutation(5000))


@pytest.mark.parametrize("skip", ["counts", "offsets", "positions"])
def test_each_output_may_be_null(skip):
    rng = np.random.default_rng(3)
    check(rng.integers(0, 9, 5000), rng.permutation(5000), **{skip: False})


def test_cap_out_one_too_small():
    rng = np.random.default_rng(4)
    counts, origin = rng.integers(0, 9, 2049).astype(np.uint32), rng.permutation(2049)
    total = int(counts.sum())
    pos = rng.integers(0, 1 << 31, total).astype(np.uint32)
    ec, eo, _ = np_csr_unpermute(counts, pos, origin)
    st, n_out, c, o, p = unpermute(counts, pos, origin, cap=total - 1)
    assert st == K.KH_ERR_INVALID and n_out == total
    assert np.array_equal(o, eo) and np.array_equal(c, ec)
    assert (p == SENTINEL).all()


def test_on_a_non_default_stream():
    """the inputs arrive late on the side stream (stream_checks.late_inputs: until a delay on that stream has run the buffers hold a
    decoy -- the same counts rotated, so the same total, another permutation, other positions) and the stream is still busy when the
    call is made: a call that ran on another stream would unpermute the decoy"""
    from stream_checks import assert_busy, late_inputs, side_stream
    s = side_stream()
    rng = np.random.default_rng(5)
    counts, origin = rng.integers(0, 9, 5000).astype(np.uint32), rng.permutation(5000).astype(np.uint32)
    total = int(counts.sum())
    pos = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)
    decoys = np.roll(counts, 1), (pos ^ np.uint32(0x0F0F0F0F)).astype(np.uint32), rng.permutation(5000).astype(np.uint32)
    ec, eo, ep = np_csr_unpermute(counts, pos, origin)
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream(0).cuda_stream == s.cuda_stream != torch.cuda.default_stream(0).cuda_stream
        bufs = late_inputs(s, (counts, decoys[0]), (pos, decoys[1]), (origin, decoys[2]))
        assert_busy(s)
        st, n_out, c, o, p = unpermute(counts, pos, origin, inputs=bufs)
    assert st == K.KH_OK and n_out == total
    assert np.array_equal(c, ec) and np.array_equal(o, eo) and np.array_equal(p[:total], ep)
