"""GPU: kh_stamp_strand against the Python-integer model (tests/strand_model.py) on host and device memory -- every k at which the
comparison loop changes shape (1, 2, the 32 / 33 and 63 / 64 borders), mixed-case text with N and newlines, palindromic ACGT repeats,
windows X + rc(X) with one changed base next to the middle (the LAST compared pair decides), shuffled and repeated positions, the last
valid window and the one past it, 0xFFFFFFFF, out aliasing pos, pos_base, the invalid count, every refusal with the output untouched --
and kh_anchors_from_csr against np.repeat (empty first / last / consecutive rows, one row of 5 000 hits, total 0 / 1 / 257, n = 0)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
from strand_model import POS_INVALID, np_stamp, revcomp_text  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
KS = [1, 2, 15, 16, 31, 32, 33, 63, 64]
MS = [0, 1, 255, 257, 4097]


def dev(a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view is not None else a.copy()).cuda()


def host(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
    return a.view(np.uint32) if a.dtype == np.int32 else a


def near_palindrome(rng, k, which):
    """X + rc(X) (+ a middle base for odd k) with the base right behind the middle changed: all compared pairs but the last are equal"""
    x = BASES[rng.integers(0, 4, k // 2)]
    w = np.concatenate([x, BASES[rng.integers(0, 4, k % 2)], revcomp_text(x)])
    if k >= 2:
        j = (k + 1) // 2                                   # first base of the second half
        w[j] = BASES[(int(np.nonzero(BASES == w[j])[0][0]) + 1 + which) % 4]
    return w


@pytest.fixture(scope="module")
def text():
    rng = np.random.default_rng(5)
    t = BASES[rng.integers(0, 4, 5000)].copy()
    t[300:700] |= 0x20                                     # lower case
    t[1000:1400] = np.frombuffer(b"ACGT" * 100, dtype=np.uint8)          # palindromic windows for even k
    o = 1500
    for k in KS:                                           # two near-palindromes per k
        for which in (0, 1):
            t[o:o + k] = near_palindrome(rng, k, which)
            o += k + 3
    assert o < 2600
    for p in rng.integers(2600, 4900, 12):
        t[p] = ord("N")
    for p in rng.integers(2600, 4900, 4):
        t[p] = 10
    t.setflags(write=False)
    return t


def positions(text, k, m, seed):
    """m positions, shuffled, with repeats, the last valid window, the one past it, a window holding N and 0xFFFFFFFF among them"""
    rng = np.random.default_rng(seed)
    n = len(text)
    n_at = int(np.nonzero(text == ord("N"))[0][0])
    special = [n - k, n - k + 1, max(n_at - k // 2, 0), 0xFFFFFFFF, n, 0, 0, 1500]
    pos = np.concatenate([np.array(special, dtype=np.int64), np.arange(1000, 1000 + 40), np.arange(1500, 1500 + 60),
                          rng.integers(0, n - k + 1, max(m - len(special) - 100, 0))])[:m]
    return rng.permutation(pos).astype(np.uint32)


@pytest.fixture(scope="module")
def expected(text):
    """the model's answer for every (k, m), computed once"""
    out = {}
    for k in KS:
        for m in MS:
            pos = positions(text, k, m, 31 * k + m)
            out[k, m] = (pos, np_stamp(text, pos, k, 0))
    return out


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("k", KS)
def test_stamp_equals_the_model(text, expected, k, where):
    t = np.array(text) if where == "host" else dev(text)
    for m in MS:
        pos, exp = expected[k, m]
        p = pos if where == "host" else dev(pos)
        got = kh.stamp_strand(t, p, k)
        assert len(got) == m and np.array_equal(host(got), exp), (k, m)
        got2, bad = kh.stamp_strand(t, p, k, count_invalid=True)
        assert np.array_equal(host(got2), exp) and bad == int((exp == POS_INVALID).sum()), (k, m)
        if where == "device":
            assert got.is_cuda and got.dtype == torch.int32
    pos, exp = expected[k, 4097]
    bits = exp[exp != POS_INVALID] & 1
    assert (exp == POS_INVALID).sum() >= 4 and bits.any() and not bits.all()          # (the case is not vacuous)


@pytest.mark.parametrize("k", [2, 16, 32, 64])
def test_palindromes_and_the_last_compared_pair(text, k):
    pos = np.arange(1000, 1400 - k + 1, dtype=np.uint32)
    got = kh.stamp_strand(np.array(text), pos, k)
    assert np.array_equal(got, np_stamp(text, pos, k))
    pal = np.array([np.array_equal(text[p:p + k], revcomp_text(text[p:p + k])) for p in pos])
    assert pal.sum() > 50 and (got[pal] & 1 == 0).all()
    # the near-palindromes of every k: equal in all compared pairs but the one at the middle
    near, o = [], 1500
    for kk in KS:
        near += [(o, kk), (o + kk + 3, kk)]
        o += 2 * (kk + 3)
    bits = [int(kh.stamp_strand(np.array(text), np.array([p], dtype=np.uint32), kk)[0]) & 1 for p, kk in near]
    assert bits == [int(np_stamp(text, [p], kk)[0]) & 1 for p, kk in near] and 0 in bits and 1 in bits


@pytest.mark.parametrize("where", ["host", "device"])
def test_pos_base_and_out_aliasing_pos(text, expected, where):
    L = K.lib()
    for k in (15, 64):
        pos, _ = expected[k, 4097]
        exp = np_stamp(text, pos, k, 123_456)
        t = np.array(text)
        got = kh.stamp_strand(t if where == "host" else dev(t), pos if where == "host" else dev(pos), k, pos_base=123_456)
        assert np.array_equal(host(got), exp)
        # in place through the C ABI: out == pos
        if where == "host":
            buf = pos.copy()
            st = L.kh_stamp_strand(t.ctypes.data, len(t), k, buf.ctypes.data, len(buf), 123_456, K.KH_MEM_HOST, buf.ctypes.data, None, 0, None)
            assert st == K.KH_OK and np.array_equal(buf, exp)
        else:
            dt, buf = dev(t), dev(pos)
            bad = C.c_uint64()
            st = L.kh_stamp_strand(dt.data_ptr(), len(t), k, buf.data_ptr(), buf.numel(), 123_456, K.KH_MEM_DEVICE, buf.data_ptr(), C.byref(bad), 0,
                                   torch.cuda.current_stream().cuda_stream)
            assert st == K.KH_OK and np.array_equal(host(buf), exp) and bad.value == int((exp == POS_INVALID).sum())
    # the top of the coordinate space: pos_base + n == 2^31
    base = 2 ** 31 - len(text)
    pos = np.array([0, len(text) - 15], dtype=np.uint32)
    assert np.array_equal(kh.stamp_strand(np.array(text), pos, 15, pos_base=base), np_stamp(text, pos, 15, base))


@pytest.mark.parametrize("where", ["host", "device"])
def test_refusals_leave_the_output_untouched(text, where):
    L = K.lib()
    t, pos = np.array(text), np.arange(64, dtype=np.uint32)
    if where == "host":
        out = np.full(64, 9, dtype=np.uint32)
        tp, pp, op, mem = t.ctypes.data, pos.ctypes.data, out.ctypes.data, K.KH_MEM_HOST
    else:
        dt, dp, out = dev(t), dev(pos), torch.full((64,), 9, dtype=torch.int32, device="cuda")
        tp, pp, op, mem = dt.data_ptr(), dp.data_ptr(), out.data_ptr(), K.KH_MEM_DEVICE
    n = len(t)
    for args in ((tp, n, 0, pp, 64, 0), (tp, n, 65, pp, 64, 0), (tp, 1 << 31, 15, pp, 64, 0), (tp, n, 15, pp, 64, 2 ** 31 - n + 1),
                 (None, n, 15, pp, 64, 0), (tp, n, 15, None, 64, 0)):
        bad = C.c_uint64(5)
        assert L.kh_stamp_strand(*args, mem, op, C.byref(bad), 0, None) == K.KH_ERR_INVALID, args
        assert bad.value == 0
    assert L.kh_stamp_strand(tp, n, 15, pp, 64, 0, mem, None, None, 0, None) == K.KH_ERR_INVALID
    assert L.kh_stamp_strand(tp, n, 15, pp, 0, 0, mem, op, None, 0, None) == K.KH_OK            # m == 0
    torch.cuda.synchronize()
    assert (host(out) == 9).all()


# ---- kh_anchors_from_csr ---------------------------------------------------------------------------------
def csr_case(counts, seed):
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    n, total = len(counts), int(counts.sum())
    qpos = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    pos = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return qpos, offs, pos


CSR_CASES = {
    "empty_first_last_and_consecutive": [0, 0, 3, 1, 0, 0, 0, 7, 2, 0],
    "one_row_of_5000": [5000],
    "5000_between_empties": [0, 1, 5000, 0, 2],
    "total_0": [0, 0, 0],
    "total_1": [0, 1, 0],
    "total_257": [100, 0, 157],
    "n_0": [],
    "many_rows": list(np.random.default_rng(3).integers(0, 4, 3000)),
}


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("case", sorted(CSR_CASES))
def test_anchors_from_csr_is_np_repeat(case, where):
    qpos, offs, pos = csr_case(CSR_CASES[case], len(case))
    rq = np.repeat(qpos, np.diff(offs.astype(np.int64)))
    args = (qpos, offs, pos) if where == "host" else (dev(qpos), dev(offs), dev(pos))
    oq, orp, orv = kh.anchors_from_csr(*args)
    if where == "device":
        assert oq.is_cuda and orp.is_cuda and orv.is_cuda and orv.dtype == torch.uint8
    assert np.array_equal(host(oq), rq >> 1) and np.array_equal(host(orp), pos >> 1)
    assert np.array_equal(host(orv), ((rq ^ pos) & 1).astype(np.uint8)) and len(host(orv)) == len(pos)


def test_anchors_refuses_2_to_32_hits():
    a = torch.zeros(4, dtype=torch.int32, device="cuda")
    o = torch.zeros(5, dtype=torch.int64, device="cuda")
    b = torch.full((4,), 9, dtype=torch.uint8, device="cuda")
    st = K.lib().kh_anchors_from_csr(a.data_ptr(), o.data_ptr(), 4, a.data_ptr(), 1 << 32, K.KH_MEM_DEVICE, a.data_ptr(), a.data_ptr(), b.data_ptr(), 0, None)
    assert st == K.KH_ERR_INVALID and (b.cpu().numpy() == 9).all()
