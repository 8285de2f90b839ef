"""GPU: every handle-free entry that takes `where` gives byte-identical outputs and counts for host memory and for device memory, at the
element counts where the 256-byte boundaries of the call's scratch layout move (1, 63, 64, 65, 255, 256, 257; odd totals for the 4-byte
arrays), and kh_csr_unpermute (device memory only) agrees with tests/csr_model.py at the same sizes with each optional output null in
turn.  Every output sits between guard words, which come back unchanged.  The model tests remain the judge of what the right answer
is: a host call runs on staged copies carved from one block, a device call on the caller's arrays, so one array carved over another
shows as a difference between the two."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from chain_cases import segment_list  # noqa: E402
from csr_model import np_csr_unpermute  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
from kmerhash_amd.kmers import synthetic_fastq  # noqa: E402
from kmerhash_amd.table import _hash_id  # noqa: E402

SIZES = [1, 63, 64, 65, 255, 256, 257]
GUARD, FILL, PAD = 0xA5, 0x5A, 256      # guard byte, what an output holds before the call, guard bytes on either side
HOST, DEVICE = K.KH_MEM_HOST, K.KH_MEM_DEVICE
MURMUR = _hash_id("murmur3avx64")


class Out:
    """an output of `count` elements of `dtype` between two guard bands, in host or in device memory"""

    def __init__(self, count, dtype, where):
        self.dtype, self.nbytes, self.where = np.dtype(dtype), int(count) * np.dtype(dtype).itemsize, where
        raw = np.full(self.nbytes + 2 * PAD, GUARD, dtype=np.uint8)
        raw[PAD: PAD + self.nbytes] = FILL
        self.buf = torch.from_numpy(raw).cuda() if where == DEVICE else raw
        base = self.buf.data_ptr() if where == DEVICE else self.buf.ctypes.data
        assert base % 16 == 0
        self.ptr = base + PAD

    def get(self, count=None):
        """the first `count` elements (all of them by default); the guards and what lies behind `count` must be untouched"""
        raw = self.buf.cpu().numpy() if self.where == DEVICE else self.buf
        assert (raw[:PAD] == GUARD).all() and (raw[PAD + self.nbytes:] == GUARD).all(), "guard words overwritten"
        used = self.nbytes if count is None else int(count) * self.dtype.itemsize
        assert (raw[PAD + used: PAD + self.nbytes] == FILL).all(), "written behind the count"
        return raw[PAD: PAD + used].copy().view(self.dtype)


class In:
    """a numpy input in host memory, or its copy in device memory"""

    def __init__(self, a, where):
        self.a = np.ascontiguousarray(a)
        self.t = torch.from_numpy(self.a.view(np.uint8).reshape(-1).copy()).cuda() if where == DEVICE else None
        self.ptr = (self.t.data_ptr() if self.t.numel() else None) if where == DEVICE else (self.a.ctypes.data if self.a.size else None)


def stream(where):
    return torch.cuda.current_stream(0).cuda_stream if where == DEVICE else None


def both(run):
    """run(where) -> list of numpy arrays / numbers; the host call and the device call must agree byte for byte"""
    h, d = run(HOST), run(DEVICE)
    assert len(h) == len(d)
    for i, (a, b) in enumerate(zip(h, d)):
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), "output %d differs between host and device memory" % i
        else:
            assert a == b, "result %d differs between host and device memory: %r, %r" % (i, a, b)
    return h


def text_of(n, seed):
    """n bytes of bases with a few bytes that are none and a few line ends"""
    rng = np.random.default_rng(seed)
    t = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]
    t[rng.random(n) < 0.03] = ord("N")
    t[rng.random(n) < 0.02] = 10
    return t


FASTQ = np.frombuffer(synthetic_fastq(5, read_len=47, genome_len=500, seed=3), dtype=np.uint8)


def k_for(n, k):
    return max(1, min(n, k))


# ---- k-mers, with and without positions, both widths ----------------------------------------------------------------------------------
def run_kmers(text, words, k, fastq, with_pos):
    name = "kh_kmers%s_from_%s%s" % ("128" if words == 2 else "", "fastq" if fastq else "sequence", "_pos" if with_pos else "")

    def run(where):
        n = len(text)
        tin, okm, n_out = In(text, where), Out(n * words, np.uint64, where), C.c_uint64(777)
        opos = Out(n, np.uint32, where) if with_pos else None
        args = [tin.ptr, n, k, 1, where, okm.ptr] + ([opos.ptr] if with_pos else []) + [C.byref(n_out), 0, stream(where)]
        assert getattr(K.lib(), name)(*args) == K.KH_OK
        torch.cuda.synchronize()
        return [n_out.value, okm.get(n_out.value * words)] + ([opos.get(n_out.value)] if with_pos else [])
    return both(run)


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("words", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_kmers(n, words, with_pos):
    got = run_kmers(text_of(n, n), words, k_for(n, 5 if words == 1 else 33), False, with_pos)
    assert got[0] <= n


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("words", [1, 2])
def test_kmers_fastq(words, with_pos):
    assert run_kmers(FASTQ, words, 21 if words == 1 else 35, True, with_pos)[0] > 0


# ---- minimizers and syncmers of both widths: the count call, then the emit call into buffers of exactly that many entries ---------------
def run_sampled(name, text, words, k, p):
    def run(where):
        n = len(text)
        tin, n_out = In(text, where), C.c_uint64(777)
        fn = getattr(K.lib(), name)
        args = (tin.ptr, n, k, p, 1, MURMUR, 42, where)
        assert fn(*args, None, None, 0, C.byref(n_out), 0, stream(where)) == K.KH_OK
        m = n_out.value
        okm, opos = Out(m * words, np.uint64, where), Out(m, np.uint32, where)
        if m:
            assert fn(*args, okm.ptr, opos.ptr, m, C.byref(n_out), 0, stream(where)) == K.KH_OK
            assert n_out.value == m
        torch.cuda.synchronize()
        return [m, okm.get(), opos.get()]
    return both(run)


@pytest.mark.parametrize("n", SIZES)
def test_minimizers(n):
    k = k_for(n, 5)
    run_sampled("kh_minimizers_from_sequence", text_of(n, n + 1), 1, k, max(1, min(3, n - k + 1)))


@pytest.mark.parametrize("words", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_syncmers(n, words):
    k = k_for(n, 7 if words == 1 else 35)
    run_sampled("kh_syncmers%s_from_sequence" % ("128" if words == 2 else ""), text_of(n, n + 2), words, k, max(1, min(k - 2, 32)))


def test_sampled_fastq():
    assert run_sampled("kh_minimizers_from_fastq", FASTQ, 1, 15, 4)[0] > 0
    assert run_sampled("kh_syncmers_from_fastq", FASTQ, 1, 15, 11)[0] > 0
    assert run_sampled("kh_syncmers128_from_fastq", FASTQ, 2, 35, 31)[0] > 0


# ---- the keep test and the hash of a key batch, both widths ------------------------------------------------------------------------------
@pytest.mark.parametrize("words", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_syncmer_mask(n, words):
    keys = np.random.default_rng(n).integers(0, 1 << 63, n * words, dtype=np.uint64)

    def run(where):
        kin, om = In(keys, where), Out(n, np.uint8, where)
        fn = K.lib().kh_wide_syncmer_mask if words == 2 else K.lib().kh_syncmer_mask
        assert fn(kin.ptr, n, 15 if words == 1 else 40, 11, 1, MURMUR, 42, where, om.ptr, 0, stream(where)) == K.KH_OK
        return [om.get()]      # (the call has waited: the mask is ready)
    both(run)


@pytest.mark.parametrize("words", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_hash_batch(n, words):
    keys = np.random.default_rng(n + 9).integers(0, 1 << 63, n * words, dtype=np.uint64)

    def run(where):
        kin, oh = In(keys, where), Out(n, np.uint64, where)
        fn = K.lib().kh_wide_hash_batch if words == 2 else K.lib().kh_hash_batch
        assert fn(MURMUR, 43, kin.ptr, n, where, oh.ptr, 0, stream(where)) == K.KH_OK
        torch.cuda.synchronize()
        return [oh.get()]
    both(run)


# ---- strand stamps, anchors, chains -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count_invalid", [False, True])
@pytest.mark.parametrize("m", SIZES)
def test_stamp_strand(m, count_invalid):
    rng = np.random.default_rng(m)
    text = text_of(m + 10, m + 3)          # (an odd and an even text length over the sweep; some windows pass the end or hold an N)
    pos = rng.integers(0, len(text), m, dtype=np.uint64).astype(np.uint32)

    def run(where):
        tin, pin, ost, bad = In(text, where), In(pos, where), Out(m, np.uint32, where), C.c_uint64(777)
        assert K.lib().kh_stamp_strand(tin.ptr, len(text), 5, pin.ptr, m, 1000, where, ost.ptr, C.byref(bad) if count_invalid else None, 0, stream(where)) == K.KH_OK
        torch.cuda.synchronize()
        return [ost.get()] + ([bad.value] if count_invalid else [])
    got = both(run)
    if count_invalid:
        assert got[1] == int((got[0] == 0xFFFFFFFF).sum())


@pytest.mark.parametrize("extra", [0, 1])          # both parities of the total: the 4-byte arrays end on and off an 8-byte boundary
@pytest.mark.parametrize("n", SIZES)
def test_anchors_from_csr(n, extra):
    rng = np.random.default_rng(n + extra)
    counts = rng.integers(0, 4, n)
    counts[-1] += 1                                             # never empty
    counts[-1] += (int(counts.sum()) % 2) ^ extra               # total odd <=> extra
    total = int(counts.sum())
    assert total > 0 and total % 2 == extra
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    qpos = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    pos = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)

    def run(where):
        qin, oin, pin = In(qpos, where), In(offsets, where), In(pos, where)
        oq, orp, orv = Out(total, np.uint32, where), Out(total, np.uint32, where), Out(total, np.uint8, where)
        assert K.lib().kh_anchors_from_csr(qin.ptr, oin.ptr, n, pin.ptr, total, where, oq.ptr, orp.ptr, orv.ptr, 0, stream(where)) == K.KH_OK
        torch.cuda.synchronize()
        return [oq.get(), orp.get(), orv.get()]
    both(run)


@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("m", SIZES)
def test_chain_anchors(m, table):
    rng = np.random.default_rng(m)
    lengths = [m] if m < 8 else [m // 3, m - m // 3 - m // 5, m // 5]
    q, r, v, seg = segment_list(rng, lengths, noise=0.1)
    aq, ar, av = np.asarray(q, dtype=np.uint32), np.asarray(r, dtype=np.uint32), np.asarray(v, dtype=np.uint8)
    aseg = np.asarray(seg, dtype=np.uint64)
    cap = m // 3 if table else 0

    def run(where):
        qin, rin, vin, sin = In(aq, where), In(ar, where), In(av, where), In(aseg, where)
        per = [Out(m, np.int32, where) for _ in range(3)]
        tab = [Out(cap, np.uint32, where) for _ in range(3)] + [Out(cap, np.int32, where)]
        ptrs = [o.ptr for o in per] + [o.ptr if table and cap else None for o in tab]
        nc = C.c_uint64(777)
        st = K.lib().kh_chain_anchors(qin.ptr, rin.ptr, vin.ptr, m, sin.ptr, len(lengths), 15, 16, 5000, 500, 20, 3, where, *ptrs,
                                      cap if table else 0, C.byref(nc), 0, stream(where))
        assert st == K.KH_OK
        torch.cuda.synchronize()
        return [nc.value] + [o.get() for o in per] + [o.get(nc.value if table and cap else 0) for o in tab]
    got = both(run)
    if m >= 63:
        assert got[0] > 0      # (the runs are long enough to be kept: the table columns are exercised)


# ---- kh_csr_unpermute: device memory only, against the model, each optional output null in turn -----------------------------------------
@pytest.mark.parametrize("drop", [None, "counts", "offsets", "positions"])
@pytest.mark.parametrize("n", SIZES)
def test_csr_unpermute(n, drop):
    rng = np.random.default_rng(n)
    counts_perm = rng.integers(0, 4, n).astype(np.uint32)
    counts_perm[0] += 1 - int(counts_perm.sum()) % 2          # an odd total
    total = int(counts_perm.sum())
    pos_perm = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)
    origin = rng.permutation(n).astype(np.uint32)
    ec, eo, ep = np_csr_unpermute(counts_perm, pos_perm, origin)
    cin, pin, oin = In(counts_perm, DEVICE), In(pos_perm, DEVICE), In(origin, DEVICE)
    oc, oo, op = Out(n, np.uint32, DEVICE), Out(n + 1, np.uint64, DEVICE), Out(total, np.uint32, DEVICE)
    n_out = C.c_uint64(777)
    st = K.lib().kh_csr_unpermute(cin.ptr, pin.ptr, oin.ptr, n, None if drop == "counts" else oc.ptr, None if drop == "offsets" else oo.ptr,
                                  None if drop == "positions" else op.ptr, total, C.byref(n_out), 0, stream(DEVICE))
    torch.cuda.synchronize()
    assert st == K.KH_OK and n_out.value == total
    untouched = lambda o: (o.get() .view(np.uint8) == FILL).all()
    assert untouched(oc) if drop == "counts" else np.array_equal(oc.get(), ec)
    assert untouched(oo) if drop == "offsets" else np.array_equal(oo.get(), eo)
    assert untouched(op) if drop == "positions" else np.array_equal(op.get(), ep)
