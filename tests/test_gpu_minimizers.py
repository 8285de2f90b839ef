"""GPU: kh_minimizers_from_sequence / _fastq (kmerhash_amd.minimizers_from_sequence / _fastq) against the numpy model of
tests/minimizer_model.py, exactly.  The texts are three tiles of the front end (4096 start offsets each) plus 300 bytes, laid out
around the tile boundaries for the (k, w) under test: runs that end one byte before, at and one byte behind a boundary, full windows
that straddle a boundary with their pick on either side, a non-base byte closer than w + k - 1 to a boundary, a poly-A stretch (every
hash ties) across one, runs of exactly w + k - 2 and w + k - 1 bases, lower case, and a last run that ends with the buffer."""
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
from kmerhash_amd.kmers import kmers_from_sequence, synthetic_fastq  # noqa: E402
from kmerhash_amd.table import HASHES  # noqa: E402
from index_model import fastq_masked, np_kmers_pos  # noqa: E402
from minimizer_model import np_minimizers, np_minimizers_fastq, order_keys  # noqa: E402

TILE = 4096
N = 3 * TILE + 300
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
SEED = 42
# (k, w, ordering hash, canonical): every (k, w) of interest, every hash, both strand rules -- not the full product
CASES = [(1, 1, "identity", False), (15, 10, "murmur", True), (21, 19, "farm", True), (31, 2, "murmur3avx64", False),
         (32, 256, "murmur", True), (15, 1, "farm", False), (15, 10, "identity", False), (32, 256, "identity", False),
         (21, 19, "murmur3avx64", False), (31, 2, "farm", True), (15, 10, "farm", False), (32, 256, "murmur3avx64", True)]
LAYOUTS = ["ends0", "ends1", "ends2", "straddle"]
POLY_A0, POLY_A1 = 3 * TILE - 310, 3 * TILE + 5


def make_text(k, w, layout):
    span = w + k - 1
    rng = np.random.default_rng(1000 * k + w)
    t = BASES[rng.integers(0, 4, N)].copy()
    # tile 0: runs of exactly span - 1 and span bases between non-bases, then lower case
    p = 50
    t[p] = ord("N"); t[p + span] = ord("N"); t[p + span + 1 + span] = 10        # [p+1, p+span): span-1 bases; then span bases
    t[1000:1400] |= 0x20
    if layout.startswith("ends"):
        s = int(layout[-1])
        t[TILE + s] = ord("N")                  # the run before it ends at byte 4095, 4096 or 4097
        t[2 * TILE + s] = 10                    # and at 8191, 8192 or 8193
    else:
        # both boundaries lie inside runs; a non-base byte less than w + k - 1 before 4096 and one less than that behind 8192,
        # the latter far enough for the windows that straddle 8192 to be full
        t[TILE - span // 2 - 1] = ord("N")
        t[2 * TILE + span - 1] = ord("n")
    # poly-A across the boundary at 12288, long enough to hold full windows of the widest case; the run goes on with random bases and
    # ends with the buffer (no newline)
    t[POLY_A0: POLY_A1] = ord("A")
    assert t[-1] in BASES and N - POLY_A1 >= 287
    return t


def check_layout(text, k, w, canonical, hash_):
    """the cases the layout is there for are really in it (decided by the model's own keys)"""
    km, pos = np_kmers_pos(text, k, canonical)
    h = dict(zip(pos.tolist(), order_keys(km, hash_, SEED).tolist()))
    sides = set()
    for edge in (TILE, 2 * TILE):
        for s in range(edge - w + 1, edge):
            if all(p in h for p in range(s, s + w)):
                sides.add(min(range(s, s + w), key=lambda p: (h[p], p)) < edge)
    return sides


@pytest.fixture(scope="module")
def cache():
    return {}


def expected(cache, k, w, hash_, canonical, layout):
    key = (k, w, hash_, canonical, layout)
    if key not in cache:
        text = make_text(k, w, layout)
        text.setflags(write=False)
        cache[key] = (text,) + np_minimizers(text, k, w, canonical, hash_, SEED)
    return cache[key]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,w,hash_,canonical", CASES)
def test_against_the_model(cache, k, w, hash_, canonical, layout):
    text, ekm, epos = expected(cache, k, w, hash_, canonical, layout)
    span = w + k - 1
    if layout == "straddle" and w > 1:
        assert check_layout(text, k, w, canonical, hash_) == {True, False}, "the layout lost its straddling picks on both sides"
    # the run of span - 1 bases yields nothing, the run of span bases exactly one
    assert not ((epos > 50) & (epos < 50 + span)).any() and ((epos > 50 + span) & (epos < 50 + 2 * span + 1)).sum() == 1
    assert len(epos) and epos[-1] >= N - span                                             # the run that ends with the buffer
    assert np.isin(np.arange(POLY_A0, POLY_A1 - span + 1), epos).all()                    # poly-A: every full-window start
    # host buffer
    km, pos = kh.minimizers_from_sequence(text, k, w, canonical, hash_, SEED)
    assert km.dtype == np.uint64 and pos.dtype == np.uint32
    assert np.array_equal(pos, epos) and np.array_equal(km, ekm)
    # device buffer, and a device view that starts one byte into an allocation (the unaligned path of the tile loader)
    d = torch.from_numpy(np.concatenate([[ord("A")], text]).astype(np.uint8)).cuda()
    for view in (d[1:].clone(), d[1:]):
        km, pos = kh.minimizers_from_sequence(view, k, w, canonical, hash_, SEED)
        assert km.is_cuda and km.dtype == torch.int64 and pos.dtype == torch.int32
        assert np.array_equal(pos.cpu().numpy().view(np.uint32), epos) and np.array_equal(km.cpu().numpy().view(np.uint64), ekm)
    assert d[1:].data_ptr() % 16 == 1


@pytest.mark.parametrize("k,canonical", [(1, False), (15, True), (15, False), (32, True)])
def test_w1_is_the_all_window_front_end(cache, k, canonical):
    text = make_text(k, 1, "straddle")
    km, pos = kh.minimizers_from_sequence(text, k, 1, canonical, "murmur", SEED)
    akm, apos = kmers_from_sequence(text, k, canonical, with_positions=True)
    assert km.tobytes() == akm.tobytes() and pos.tobytes() == apos.tobytes() and len(km) > 3 * TILE - 300


@pytest.mark.parametrize("where", ["host", "device"])
def test_count_only_and_short_room(cache, where):
    k, w, hash_, canonical = 15, 10, "murmur", True
    text, ekm, epos = expected(cache, k, w, hash_, canonical, "straddle")
    L = K.lib()
    n_out = C.c_uint64(0)
    dev = where == "device"
    if dev:
        dt = torch.from_numpy(np.array(text)).cuda()
        tptr, mem = dt.data_ptr(), K.KH_MEM_DEVICE
    else:
        tptr, mem = text.ctypes.data, K.KH_MEM_HOST
    args = (tptr, len(text), k, w, 1, HASHES[hash_], SEED, mem)
    assert L.kh_minimizers_from_sequence(*args, None, None, 0, C.byref(n_out), 0, None) == K.KH_OK
    assert n_out.value == len(epos)
    m = len(epos)

    def room(cap):
        if dev:
            a = torch.full((cap,), 7, dtype=torch.int64, device="cuda"); b = torch.full((cap,), 9, dtype=torch.int32, device="cuda")
            return a, b, a.data_ptr(), b.data_ptr(), lambda x: x.cpu().numpy()
        a = np.full(cap, 7, dtype=np.int64); b = np.full(cap, 9, dtype=np.int32)
        return a, b, a.ctypes.data, b.ctypes.data, lambda x: x

    a, b, ap, bp, host = room(m)
    n_out = C.c_uint64(0)
    assert L.kh_minimizers_from_sequence(*args, ap, bp, m - 1, C.byref(n_out), 0, None) == K.KH_ERR_INVALID
    torch.cuda.synchronize()
    assert n_out.value == m and (host(a) == 7).all() and (host(b) == 9).all()            # refused with the outputs untouched
    assert L.kh_minimizers_from_sequence(*args, ap, bp, m, C.byref(n_out), 0, None) == K.KH_OK
    torch.cuda.synchronize()
    assert n_out.value == m
    assert np.array_equal(host(a).view(np.uint64), ekm) and np.array_equal(host(b).view(np.uint32), epos)


def test_nothing_to_sample():
    for text in (np.zeros(0, dtype=np.uint8), np.frombuffer(b"ACGT" * 5, dtype=np.uint8)):      # n == 0, n < w + k - 1
        km, pos = kh.minimizers_from_sequence(text, 15, 10)
        assert len(km) == 0 and len(pos) == 0
        km, pos = kh.minimizers_from_sequence(torch.from_numpy(np.array(text)).cuda(), 15, 10)
        assert len(km) == 0 and len(pos) == 0 and km.is_cuda
    text = np.frombuffer(b"ACGTTGCAACGTGGCATTACGATC", dtype=np.uint8)                         # exactly w + k - 1 bytes: one pick
    km, pos = kh.minimizers_from_sequence(text, 15, 10)
    ekm, epos = np_minimizers(text, 15, 10, True, "murmur", 42)
    assert len(km) == 1 and np.array_equal(km, ekm) and np.array_equal(pos, epos)


@pytest.mark.parametrize("k,w,hash_,canonical", [(15, 10, "murmur", True), (21, 19, "farm", False), (31, 2, "identity", True)])
def test_fastq(k, w, hash_, canonical):
    raw = synthetic_fastq(200, 150, genome_len=20_000, seed=5).replace(b"I" * 150, b"ACGT" * 37 + b"AC")      # ACGT-only quality strings
    text = np.frombuffer(raw, dtype=np.uint8)
    ekm, epos = np_minimizers_fastq(text, k, w, canonical, hash_, SEED)
    assert len(epos) > 200
    line = np.concatenate([[0], np.cumsum(text == 10)[:-1]])
    # no pick on an id or quality line, and the whole window of every pick's full windows lies on one sequence line
    assert (line[epos] % 4 == 1).all() and (line[epos + k - 1] == line[epos]).all()
    for t in (text, torch.from_numpy(np.array(text)).cuda()):
        km, pos = kh.minimizers_from_fastq(t, k, w, canonical, hash_, SEED)
        if hasattr(km, "is_cuda"):
            km, pos = km.cpu().numpy().view(np.uint64), pos.cpu().numpy().view(np.uint32)
        assert np.array_equal(pos, epos) and np.array_equal(km, ekm)
    # the masked text through the sequence entry point is the same thing
    km, pos = kh.minimizers_from_sequence(fastq_masked(text), k, w, canonical, hash_, SEED)
    assert np.array_equal(pos, epos) and np.array_equal(km, ekm)
