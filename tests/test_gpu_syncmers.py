"""GPU: kh_syncmers[128]_from_sequence / _fastq and kh_[wide_]syncmer_mask (kmerhash_amd.syncmers_from_sequence, syncmers128_from_sequence,
is_syncmer, is_syncmer128) against the numpy model of tests/syncmer_model.py, exactly.  The shapes are the smallest at which the tile
logic can go wrong (a tile is 4096 start offsets, the halo lies on its right): texts of 0, k - 1 and k bytes, texts that end with the
last window of tile 0, with the first window of tile 1 and one byte behind it -- so the k-mers whose s-mers straddle the tile edge are
decided with the halo being text and being past the end --, and three tiles plus 17 bytes with an N at a tile edge, broken by newlines,
and with a poly-A stretch that covers a whole tile (every window kept: the full-tile case of the 16-byte emit)."""
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
from kmerhash_amd.wide import kmers128_from_sequence  # noqa: E402
from index_model import fastq_masked  # noqa: E402
from syncmer_model import kept_flags, np_syncmers, np_syncmers_fastq  # noqa: E402

TILE = 4096
BIG = 3 * TILE + 17
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
SEED = 42
KS = [(15, 11), (15, 15), (15, 1), (32, 32), (32, 1), (31, 21)]
KS_WIDE = [(33, 32), (63, 31), (64, 32), (64, 1), (40, 20)]
ALL_KS = [(k, s, False) for k, s in KS] + [(k, s, True) for k, s in KS_WIDE]
LAYOUTS = ["n_edge", "newlines", "polya"]


def lengths(k):
    return sorted({0, k - 1, k, TILE - 2 + k, TILE - 1 + k, TILE + k - 1, TILE + k, BIG})


def make_text(n, k, layout="plain"):
    rng = np.random.default_rng(7 * n + k)
    t = BASES[rng.integers(0, 4, n)].copy()
    if layout == "n_edge":
        for p, c in ((TILE - 1, "N"), (2 * TILE, "n"), (3 * TILE - 1, "\n"), (3 * TILE, "N")):
            if p < n:
                t[p] = ord(c)
        t[100:400] |= 0x20                                  # lower case
    elif layout == "newlines":
        t[60::61] = 10                                      # lines of 60 bases: k = 63 and 64 have no window at all
        t[TILE - 70: TILE + 70] = BASES[rng.integers(0, 4, 140)]      # but one run crosses the first tile edge
    elif layout == "polya":
        t[TILE - 200: 2 * TILE + 300] = ord("A")            # covers tile 1 whole and both of its edges
    return t


def sample(text, k, s, canonical, hash_, wide, fastq=False):
    if wide:
        fn = kh.syncmers128_from_fastq if fastq else kh.syncmers128_from_sequence
    else:
        fn = kh.syncmers_from_fastq if fastq else kh.syncmers_from_sequence
    km, pos = fn(text, k, s, canonical, hash_, SEED)
    if hasattr(km, "is_cuda"):
        assert km.is_cuda and km.dtype == torch.int64 and pos.dtype == torch.int32
        km, pos = km.cpu().numpy().view(np.uint64), pos.cpu().numpy().view(np.uint32)
    assert km.dtype == np.uint64 and pos.dtype == np.uint32 and km.shape == ((len(pos), 2) if wide else (len(pos),))
    return km, pos


@pytest.mark.parametrize("hash_", ["murmur", "farm"])
@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k,s,wide", ALL_KS)
def test_text_lengths_around_the_tile_edge(k, s, wide, canonical, hash_):
    for n in lengths(k):
        text = make_text(n, k)
        ekm, epos = np_syncmers(text, k, s, canonical, hash_, SEED, wide)
        km, pos = sample(text, k, s, canonical, hash_, wide)
        assert np.array_equal(pos, epos) and np.array_equal(km, ekm), (n, len(pos), len(epos))
        if n >= TILE + k - 1 and s < k and s > 1:
            # the windows whose s-mers straddle the tile edge are all there, and the model decided each of them
            pall, _ = kept_flags(text, k, s, canonical, hash_, SEED)
            assert ((pall > TILE - 1 - (k - s)) & (pall < TILE)).sum() == k - s


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,s,wide", ALL_KS)
def test_text_contents_host_device_and_unaligned(k, s, wide, layout):
    canonical, hash_ = (k + s) % 2 == 0, "murmur" if k % 2 else "farm"
    text = make_text(BIG, k, layout)
    ekm, epos = np_syncmers(text, k, s, canonical, hash_, SEED, wide)
    if layout == "polya":
        assert np.isin(np.arange(TILE - 200, 2 * TILE + 300 - k + 1), epos).all()          # every window of the stretch, all of tile 1
    elif layout == "n_edge":
        assert not np.isin(np.arange(TILE - k, TILE), epos).any() and len(epos) > 0
    elif k <= 60:
        assert len(epos) > 0
    km, pos = sample(text, k, s, canonical, hash_, wide)
    assert np.array_equal(pos, epos) and np.array_equal(km, ekm)
    # device buffer, and a device view that starts one byte into an allocation (the unaligned path of the tile loader)
    d = torch.from_numpy(np.concatenate([[ord("A")], text]).astype(np.uint8)).cuda()
    assert d[1:].data_ptr() % 16 == 1
    for view in (d[1:].clone(), d[1:]):
        km, pos = sample(view, k, s, canonical, hash_, wide)
        assert np.array_equal(pos, epos) and np.array_equal(km, ekm)


@pytest.mark.parametrize("k,wide,canonical", [(15, False, True), (32, False, False), (1, False, False), (20, True, True), (32, True, False), (1, True, True)])
def test_s_equal_k_is_the_all_window_front_end_byte_for_byte(k, wide, canonical):
    text = make_text(BIG, k, "n_edge")
    for t in (text, torch.from_numpy(text).cuda()):
        km, pos = (kh.syncmers128_from_sequence if wide else kh.syncmers_from_sequence)(t, k, k, canonical, "murmur", SEED)
        akm, apos = (kmers128_from_sequence if wide else kmers_from_sequence)(t, k, canonical, with_positions=True)
        if hasattr(km, "is_cuda"):
            km, pos, akm, apos = (x.cpu().numpy() for x in (km, pos, akm, apos))
        assert km.tobytes() == akm.tobytes() and pos.tobytes() == apos.tobytes() and len(pos) > 3 * TILE - 300


@pytest.mark.parametrize("k,s,wide,hash_,canonical", [(15, 11, False, "murmur", True), (31, 21, False, "farm", False), (40, 20, True, "murmur", True),
                                                     (63, 31, True, "farm", False)])
def test_fastq(k, s, wide, hash_, canonical):
    raw = synthetic_fastq(200, 150, genome_len=20_000, seed=5).replace(b"I" * 150, b"ACGT" * 37 + b"AC")      # ACGT-only quality strings
    text = np.frombuffer(raw, dtype=np.uint8)
    ekm, epos = np_syncmers_fastq(text, k, s, canonical, hash_, SEED, wide)
    assert len(epos) > 200
    line = np.concatenate([[0], np.cumsum(text == 10)[:-1]])
    assert (line[epos] % 4 == 1).all() and (line[epos + k - 1] == line[epos]).all()      # nothing on an id or quality line, nothing across reads
    for t in (text, torch.from_numpy(np.array(text)).cuda()):
        km, pos = sample(t, k, s, canonical, hash_, wide, fastq=True)
        assert np.array_equal(pos, epos) and np.array_equal(km, ekm)
    km, pos = sample(fastq_masked(text), k, s, canonical, hash_, wide)                    # the masked text through the sequence entry point
    assert np.array_equal(pos, epos) and np.array_equal(km, ekm)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("k,s,wide", [(15, 11, False), (40, 20, True)])
def test_count_only_and_short_room(k, s, wide, where):
    hash_, words = "murmur", 2 if wide else 1
    text = make_text(BIG, k, "polya")
    ekm, epos = np_syncmers(text, k, s, True, hash_, SEED, wide)
    fn = getattr(K.lib(), "kh_syncmers128_from_sequence" if wide else "kh_syncmers_from_sequence")
    n_out = C.c_uint64(0)
    dev = where == "device"
    if dev:
        dt = torch.from_numpy(np.array(text)).cuda()
        tptr, mem = dt.data_ptr(), K.KH_MEM_DEVICE
    else:
        tptr, mem = text.ctypes.data, K.KH_MEM_HOST
    args = (tptr, len(text), k, s, 1, HASHES[hash_], SEED, mem)
    assert fn(*args, None, None, 0, C.byref(n_out), 0, None) == K.KH_OK
    m = len(epos)
    assert n_out.value == m > TILE

    if dev:
        a = torch.full((m * words,), 7, dtype=torch.int64, device="cuda"); b = torch.full((m,), 9, dtype=torch.int32, device="cuda")
        ap, bp, host = a.data_ptr(), b.data_ptr(), lambda x: x.cpu().numpy()
    else:
        a = np.full(m * words, 7, dtype=np.int64); b = np.full(m, 9, dtype=np.int32)
        ap, bp, host = a.ctypes.data, b.ctypes.data, lambda x: x
    n_out = C.c_uint64(0)
    assert fn(*args, ap, bp, m - 1, C.byref(n_out), 0, None) == K.KH_ERR_INVALID
    torch.cuda.synchronize()
    assert n_out.value == m and (host(a) == 7).all() and (host(b) == 9).all()            # refused with the outputs untouched
    assert fn(*args, ap, bp, m, C.byref(n_out), 0, None) == K.KH_OK
    torch.cuda.synchronize()
    assert n_out.value == m
    assert np.array_equal(host(a).view(np.uint64).reshape(ekm.shape), ekm) and np.array_equal(host(b).view(np.uint32), epos)


@pytest.mark.parametrize("hash_", ["murmur", "farm"])
@pytest.mark.parametrize("k,s,wide", ALL_KS)
def test_is_syncmer_is_the_kept_flag_of_every_window(k, s, wide, hash_):
    text = make_text(TILE + 300, k, "n_edge")
    is_fn = kh.is_syncmer128 if wide else kh.is_syncmer
    all_fn = kmers128_from_sequence if wide else kmers_from_sequence
    for canonical in (True, False):
        _, keep = kept_flags(text, k, s, canonical, hash_, SEED)
        km = all_fn(text, k, canonical)
        assert len(km) == len(keep) > TILE
        got = is_fn(km, k, s, canonical, hash_, SEED)
        assert got.dtype == bool and np.array_equal(got, keep)
        dgot = is_fn(torch.from_numpy(km.view(np.int64)).cuda(), k, s, canonical, hash_, SEED)
        assert dgot.is_cuda and dgot.dtype == torch.bool and np.array_equal(dgot.cpu().numpy(), keep)
        if canonical:      # the other strand's bit pattern of a canonical key gives the same answer
            fw = all_fn(text, k, False)
            assert (fw != km).any() and np.array_equal(is_fn(fw, k, s, True, hash_, SEED), keep)
    assert len(is_fn(np.zeros((0, 2) if wide else 0, dtype=np.uint64), k, s, True, hash_, SEED)) == 0
