"""GPU: the alignment rule of 16-byte keys (include/kmerhash_amd.h, above kh_wide_create).  A device array of 16-byte keys must be
16-byte aligned wherever a key moves as one 16-byte access: every entry point that reads one refuses the view flat[1:2n+1].view(n, 2) -- 8 bytes past a 16-byte
boundary -- with KH_ERR_INVALID before anything is launched.  Per entry point: the refusal; the handle's state (size, capacity, info
bytes, items; export of an index; registers) bit-identical before and after; sentinel-filled outputs untouched; the same keys in an
aligned clone give the result of the CPU model (oracle/wide_model.py, tests/index_seq_model.py, the oracle's hashes, tests/syncmer_model.py);
and a host numpy view at the same odd offset, which the library stages, gives the model's result too.  The front ends that WRITE
16-byte k-mers with one store each (kh_kmers128_*, kh_syncmers128_*) refuse such an output the same way.  No misaligned array reaches a
kernel here: every call on the view is expected to return before its first launch."""
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
from kmerhash_amd._capi import KH_ERR_INVALID, KhError  # noqa: E402
from kmerhash_amd.hll import hyperloglog64  # noqa: E402
from kmerhash_amd.index import WideKmerPositionIndex  # noqa: E402
from kmerhash_amd.table import _hash_id  # noqa: E402
from kmerhash_amd.wide import hashmap_robinhood_doubling_wide_stream  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from oracle.wide_model import WideModel  # noqa: E402
from refusal_checks import assert_unchanged, snapshot  # noqa: E402
from index_seq_model import WideSeqModel, text_pairs  # noqa: E402
from syncmer_model import np_is_syncmer, np_syncmers, np_syncmers_fastq  # noqa: E402

N = 1000                       # one partition pass
SENTINEL = 0xA5
HASH, HID, SEED = "murmur3avx64", O.HASH_MURMUR3_X86, 43


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def u64(x):
    return host(x).view(np.uint64)


def u32(x):
    return host(x).view(np.uint32)


def make_keys(seed, n=N):
    """n 16-byte keys, a fifth of them repeats of earlier ones, both words in use"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 63, size=(n, 2), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 2), dtype=np.uint64)
    k[n - n // 5:] = k[rng.integers(0, n - n // 5, n // 5)]
    return np.ascontiguousarray(k[rng.permutation(n)])


def aligned(keys):
    t = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def misaligned(keys):
    """the same keys as a device view 8 bytes past a 16-byte boundary; the words around it are keys too (poison: a call that rounded
    the pointer down or read on would see other keys)"""
    n = len(keys)
    flat = torch.full((2 * n + 2,), 0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    flat[1:2 * n + 1] = aligned(keys).reshape(-1)
    v = flat[1:2 * n + 1].view(n, 2)
    assert flat.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 8 and v.is_contiguous()
    return v


def host_odd(keys):
    """the same keys as a host numpy view 8 bytes past a 16-byte boundary"""
    n = len(keys)
    raw = bytearray(16 * n + 32)
    base = np.frombuffer(raw, dtype=np.uint8).ctypes.data
    off = (8 - base) % 16
    v = np.frombuffer(raw, dtype=np.uint64, offset=off, count=2 * n).reshape(n, 2)
    v[:] = keys
    assert v.ctypes.data % 16 == 8
    return v


def sentinels(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def untouched(t):
    return bool((t.view(torch.uint8) == SENTINEL).all())


def refused(fn, *args):
    with pytest.raises(KhError) as e:
        fn(*args)
    assert e.value.status == KH_ERR_INVALID
    return e.value


# ---- the table ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def table():
    """a wide table and its model holding the same 1000 pairs"""
    keys, vals = make_keys(1), np.arange(N, dtype=np.uint32) + np.uint32(5)
    t, m = hashmap_robinhood_doubling_wide_stream(128, 0.4, 0.9, hash=HASH, seed=SEED), WideModel(128, 0.4, 0.9, HASH, SEED)
    assert t.insert(keys, vals) == m.insert(keys, vals)
    yield t, m
    t.close(); m.close()


def same_table(t, m):
    assert (t.size(), t.capacity()) == (m.size(), m.capacity())
    assert np.array_equal(t.export_info(), m.export_info())
    assert all(np.array_equal(a, b) for a, b in zip(t.sorted_items(), m.sorted_items()))


INSERTS = {
    "insert": (lambda t, k, v: t.insert(k, v), lambda m, k, v: m.insert(k, v)),
    "insert_reduce_plus": (lambda t, k, v: t.insert_reduce_plus(k, v), lambda m, k, v: m.insert_reduce_plus(k, v)),
    "insert_reduce_plus_ones": (lambda t, k, v: t.insert_reduce_plus(k), lambda m, k, v: m.insert_reduce_plus(k)),
    "insert_reduce_op_plus": (lambda t, k, v: t.insert_reduce(k, v, "plus"), lambda m, k, v: m.insert_reduce_plus(k, v)),
}


@pytest.mark.parametrize("name", sorted(INSERTS))
def test_insert_forms_refuse_a_misaligned_device_batch(table, name):
    t, m = table
    gpu, model = INSERTS[name]
    batch = np.concatenate([make_keys(2)[:N // 2], make_keys(1)[:N // 2]])      # half new keys, half held ones
    vals = np.arange(N, dtype=np.uint32) * np.uint32(3) + np.uint32(1)
    dv = torch.from_numpy(vals.view(np.int32)).cuda()
    snap = snapshot(t)
    err = refused(gpu, t, misaligned(batch), dv)
    assert "16-byte aligned" in str(err)
    assert_unchanged(t, snap, new_keys=batch[:N // 2])
    same_table(t, m)
    # the same keys in an aligned clone, then once more from a host view at the odd offset: the model's results
    assert gpu(t, misaligned(batch).clone(), dv) == model(m, batch, vals)
    same_table(t, m)
    assert gpu(t, host_odd(batch), vals) == model(m, batch, vals)
    same_table(t, m)


def test_streamed_insert_refuses_a_misaligned_piece_and_stays_open(table):
    t, m = table
    a, b = make_keys(3), make_keys(4)
    snap = snapshot(t)
    t.insert_begin(2 * N, reduce_plus=True)
    t.insert_feed(aligned(a))
    refused(t.insert_feed, misaligned(b))                  # nothing fed: the insert is still open and takes the piece once it is aligned
    t.insert_feed(host_odd(b))
    assert t.insert_end() == m.insert_reduce_plus(np.concatenate([a, b]))
    same_table(t, m)
    assert t.size() > snap["size"]
    # refused right after begin, then aborted: the table as it was
    snap = snapshot(t)
    t.insert_begin(N)
    refused(t.insert_feed, misaligned(b), torch.zeros(N, dtype=torch.int32, device="cuda"))
    t.insert_abort()
    assert_unchanged(t, snap)


def test_queries_and_erase_refuse_a_misaligned_device_batch(table):
    t, m = table
    L = K.lib()
    q = np.concatenate([make_keys(1)[:600], make_keys(5)[:400]])                  # hits and misses
    bad, good, odd = misaligned(q), misaligned(q).clone(), host_odd(q)
    assert good.data_ptr() % 16 == 0
    snap = snapshot(t)
    for fn in (t.count, t.find_values, t.find, t.erase):
        refused(fn, bad)
    # the C entry points over sentinel-filled outputs: nothing written, the scalar left at 0
    n_out = C.c_uint64(77)
    o8, o32, ok = sentinels(N, torch.uint8), sentinels(N, torch.int32), sentinels((N, 2), torch.int64)
    assert L.kh_wide_count(t._h, bad.data_ptr(), N, K.KH_MEM_DEVICE, o8.data_ptr()) == KH_ERR_INVALID
    assert L.kh_wide_find(t._h, bad.data_ptr(), N, K.KH_MEM_DEVICE, o32.data_ptr(), o8.data_ptr(), C.byref(n_out)) == KH_ERR_INVALID
    assert L.kh_wide_find_compact(t._h, bad.data_ptr(), N, K.KH_MEM_DEVICE, ok.data_ptr(), o32.data_ptr(), C.byref(n_out)) == KH_ERR_INVALID
    assert L.kh_wide_erase(t._h, bad.data_ptr(), N, K.KH_MEM_DEVICE, C.byref(n_out)) == KH_ERR_INVALID
    torch.cuda.synchronize()
    assert n_out.value == 0 and untouched(o8) and untouched(o32) and untouched(ok)
    assert_unchanged(t, snap)
    same_table(t, m)
    for keys in (good, odd):
        assert np.array_equal(host(t.count(keys)), m.count(q))
        gv, gf = t.find_values(keys)
        ev, ef = m.find_values(q)
        assert np.array_equal(host(gf), ef) and np.array_equal(u32(gv), ev)
        gk, gv = t.find(keys)
        ek, ev = m.find(q)
        assert np.array_equal(u64(gk), ek) and np.array_equal(u32(gv), ev)
    assert 0 < m.count(q).sum() < N
    assert t.erase(good) == m.erase(q)
    same_table(t, m)
    again = make_keys(1)[600:]
    assert t.erase(host_odd(again)) == m.erase(again)
    same_table(t, m)


# ---- the handle-free calls ----------------------------------------------------------------------------------------------------------
def test_hash_batch_refuses_a_misaligned_device_batch():
    keys = make_keys(6)
    bad = misaligned(keys)
    refused(kh.hash_batch_wide, bad, HASH, SEED)
    out = sentinels(N, torch.int64)
    st = K.lib().kh_wide_hash_batch(HID, SEED, bad.data_ptr(), N, K.KH_MEM_DEVICE, out.data_ptr(), 0, None)
    torch.cuda.synchronize()
    assert st == KH_ERR_INVALID and untouched(out)
    exp = O.hash16_batch(HID, SEED, keys)
    assert np.array_equal(u64(kh.hash_batch_wide(bad.clone(), HASH, SEED)), exp)
    assert np.array_equal(kh.hash_batch_wide(host_odd(keys), HASH, SEED), exp)


def test_shard_permute_refuses_misaligned_keys_and_outputs():
    keys = make_keys(7)
    bad, good = misaligned(keys), aligned(keys)
    counts = (C.c_uint64 * 4)(9, 9, 9, 9)
    fn = K.lib().kh_wide_shard_permute
    out = sentinels((N + 1, 2), torch.int64)
    assert fn(HID, SEED, 4, bad.data_ptr(), None, N, out.data_ptr(), None, counts, 0, None) == KH_ERR_INVALID
    assert fn(HID, SEED, 4, good.data_ptr(), None, N, out.data_ptr() + 8, None, counts, 0, None) == KH_ERR_INVALID
    torch.cuda.synchronize()
    assert untouched(out)
    assert fn(HID, SEED, 4, good.data_ptr(), None, N, out.data_ptr(), None, counts, 0, None) == K.KH_OK
    torch.cuda.synchronize()
    rank = O.hash16_batch(HID, SEED, keys) & np.uint64(3)
    order = np.argsort(rank, kind="stable")
    assert list(counts) == np.bincount(rank.astype(np.int64), minlength=4).tolist()
    assert np.array_equal(u64(out[:N]), keys[order]) and untouched(out[N:])


@pytest.mark.parametrize("k,s,canonical", [(63, 31, True), (40, 11, False)])
def test_syncmer_mask_refuses_a_misaligned_device_batch(k, s, canonical):
    keys = make_keys(8)
    if k < 64:
        keys[:, 1] &= np.uint64((1 << (2 * k - 64)) - 1)
    n = len(keys)
    bad = misaligned(keys)
    refused(kh.is_syncmer128, bad, k, s, canonical)
    out = sentinels(n, torch.uint8)
    st = K.lib().kh_wide_syncmer_mask(bad.data_ptr(), n, k, s, int(canonical), _hash_id("murmur"), 42, K.KH_MEM_DEVICE, out.data_ptr(), 0, None)
    torch.cuda.synchronize()
    assert st == KH_ERR_INVALID and untouched(out)
    exp = np_is_syncmer(keys, k, s, canonical, "murmur", 42)
    assert 0 < exp.sum() < n
    assert np.array_equal(host(kh.is_syncmer128(bad.clone(), k, s, canonical)), exp)
    assert np.array_equal(kh.is_syncmer128(host_odd(keys), k, s, canonical), exp)


# ---- 16-byte k-mers as an OUTPUT: the front ends that store one k-mer per 16-byte access -------------------------------------------------
def front_end_texts():
    """-> (a sequence text with exactly N windows of 63 bases, a FASTQ text of 12 reads of 101 bases)"""
    rng = np.random.default_rng(21)
    base = np.frombuffer(b"ACGT", dtype=np.uint8)
    seq = base[rng.integers(0, 4, N + 62)].copy()
    recs = [b"@r%d\n%s\n+\n%s\n" % (i, base[rng.integers(0, 4, 101)].tobytes(), b"I" * 101) for i in range(12)]
    return seq, np.frombuffer(b"".join(recs), dtype=np.uint8).copy()


FRONT_ENDS = ["kh_kmers128_from_sequence", "kh_kmers128_from_fastq", "kh_kmers128_from_sequence_pos", "kh_kmers128_from_fastq_pos",
              "kh_syncmers128_from_sequence", "kh_syncmers128_from_fastq"]


@pytest.mark.parametrize("name", FRONT_ENDS)
def test_wide_front_ends_refuse_a_misaligned_device_output(name):
    k, s, canonical = 63, 31, True
    fastq, sampler, with_pos = "fastq" in name, "syncmers" in name, "syncmers" in name or name.endswith("_pos")
    seq, fq = front_end_texts()
    text = fq if fastq else seq
    if sampler:
        ekm, epos = (np_syncmers_fastq if fastq else np_syncmers)(text, k, s, canonical, "murmur", 42, True)
        ekm = np.asarray(ekm, dtype=np.uint64).reshape(-1, 2)
    else:
        ekm, epos = text_pairs(text, k, canonical, fastq=fastq, wide=True)
        assert fastq or len(ekm) == N
    m = len(ekm)
    assert m > 20
    fn = getattr(K.lib(), name)

    def call(tptr, where, kptr, pptr):
        n_out = C.c_uint64(77)
        lead = (tptr, len(text), k) + ((s, int(canonical), _hash_id("murmur"), 42) if sampler else (int(canonical),)) + (where, kptr)
        tail = ((pptr, len(text)) if sampler else (pptr,) if with_pos else ()) + (C.byref(n_out), 0, None)
        return fn(*lead, *tail), n_out.value

    dtext = torch.from_numpy(text).cuda()
    room = sentinels((len(text) + 1, 2), torch.int64)
    pos = sentinels(len(text), torch.int32)
    assert room.data_ptr() % 16 == 0
    # a device output 8 bytes past a 16-byte boundary: refused before the count pass, nothing written, *n_out left at 0
    st, n = call(dtext.data_ptr(), K.KH_MEM_DEVICE, room.data_ptr() + 8, pos.data_ptr())
    torch.cuda.synchronize()
    assert (st, n) == (KH_ERR_INVALID, 0) and untouched(room) and untouched(pos)
    # the aligned output: the model's k-mers, the room behind them untouched
    st, n = call(dtext.data_ptr(), K.KH_MEM_DEVICE, room.data_ptr(), pos.data_ptr())
    torch.cuda.synchronize()
    assert (st, n) == (K.KH_OK, m)
    assert np.array_equal(u64(room[:m]), ekm) and untouched(room[m:])
    if with_pos:
        assert np.array_equal(u32(pos[:m]), epos) and untouched(pos[m:])
    # a host output at the odd offset is staged: the model's k-mers
    hk, hp = host_odd(np.zeros((len(text), 2), dtype=np.uint64)), np.zeros(len(text), dtype=np.uint32)
    st, n = call(text.ctypes.data, K.KH_MEM_HOST, hk.ctypes.data, hp.ctypes.data)
    assert (st, n) == (K.KH_OK, m) and np.array_equal(hk[:m], ekm) and (not with_pos or np.array_equal(hp[:m], epos))


def test_hll_update_wide_refuses_a_misaligned_device_batch():
    keys = make_keys(9)
    h = hyperloglog64(12, 0, HASH, SEED)
    o = O.OracleHLL(12, 0, HID, SEED)
    h.update_wide(keys[:100]); o.update_via_hashval(O.hash16_batch(HID, SEED, keys[:100]))
    before = h.registers().copy()
    refused(h.update_wide, misaligned(keys))
    assert np.array_equal(h.registers(), before) and np.array_equal(before, o.registers())
    h.update_wide(misaligned(keys).clone()); o.update_via_hashval(O.hash16_batch(HID, SEED, keys))
    assert np.array_equal(h.registers(), o.registers())
    more = make_keys(10)
    h.update_wide(host_odd(more)); o.update_via_hashval(O.hash16_batch(HID, SEED, more))
    assert np.array_equal(h.registers(), o.registers())
    h.close()


# ---- the position index -------------------------------------------------------------------------------------------------------------
def index_state(x):
    return (x.size(), x.total(), x.capacity(), x.export_info().copy()) + tuple(a.copy() for a in x.export())


def same_state(a, b):
    return a[:3] == b[:3] and all(np.array_equal(p, q) for p, q in zip(a[3:], b[3:]))


def same_index(x, keys, pos):
    """the index against the model of the pairs given so far: sizes, the export per key, count and find of hits and misses"""
    m = WideSeqModel(keys, pos)
    assert (x.size(), x.total()) == (m.size(), m.total())
    k, off, p = x.export()
    eo, ep = m.export_in_key_order(k)
    assert np.array_equal(off, eo) and np.array_equal(p, ep)
    q = np.concatenate([keys[:300], make_keys(11)[:100]])
    for qq in (aligned(q), host_odd(q)):
        assert np.array_equal(u32(x.count(qq)), m.count(q))
        go, gp = x.find(qq)
        eo, ep = m.find(q)
        assert np.array_equal(u64(go), eo) and np.array_equal(u32(gp), ep)


def test_wide_index_refuses_misaligned_device_keys():
    L = K.lib()
    k1, k2 = make_keys(12), make_keys(13)
    p1, p2 = np.arange(N, dtype=np.uint32) * np.uint32(7), np.arange(N, dtype=np.uint32) + np.uint32(100000)
    dp1, dp2 = (torch.from_numpy(p.view(np.int32)).cuda() for p in (p1, p2))
    x = WideKmerPositionIndex(k=63, hash=HASH, seed=SEED)
    # build: refused on an empty index, which stays empty
    empty = index_state(x)
    err = refused(x.build, misaligned(k1), dp1)
    assert "16-byte aligned" in str(err)
    assert same_state(index_state(x), empty) and x.total() == 0
    x.build(misaligned(k1).clone(), dp1)
    same_index(x, k1, p1)
    # append, erase, count, find: refused on a built index, which keeps every byte
    built = index_state(x)
    bad = misaligned(k2)
    for fn, args in ((x.append, (bad, dp2)), (x.erase, (misaligned(k1),)), (x.count, (bad,)), (x.find, (bad,))):
        refused(fn, *args)
    nk, npos, n_out = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    cnt, offs, pos = sentinels(N, torch.int32), sentinels(N + 1, torch.int64), sentinels(4 * N, torch.int32)
    assert L.kh_wide_index_erase(x._h, misaligned(k1).data_ptr(), N, K.KH_MEM_DEVICE, C.byref(nk), C.byref(npos)) == KH_ERR_INVALID
    assert L.kh_wide_index_count(x._h, bad.data_ptr(), N, K.KH_MEM_DEVICE, cnt.data_ptr()) == KH_ERR_INVALID
    assert L.kh_wide_index_find(x._h, bad.data_ptr(), N, K.KH_MEM_DEVICE, offs.data_ptr(), pos.data_ptr(), 4 * N, C.byref(n_out)) == KH_ERR_INVALID
    torch.cuda.synchronize()
    assert (nk.value, npos.value, n_out.value) == (0, 0, 0) and untouched(cnt) and untouched(offs) and untouched(pos)
    assert same_state(index_state(x), built)
    same_index(x, k1, p1)
    # the same calls on aligned clones and on host views at the odd offset
    x.append(bad.clone(), dp2)
    same_index(x, np.concatenate([k1, k2]), np.concatenate([p1, p2]))
    gone = k1[:200]
    keep = ~(WideSeqModel(gone, np.zeros(len(gone), dtype=np.uint32)).count(np.concatenate([k1, k2])) > 0)
    m = WideSeqModel(np.concatenate([k1, k2]), np.concatenate([p1, p2]))
    assert x.erase(misaligned(gone).clone()) == (len(np.unique(gone, axis=0)), int(m.count(np.unique(gone, axis=0)).sum()))
    left_k, left_p = np.concatenate([k1, k2])[keep], np.concatenate([p1, p2])[keep]
    same_index(x, left_k, left_p)
    k3, p3 = make_keys(14), np.arange(N, dtype=np.uint32) + np.uint32(500000)
    x.append(host_odd(k3), p3)
    same_index(x, np.concatenate([left_k, k3]), np.concatenate([left_p, p3]))
    x.close()
