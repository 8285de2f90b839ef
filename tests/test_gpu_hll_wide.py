"""GPU: HyperLogLog over 16-byte keys (kh_hll_update_wide) and the fused text -> registers pass (kh_hll_update_from_sequence /
_from_fastq, k = 1..64): registers bit-exact against the reference hyperloglog64 / the oracle fed the CPU hashes of the CPU k-mers,
the fused pass against the two-step route (front end + update) across the persistent loop, the estimate's quality, and the
pre-sizing of KmerCounter and of benchmark/kmer_counter.py --estimate-reserve."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import kmers as KM  # noqa: E402
from kmerhash_amd._capi import KH_ERR_INVALID, KhError  # noqa: E402
from kmerhash_amd.hll import hyperloglog64  # noqa: E402
from oracle import oracle_py as O  # noqa: E402
from oracle.kmers_np import np_kmers  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASHES = (("identity", O.HASH_IDENTITY), ("murmur3avx64", O.HASH_MURMUR3_X86), ("murmur", O.HASH_MURMUR3_X64), ("farm", O.HASH_FARM))


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def np_kmers128(seq, k, canonical):
    """the 128-bit k-mer statement, 32 < k <= 64 (numpy): windows of k valid bases (ACGT, either case), first base most significant,
    A0 C1 G2 T3, V stored as {w0 = V mod 2^64, w1 = V >> 64}; canonical = min(V, revcomp_k(V)) as 128-bit integers -> (n, 2) uint64"""
    code = np.full(256, 4, dtype=np.uint8)
    for ch, c in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
        code[ch] = c
    c = code[np.asarray(seq, dtype=np.uint8)]
    n = len(c)
    if n < k:
        return np.zeros((0, 2), dtype=np.uint64)
    m = n - k + 1
    bad = np.concatenate([[0], np.cumsum(c > 3)])
    ok = (bad[k:] - bad[:m]) == 0
    cc = (c & 3).astype(np.uint64)
    f0, f1, r0, r1 = (np.zeros(m, dtype=np.uint64) for _ in range(4))
    two, top = np.uint64(2), np.uint64(62)
    for j in range(k):
        b = cc[j: m + j]
        f1 = (f1 << two) | (f0 >> top)
        f0 = (f0 << two) | b
        if 2 * j < 64:
            r0 |= (np.uint64(3) - b) << np.uint64(2 * j)
        else:
            r1 |= (np.uint64(3) - b) << np.uint64(2 * j - 64)
    if k < 64:
        f1 &= np.uint64((1 << (2 * k - 64)) - 1)
    if canonical:
        fw = (f1 < r1) | ((f1 == r1) & (f0 <= r0))
        f0, f1 = np.where(fw, f0, r0), np.where(fw, f1, r1)
    return np.ascontiguousarray(np.stack([f0, f1], axis=1)[ok])


def test_np_kmers128_statement_against_python_ints():
    """the numpy statement above against plain Python integers on a short text"""
    # 300 random bases, either case, cut by an N, a newline and an N into valid runs of 100, 79, 69 and 49:
    # 59 windows of k = 64 (37 + 16 + 6 + 0) and 169 of k = 33 (68 + 47 + 37 + 17)
    rng = np.random.default_rng(33)
    t = np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.integers(0, 8, 300)].copy()
    t[[100, 250]] = ord("N")
    t[180] = 10
    seq = t.tobytes()
    code = {ord(a): i % 4 for i, a in enumerate("ACGTacgt")}
    for k in (33, 64):
        for canonical in (False, True):
            exp = []
            for s in range(len(seq) - k + 1):
                w = seq[s:s + k]
                if all(b in code for b in w):
                    v = 0
                    for b in w:
                        v = (v << 2) | code[b]
                    rc = 0
                    for i in range(k):
                        rc = (rc << 2) | (3 - ((v >> (2 * i)) & 3))
                    v = min(v, rc) if canonical else v
                    exp.append([v & ((1 << 64) - 1), v >> 64])
            got = np_kmers128(np.frombuffer(seq, dtype=np.uint8), k, canonical)
            assert len(exp) == {33: 169, 64: 59}[k] and got.tolist() == exp


# ---- 1. update_wide pinned to the reference -------------------------------------------------------------------------------------
def wide_keys():
    rng = np.random.default_rng(16)
    k = rng.integers(0, 1 << 63, size=(5000, 2), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(5000, 2), dtype=np.uint64)
    x, ones = np.uint64(0x0123456789ABCDEF), np.uint64(0xFFFFFFFFFFFFFFFF)
    edge = np.array([[0, 0], [ones, ones], [x, 0], [0, x]], dtype=np.uint64)
    return np.ascontiguousarray(np.concatenate([k, edge]))


@pytest.mark.parametrize("hname,hid", HASHES)
def test_update_wide_matches_reference_and_oracle(hname, hid):
    keys = wide_keys()
    hv = O.hash16_batch(hid, 43, keys)
    exp = O.OracleHLL(12, 0, hid, 43)
    exp.update_via_hashval(hv)
    refs = [exp.registers()]
    if O.ref_hll_available():
        r = O.RefHLL(0, hid, 43)
        r.update_via_hashval(hv)
        refs.append(r.registers())
    for feed in (lambda h: h.update_wide(keys), lambda h: h.update_wide(dev(keys)),
                 lambda h: (h.update_wide(keys[:1234]), h.update_wide(dev(keys[1234:])))):
        h = hyperloglog64(12, 0, hname, 43)
        feed(h)
        got = h.registers()
        for ref in refs:
            assert np.array_equal(got, ref)
        assert h.estimate() == exp.estimate()
        h.close()
    # the contract in the library's own terms: update_via_hashval of kh_wide_hash_batch
    a, b = hyperloglog64(12, 0, hname, 43), hyperloglog64(12, 0, hname, 43)
    a.update_wide(dev(keys)); b.update_via_hashval(kh.hash_batch_wide(dev(keys), hname, 43))
    assert np.array_equal(a.registers(), b.registers())
    a.close(); b.close()


@pytest.mark.parametrize("precision,ignore_msb", [(14, 0), (12, 5), (14, 5), (13, 1), (4, 0)])
def test_update_wide_other_precisions_and_ignored_bits(precision, ignore_msb):
    keys = wide_keys()
    for hname, hid in HASHES[1:]:
        o = O.OracleHLL(precision, ignore_msb, hid, 43)
        o.update_via_hashval(O.hash16_batch(hid, 43, keys))
        h = hyperloglog64(precision, ignore_msb, hname, 43)
        h.update_wide(dev(keys[:3000])); h.update_wide(keys[3000:])
        assert np.array_equal(h.registers(), o.registers()) and h.estimate() == o.estimate()
        h.close()


def test_update_wide_empty_and_misaligned():
    keys = wide_keys()
    h = hyperloglog64(12, 0, "murmur", 43)
    h.update_wide(np.zeros((0, 2), dtype=np.uint64))
    h.update_wide(torch.empty((0, 2), dtype=torch.int64, device="cuda"))
    assert not h.registers().any()
    h.update_wide(keys[:100])
    before = h.registers()
    flat = dev(keys).reshape(-1)
    assert flat.data_ptr() % 16 == 0
    off = flat[1:2001].view(1000, 2)                  # a device pointer 8 bytes past a 16-byte boundary: refused before any launch
    assert off.data_ptr() % 16 == 8
    with pytest.raises(KhError) as e:
        h.update_wide(off)
    assert e.value.status == KH_ERR_INVALID
    assert np.array_equal(h.registers(), before)
    with pytest.raises(ValueError):
        h.update_wide(np.zeros(6, dtype=np.uint64))
    h.close()


# ---- 2. the fused pass pinned to the CPU ------------------------------------------------------------------------------------------
def cpu_registers(seq, k, canonical, hid, precision=12, ignore_msb=0):
    """(registers of the oracle fed the CPU hashes of the CPU k-mers, number of k-mers)"""
    o = O.OracleHLL(precision, ignore_msb, hid, 43)
    if k <= 32:
        km = np_kmers(seq, k, canonical)
        o.update_via_hashval(O.hash_batch(hid, 43, km))
    else:
        km = np_kmers128(seq, k, canonical)
        o.update_via_hashval(O.hash16_batch(hid, 43, km))
    return o.registers(), len(km)


def three_tile_text():
    n = 2 * 4096 + 100
    rng = np.random.default_rng(2)
    t = np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.integers(0, 8, n)].copy()
    t[rng.random(n) < 0.01] = ord("N")
    t[150::151] = 10
    return t


@pytest.fixture(scope="module")
def text3():
    t = three_tile_text()
    buf = torch.zeros(len(t) + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return t, buf


@pytest.mark.parametrize("canonical", [True, False])
@pytest.mark.parametrize("k", [1, 31, 32, 33, 63, 64])
def test_fused_pass_matches_cpu(text3, k, canonical):
    t, buf = text3
    hname, hid = HASHES[1 + k % 3]                                    # every hash takes part over the k's
    exp, n_exp = cpu_registers(t, k, canonical, hid)
    assert n_exp > 0 and exp.any()
    for o in (1, 7):                                                  # device slices off the 16-byte grid: the packer's byte-wise path
        buf[o:o + len(t)] = torch.from_numpy(t).cuda()
        s = buf[o:o + len(t)]
        assert s.data_ptr() % 16 == o
        h = hyperloglog64(12, 0, hname, 43)
        assert h.update_from_sequence(s, k, canonical) == n_exp
        assert np.array_equal(h.registers(), exp)
        h.close()
    for x in (t, dev(t)):
        h = hyperloglog64(12, 0, hname, 43)
        assert h.update_from_sequence(x, k, canonical) == n_exp
        assert np.array_equal(h.registers(), exp)
        # a text shorter than k, and an empty one: nothing changes
        assert h.update_from_sequence(x[:k - 1], k, canonical) == 0
        assert h.update_from_sequence(x[:0], k, canonical) == 0
        assert np.array_equal(h.registers(), exp)
        h.close()
    # the global-atomic branch (precision 14) and ignored bits
    exp14, _ = cpu_registers(t, k, canonical, hid, 14, 5)
    h = hyperloglog64(14, 5, hname, 43)
    assert h.update_from_sequence(dev(t), k, canonical) == n_exp
    assert np.array_equal(h.registers(), exp14)
    h.close()


def test_fused_pass_refuses_bad_arguments():
    t = three_tile_text()
    h = hyperloglog64(12, 0, "farm", 43)
    for k in (0, 65):
        for fn in (h.update_from_sequence, h.update_from_fastq):
            with pytest.raises(KhError) as e:
                fn(t, k)
            assert e.value.status == KH_ERR_INVALID
    assert not h.registers().any()
    h.close()


# ---- 3. the fused pass equals the two-step route across the persistent loop ------------------------------------------------------
def random_bases(n, seed):
    rng = np.random.default_rng(seed)
    t = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    t[rng.random(n) < 0.002] = ord("N")
    t[rng.integers(0, n, n // 180)] = 10
    return t


@pytest.mark.parametrize("k", [31, 63])
def test_fused_pass_equals_two_steps_over_the_persistent_loop(k):
    h = hyperloglog64(12, 0, "farm", 43)
    grid_max = h.text_grid(1 << 40)                                   # the largest grid the host code launches on this device
    n = (2 * grid_max + 3) * h.TEXT_TILE + 1234                       # every workgroup gets two tiles, three get a third, the last is ragged
    assert h.text_grid(n) == grid_max and n // h.TEXT_TILE >= 2 * grid_max
    t = dev(random_bases(n, k))
    km = (KM.kmers_from_sequence if k <= 32 else kh.kmers128_from_sequence)(t, k, True)
    two = hyperloglog64(12, 0, "farm", 43)
    (two.update if k <= 32 else two.update_wide)(km)
    assert h.update_from_sequence(t, k, True) == len(km) > n // 2
    assert np.array_equal(h.registers(), two.registers())
    h.close(); two.close()


@pytest.mark.parametrize("k", [31, 63])
def test_fused_fastq_equals_two_steps(k):
    fq = KM.synthetic_fastq_fixed(2000, 150, 100_000, seed=5)
    for x in (fq, dev(fq)):
        km = (KM.kmers_from_fastq if k <= 32 else kh.kmers128_from_fastq)(x, k, True)
        two = hyperloglog64(12, 0, "murmur", 43)
        (two.update if k <= 32 else two.update_wide)(km)
        h = hyperloglog64(12, 0, "murmur", 43)
        assert h.update_from_fastq(x, k, True) == len(km) > 1000 * (150 - k)
        assert np.array_equal(h.registers(), two.registers())
        # the estimator accumulates: a second, different batch on top, through the other route
        fq2 = KM.synthetic_fastq_fixed(500, 150, 100_000, seed=6)
        h.update_from_fastq(fq2, k, True)
        km2 = (KM.kmers_from_fastq if k <= 32 else kh.kmers128_from_fastq)(fq2, k, True)
        (two.update if k <= 32 else two.update_wide)(km2)
        assert np.array_equal(h.registers(), two.registers())
        h.close(); two.close()


# ---- 4. estimate quality and pre-sizing -------------------------------------------------------------------------------------------
# synthetic_fastq(40000, 150, 300000): 6e6 bases over a 3e5 genome, so nearly every genome k-mer occurs.  Worked out on the CPU (numpy
# k-mers, OracleHLL farm / seed 43 / precision 12, the oracle table's reserve) before these numbers were fixed:
#   k = 31: 299 946 distinct, estimate 292 466.7 (2.5 % low), reserve(estimate x 1.01625) -> capacity 524 288 = 1.398 x distinct / 0.8
#   k = 63: 299 903 distinct, estimate 292 033.0 (2.6 % low), reserve(estimate x 1.01625) -> capacity 524 288 = 1.399 x distinct / 0.8
# The capacity is a power of two: the estimate would have to be 30 % low (20 standard errors) to reserve 2^18 < distinct / max_load.
@pytest.fixture(scope="module")
def fastq40k():
    return np.frombuffer(KM.synthetic_fastq(40000, 150, 300000), dtype=np.uint8)


@pytest.mark.parametrize("k", [63, 31])
def test_estimate_quality_and_presizing(fastq40k, k):
    text = dev(fastq40k)
    plain = KM.KmerCounter(k)
    n_kmers = plain.add_fastq(text)
    distinct = plain.table.size()
    assert distinct > 250_000
    h = hyperloglog64(12, 0, "farm", 43)
    assert h.update_from_fastq(text, k) == n_kmers
    est = h.estimate()
    print("k=%d distinct=%d estimate=%.1f rel_err=%.4f" % (k, distinct, est, abs(est - distinct) / distinct))
    assert abs(est - distinct) < 0.08 * distinct
    h.close()

    kc = KM.KmerCounter(k, reserve_from_estimate=True)
    assert kc.table.capacity() == 128
    assert kc.presize_fastq(text) == est
    cap = kc.table.capacity()
    print("k=%d capacity=%d distinct/max_load=%.1f" % (k, cap, distinct / 0.8))
    assert cap >= distinct / 0.8
    assert kc.add_fastq(text) == n_kmers
    assert kc.table.capacity() == cap
    a, b = kc.table.sorted_items(), plain.table.sorted_items()
    assert len(a[0]) == distinct and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # sequence lines through add_sequences / presize_sequences: the same k-mers
    seqs = KM.sequences_from_fastq(fastq40k)
    ks = KM.KmerCounter(k, reserve_from_estimate=True)
    assert ks.presize_sequences(seqs) == est
    assert ks.add_sequences(seqs) == n_kmers and ks.table.capacity() == cap and ks.table.size() == distinct
    for c in (plain, kc, ks):
        c.close()


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("k", [63, 31])
def test_kmer_counter_estimate_reserve(k):
    env = {a: b for a, b in os.environ.items() if a != "KH_DIST_FORCE_COLLECTIVES"}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "benchmark", "kmer_counter.py"), "-k", str(k), "--estimate-reserve", "--verify",
                        "--reads", "20000", "--genome", "200000", "--batches", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=500, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    er = d["estimate_reserve"]
    print(er)
    assert d["ok"] and d["verify"]["ok"] and d["k"] == k
    assert er["rel_err"] < 0.08 and er["distinct"] == d["distinct_global"] == d["verify"]["expected_distinct"]
    assert er["capacity"] >= er["distinct"] / 0.8 and er["capacity"] == d["capacity_per_batch_rank0"][-1]
