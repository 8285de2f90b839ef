"""GPU: the 128-bit k-mer front end (kh_kmers128_*, k <= 64) against a Python-int statement of the definition (first base most
significant, A0 C1 G2 T3, V stored as w0 = V mod 2^64, w1 = V >> 64, canonical = min(V, revcomp_k(V))), and KmerCounter for k > 32.
kmerind's own packing is absent from the reference tree: PARITY UNPINNED."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import kmers as KM  # noqa: E402

CODE = {ord(c): i for i, c in enumerate("ACGT")}
CODE.update({ord(c): i for i, c in enumerate("acgt")})
M64 = (1 << 64) - 1


def revcomp(v, k):
    r = 0
    for i in range(k):
        r = (r << 2) | (3 - ((v >> (2 * i)) & 3))
    return r


def py_kmers(seq, k, canonical):
    out = []
    run = []
    for b in bytes(seq) + b"\n":
        if b in CODE:
            run.append(CODE[b])
            continue
        for s in range(len(run) - k + 1):
            v = 0
            for c in run[s:s + k]:
                v = (v << 2) | c
            out.append(min(v, revcomp(v, k)) if canonical else v)
        run = []
    return out


def as_wide(vs):
    return np.array([[v & M64, v >> 64] for v in vs], dtype=np.uint64).reshape(-1, 2)


def random_seq(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGTNacgtn\n", dtype=np.uint8)[rng.choice(11, n, p=[.24, .24, .24, .24, .005, .005, .005, .005, .005, .005, .01])].copy()


def fastq_text(reads):
    return "".join("@r%d\n%s\n+\n%s\n" % (i, r, "I" * len(r)) for i, r in enumerate(reads)).encode()


@pytest.mark.parametrize("k", [1, 21, 31, 32])
@pytest.mark.parametrize("canonical", [False, True])
def test_k_up_to_32_matches_the_64bit_front_end(k, canonical):
    seq = random_seq(30_000, k)
    got = kh.kmers128_from_sequence(seq, k, canonical)
    exp = KM.kmers_from_sequence(seq, k, canonical)
    assert np.array_equal(got[:, 0], exp) and not got[:, 1].any()
    fq = np.frombuffer(fastq_text(["ACGT" * 30, "GGATCCNNACGT" * 10, "AC"]), dtype=np.uint8)
    got = kh.kmers128_from_fastq(fq, k, canonical)
    exp = KM.kmers_from_fastq(fq, k, canonical)
    assert np.array_equal(got[:, 0], exp) and not got[:, 1].any()


@pytest.mark.parametrize("k", [33, 47, 63, 64])
@pytest.mark.parametrize("canonical", [False, True])
def test_wide_kmers_match_python_statement(k, canonical):
    seq = random_seq(12_000, 100 + k)
    exp = as_wide(py_kmers(seq, k, canonical))
    assert np.array_equal(kh.kmers128_from_sequence(seq, k, canonical), exp)
    got_d = kh.kmers128_from_sequence(torch.from_numpy(seq).cuda(), k, canonical)
    assert np.array_equal(got_d.cpu().numpy().view(np.uint64), exp)
    for m in (0, k - 1, k, k + 1, 4095, 4096, 4096 + k, 4097 + k):           # tile boundaries, inputs shorter than k
        assert np.array_equal(kh.kmers128_from_sequence(seq[:m], k, canonical), as_wide(py_kmers(seq[:m], k, canonical)))
    # N runs
    nrun = np.frombuffer(b"ACGT" * 40 + b"N" * 70 + b"TTGCA" * 30 + b"n" + b"G" * 80, dtype=np.uint8)
    assert np.array_equal(kh.kmers128_from_sequence(nrun, k, canonical), as_wide(py_kmers(nrun, k, canonical)))
    # FASTQ: sequence lines only, reads shorter than k yield nothing, k-mers never span reads
    rng = np.random.default_rng(k)
    reads = ["".join("ACGTN"[c] for c in rng.choice(5, int(rng.integers(1, 180)), p=[.245, .245, .245, .245, .02])) for _ in range(60)]
    fq = fastq_text(reads)
    exp = as_wide([v for r in reads for v in py_kmers(r.encode(), k, canonical)])
    assert np.array_equal(kh.kmers128_from_fastq(np.frombuffer(fq, dtype=np.uint8), k, canonical), exp)
    got_d = kh.kmers128_from_fastq(torch.from_numpy(np.frombuffer(fq, dtype=np.uint8).copy()).cuda(), k, canonical)
    assert np.array_equal(got_d.cpu().numpy().view(np.uint64), exp)


def test_kmer_counter_k63(tmp_path):
    rng = np.random.default_rng(63)
    genome = "".join("ACGT"[c] for c in rng.integers(0, 4, 5000))
    reads = []
    for _ in range(400):
        s = int(rng.integers(0, len(genome) - 150))
        reads.append(genome[s:s + 150])
    fq = fastq_text(reads)
    kc = KM.KmerCounter(k=63, canonical=True)
    kc.add_fastq(np.frombuffer(fq, dtype=np.uint8))
    kc.add_sequences(np.frombuffer(("\n".join(reads[:50]) + "\n").encode(), dtype=np.uint8))
    exp = collections.Counter(v for r in reads + reads[:50] for v in py_kmers(r.encode(), 63, True))
    k, v = kc.counts()
    got = {int(a) | (int(b) << 64): int(c) for (a, b), c in zip(k.tolist(), v.tolist())}
    assert got == dict(exp)
    path = tmp_path / "counts.bin"
    assert kc.write(str(path)) == len(exp)
    raw = np.fromfile(str(path), dtype=np.dtype([("kmer", "<u8", (2,)), ("count", "<u2")]))
    assert raw.dtype.itemsize == 18
    assert {int(a) | (int(b) << 64): int(c) for (a, b), c in zip(raw["kmer"].tolist(), raw["count"].tolist())} == dict(exp)
    kc.close()
