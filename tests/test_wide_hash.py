"""CPU: the 16-byte hashes and the 128-bit k-mer helpers of include/kmerhash_amd/kh_hash.h (host build of the same header the kernels
use) against independent statements: the oracle's MurmurHash3 over 16-byte inputs (and SMHasher's, where that library builds), a Python
statement of farmhash Hash64WithSeed for len 16, identity = w0, and a Python-int statement of the reverse complement."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
SEEDS = (0, 43, 9876543)

PROG = r"""
#include <cstdio>
#include <cinttypes>
#include "kmerhash_amd/kh_hash.h"
int main() {
  unsigned long long a, b, s; unsigned k;
  while (scanf("%llu %llu %llu %u", &a, &b, &s, &k) == 4) {
    uint64_t r0 = 0, r1 = 0, c0 = a, c1 = b;
    if (k) { kh_revcomp128(a, b, k, &r0, &r1); kh_xf128(&c0, &c1, k); }
    printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n",
           kh_hash128<KHH_IDENTITY>(a, b, s), kh_hash128<KHH_MURMUR3_X86>(a, b, s), kh_hash128<KHH_MURMUR3_X64>(a, b, s),
           kh_hash128<KHH_FARM>(a, b, s), r0, r1, c0, c1);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def hashprog():
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tempfile.mkdtemp(prefix="kh_wide_hash_")
    src, exe = os.path.join(d, "h.cpp"), os.path.join(d, "h")
    open(src, "w").write(PROG)
    subprocess.check_call([cxx, "-O1", "-std=c++11", "-I", os.path.join(ROOT, "include"), "-o", exe, src])

    def run(rows):
        inp = "".join("%d %d %d %d\n" % r for r in rows)
        out = subprocess.run([exe], input=inp, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        return [tuple(int(x) for x in ln.split()) for ln in out.splitlines()]
    yield run
    shutil.rmtree(d, ignore_errors=True)


def _keys(n, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1 << 64, (n, 2), dtype=np.uint64, endpoint=False)
    k[:4] = [[0, 0], [M64, M64], [1, 0], [0, 1]]
    return [(int(a), int(b)) for a, b in k]


def _b16(w0, w1):
    return w0.to_bytes(8, "little") + w1.to_bytes(8, "little")


def test_wide_hashes_match_statements(hashprog):
    from oracle import oracle_py as O
    from oracle.farm16 import farm_hash64_with_seed_16      # (the Python statement of farmhash for 16 bytes, shared with the wide model's tests)
    keys = _keys(400, 5)
    for seed in SEEDS:
        got = hashprog([(a, b, seed, 0) for a, b in keys])
        for (a, b), g in zip(keys, got):
            assert g[0] == a                                               # identity: w0
            x86 = O.murmur3_x86_128(_b16(a, b), seed)
            assert g[1] == int(x86[0]) | (int(x86[1]) << 32), (a, b, seed)
            assert g[2] == int(O.murmur3_x64_128(_b16(a, b), seed)[0]), (a, b, seed)
            assert g[3] == farm_hash64_with_seed_16(a, b, seed), (a, b, seed)


def test_wide_murmur_matches_smhasher_where_it_builds(hashprog):
    from oracle import oracle_py as O
    try:
        O.smhasher()
    except Exception:             # (the independent SMHasher build is optional; the oracle comparison above always runs)
        return
    keys = _keys(200, 6)
    for seed in SEEDS:
        got = hashprog([(a, b, seed, 0) for a, b in keys])
        for (a, b), g in zip(keys, got):
            x86 = O.smhasher_x86_128(_b16(a, b), seed)
            assert g[1] == int(x86[0]) | (int(x86[1]) << 32)
            assert g[2] == int(O.smhasher_x64_128(_b16(a, b), seed)[0])


def test_eight_byte_and_sixteen_byte_forms_differ(hashprog):
    """the 16-byte forms hash 16 bytes: a key with w1 = 0 is not hashed like the 8-byte key w0 (except identity)"""
    from oracle import oracle_py as O
    got = hashprog([(12345, 0, 43, 0)])[0]
    x86_8 = O.murmur3_x86_128((12345).to_bytes(8, "little"), 43)
    assert got[1] != int(x86_8[0]) | (int(x86_8[1]) << 32)


def revcomp_py(v, k):
    r = 0
    for i in range(k):
        r = (r << 2) | (3 - ((v >> (2 * i)) & 3))
    return r


@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 47, 63, 64])
def test_revcomp128_and_canonical(hashprog, k):
    rng = np.random.default_rng(k)
    vals = [int.from_bytes(rng.bytes(16), "little") & ((1 << (2 * k)) - 1) for _ in range(200)]
    got = hashprog([(v & M64, v >> 64, 0, k) for v in vals])
    for v, g in zip(vals, got):
        rc = revcomp_py(v, k)
        assert (g[4] | (g[5] << 64)) == rc, (k, v)
        assert (g[6] | (g[7] << 64)) == min(v, rc), (k, v)
