"""Python-int statement of google/farmhash util::Hash64WithSeed for a 16-byte input (the HashLen0to16 branch for len >= 8), as
published in farmhash.cc (farmhashna).  TEST INFRASTRUCTURE ONLY: tests/test_wide_hash.py pins the kernels' header against it,
tests/test_wide_model.py the oracle's ora_hash16_batch."""
M64 = (1 << 64) - 1


def _rotr(x, r):
    return ((x >> r) | (x << (64 - r))) & M64


def _hashlen16(u, v, mul):
    a = ((u ^ v) * mul) & M64
    a ^= a >> 47
    b = ((v ^ a) * mul) & M64
    b ^= b >> 47
    return (b * mul) & M64


def farm_hash64_with_seed_16(w0, w1, seed):
    """farmhash Hash64WithSeed(s, 16, seed) = HashLen16(HashLen0to16(s, 16) - k2, seed): the len >= 8 branch with
    a = Fetch(s) + k2, b = Fetch(s + len - 8), mul = k2 + 2 len"""
    k2 = 0x9ae16a3b2f90404f
    mul = k2 + 32
    a = (w0 + k2) & M64
    b = w1
    c = (_rotr(b, 37) * mul + a) & M64
    d = ((_rotr(a, 25) + b) * mul) & M64
    h = _hashlen16(c, d, mul)
    return _hashlen16((h - k2) & M64, seed & M64, 0x9ddfea08eb382d69)
