"""tests/rh_canon.py (the numpy model of the canonical Robin Hood layout that tests/test_gpu_refusals.py judges tables by) against
both CPU oracles, without a GPU: the 64-bit oracle table under the identity hash (OracleTable(0, ..., hash identity): info bytes as
its own single-key inserts leave them, and its probe_overflow flag) and oracle/wide_model.py (rh_info_model / rh_max_distance).
The model was checked against both; info bytes and the overflow flag agree in every case below.

Where a layout does not exist (a distance above 127) only the flag is compared: the oracle, like the reference under NDEBUG,
goes on with a wrapped distance, and rh_info_model asserts."""
import numpy as np
import pytest

from oracle.wide_model import rh_info_model, rh_max_distance
from rh_canon import canonical_info

CAPS = [128, 4096, 16384]


def spread(n, seed):
    """n distinct 64-bit keys with uniform low bits"""
    k = np.unique(np.random.default_rng(seed).integers(0, 1 << 63, 2 * n + 16, dtype=np.uint64))
    return k[np.random.default_rng(seed + 1).permutation(len(k))][:n]


def pile(home, m, first=1):
    """m keys whose home bucket under the identity hash is `home` at every capacity up to 2^32"""
    return np.uint64(home) + (np.arange(first, first + m, dtype=np.uint64) << np.uint64(32))


def agree(oracle, keys, cap):
    """the model, the 64-bit oracle and the wide model on one key set at one capacity -> (info, overflow)"""
    keys = keys[np.random.default_rng(len(keys)).permutation(len(keys))]
    homes = keys & np.uint64(cap - 1)
    info, overflow = canonical_info(homes, cap)
    assert overflow == (rh_max_distance(homes.astype(np.int64), cap) >= 128)
    o = oracle.OracleTable(0, cap, 0.0, 1.0, oracle.HASH_IDENTITY, 43)      # max load 1.0: no insert below `cap` keys doubles
    assert o.insert(keys, np.zeros(len(keys), dtype=np.uint32)) == len(keys) and o.capacity() == cap
    assert o.probe_overflow() == overflow
    if not overflow:
        assert np.array_equal(info, rh_info_model(homes.astype(np.int64), cap))
        assert np.array_equal(info, o.export_info())
        assert int((info >= 0x80).sum()) == len(keys)
    o.close()
    return info, overflow


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("load", [0.3, 0.8])
def test_spread_keys(oracle, cap, load):
    info, overflow = agree(oracle, spread(int(cap * load), 7 + cap), cap)
    assert not overflow


def test_empty_and_single():
    info, overflow = canonical_info(np.zeros(0, dtype=np.uint64), 128)
    assert not overflow and not info.any()
    info, overflow = canonical_info([5], 128)
    assert not overflow and info[5] == 0x80 and int(info.astype(bool).sum()) == 1


# (129 keys have no room among 128 buckets at all; 128 keys fill them: distances 0..127 in a table without an empty slot)
@pytest.mark.parametrize("cap,m", [(c, m) for c in CAPS for m in (1, 127, 128, 129) if m <= c])
def test_one_pile(oracle, cap, m):
    """m keys of one home bucket, on a spread background where there is room for one: the last stands at distance m - 1; 128 is the
    most a table takes"""
    home = cap // 2 + 3
    bg = spread(cap // 4, 11)
    bg = bg[((bg & np.uint64(cap - 1)).astype(np.int64) - home) % cap >= 300] if cap > 512 else bg[:0]      # the pile's slots stay its own
    info, overflow = agree(oracle, np.concatenate([bg, pile(home, m)]), cap)
    assert overflow == (m > 128)
    if not overflow:
        assert info[(home + m - 1) % cap] == 0x80 | (m - 1)
        if m == 128:
            assert info[(home + 127) % cap] == 0xFF


@pytest.mark.parametrize("cap", [4096, 16384])
def test_two_piles_overflow_only_together(oracle, cap):
    """100 keys at home h and 100 at h + 55: each alone reaches distance 99, together the second reaches 100 + 100 - 55 - 1 = 144;
    with 80 in the first the largest distance is 124"""
    h = cap // 2 - 50
    a, b = pile(h, 100), pile(h + 55, 100)
    assert not agree(oracle, a, cap)[1] and not agree(oracle, b, cap)[1]
    assert agree(oracle, np.concatenate([a, b]), cap)[1]
    info, overflow = agree(oracle, np.concatenate([a[:80], b]), cap)
    assert not overflow and int((info[info >= 0x80] & 0x7F).max()) == 124


@pytest.mark.parametrize("cap,m", [(c, m) for c in CAPS for m in (100, 120, 140) if m + 8 <= c])
def test_pile_that_wraps(oracle, cap, m):
    """a pile at cap - 60 runs over the last slot into slot 0 and pushes what lives there"""
    front = np.concatenate([pile(0, 3, 1000), pile(2, 2, 2000)])      # elements at the start of the table, in the pile's way
    info, overflow = agree(oracle, np.concatenate([front, pile(cap - 60, m)]), cap)
    assert overflow == (m > 128)
    if not overflow:
        assert info[cap - 1] == 0x80 | 59 and info[0] == 0x80 | 60        # the pile goes on from the last slot to slot 0
        assert info[(m - 60) % cap] == 0x80 | (m - 60)                     # the first element of home 0 stands behind the pile
