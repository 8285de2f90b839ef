"""The before/after checks of a refused call, shared by tests/test_gpu_refusals.py and tests/test_gpu_parity.py.  TEST INFRASTRUCTURE ONLY.

snapshot(t) / assert_unchanged(t, snap): a refused call leaves size, capacity, load thresholds, info bytes, keys and values as they
were.  assert_consistent(t): a table whose key set the test did not choose is a Robin Hood table of the keys it holds, judged by the
layout model of tests/rh_canon.py (identity hash)."""
import numpy as np

from rh_canon import canonical_info


def thresholds(t):
    return t.load_thresholds() if hasattr(t, "load_thresholds") else (t.get_min_load_factor(), t.get_max_load_factor())


def snapshot(t):
    k, v = t.sorted_items()
    return dict(size=t.size(), capacity=t.capacity(), thresholds=thresholds(t), info=t.export_info().copy(), keys=k.copy(), vals=v.copy())


def host_count(t, keys):
    c = t.count(keys)
    return np.asarray(c.cpu() if hasattr(c, "cpu") else c)


def assert_unchanged(t, snap, new_keys=None):
    assert t.size() == snap["size"]
    assert t.capacity() == snap["capacity"]
    assert thresholds(t) == snap["thresholds"]
    assert np.array_equal(t.export_info(), snap["info"]), "info bytes changed by a refused call"
    k, v = t.sorted_items()
    assert np.array_equal(k, snap["keys"]), "key set changed by a refused call"
    assert np.array_equal(v, snap["vals"]), "values changed by a refused call"
    if len(snap["keys"]):
        assert host_count(t, snap["keys"]).all()
    if new_keys is not None and len(new_keys):
        assert not host_count(t, new_keys).any()


def homes_of(t, keys):
    if keys.ndim == 2:
        import kmerhash_amd as kh
        return kh.hash_batch_wide(keys, "identity", 43) & np.uint64(t.capacity() - 1)
    return keys & np.uint64(t.capacity() - 1)


def assert_consistent(t):
    """size == items, the info array is the canonical one of the held keys, every held key is found with its value (identity hash)"""
    k, v = t.to_vector()
    assert t.size() == len(k)
    info, overflow = canonical_info(homes_of(t, k), t.capacity())
    assert not overflow
    assert np.array_equal(t.export_info(), info), "not the canonical Robin Hood layout of the held keys"
    if len(k):
        fv, ff = t.find_values(k)
        assert np.asarray(ff).all() and np.array_equal(np.asarray(fv).view(np.uint32), v)
