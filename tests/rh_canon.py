"""numpy model of the canonical Robin Hood layout.  TEST INFRASTRUCTURE ONLY; no GPU, no torch.

The info array of a Robin Hood table is a function of the key set and the capacity alone: the elements stand in
ascending order of their home bucket, each in the first slot at or after its home that the one before leaves free, circular.  So a
test can check the layout of a table whose key set it did not choose: export_info() == canonical_info(homes of to_vector(), cap).

Written apart from oracle/wide_model.py (which runs a (max,+) scan twice round the circle): here the circle is cut open behind a
slot that stays empty -- the slot at which the running sum of (keys per home - 1) is smallest -- and laid out once from there.
tests/test_rh_canon.py checks it against the 64-bit CPU oracle and against that model."""
import numpy as np


def canonical_info(homes, capacity):
    """homes: home bucket of every element (any order, any integer type) -> (info, overflow).
    info: uint8[capacity], 0x80 | distance in an occupied slot, 0 in an empty one.  overflow: some distance is above 127 (no table
    with a 7-bit distance field holds this key set at this capacity); the distances in `info` are then cut to 7 bits."""
    cap = int(capacity)
    h = np.sort(np.asarray(homes).astype(np.int64))
    info = np.zeros(cap, dtype=np.uint8)
    if len(h) == 0:
        return info, False
    assert len(h) <= cap and 0 <= h[0] and h[-1] < cap
    if len(h) == cap:
        start = 0                                                     # no empty slot: every slot is taken, any cut gives the distances
    else:
        excess = np.cumsum(np.bincount(h, minlength=cap) - 1)         # keys that want a slot up to s, minus the slots up to s
        start = (int(np.argmin(excess)) + 1) % cap                    # the slot behind the emptiest prefix: nothing runs into it
    r = np.sort((h - start) % cap)                                    # homes counted from the cut
    i = np.arange(len(r), dtype=np.int64)
    slot = i + np.maximum.accumulate(r - i)                           # slot = max(home, slot of the one before + 1)
    dist = slot - r
    if len(h) < cap:
        assert slot[-1] < cap, "the cut was not behind an empty slot"
    info[(slot + start) % cap] = 0x80 | (dist & 0x7F)
    return info, bool(dist.max() > 127)
