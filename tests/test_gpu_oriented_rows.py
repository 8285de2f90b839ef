"""GPU: kh_oriented_rows against its model (tests/orient_model.py) byte for byte, host and device memory: the lengths around the 8-byte
word and the 64-lane step at every source alignment (lo mod 8) -- the destination alignment follows from the rows before -- both
strands, both complement values, lo > hi, hi > n, random batches, and a cap_text that is too small."""
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
import orient_model as OM  # noqa: E402
from stream_checks import to_dev  # noqa: E402

LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257)


def text_of(n, seed):
    rng = np.random.RandomState(seed)
    return np.frombuffer(b"ACGTacgtNn!Z", dtype=np.uint8)[rng.randint(0, 12, size=n)].copy()


def grid_batch():
    text = text_of(3000, 1)
    lo, hi, rev = [], [], []
    for n in LENGTHS:
        for a in range(8):
            for r in (0, 1):
                lo.append(1000 + a); hi.append(1000 + a + n); rev.append(r)
    # lo > hi; hi > n (clamped); lo > n; the whole text; rev with more bits than bit 0
    lo += [50, 2990, 4000, 0, 10, 10]; hi += [40, 3100, 4100, 3000, 30, 30]; rev += [1, 1, 0, 1, 2, 255]
    return text, np.array(lo, dtype=np.uint32), np.array(hi, dtype=np.uint32), np.array(rev, dtype=np.uint8)


def random_batch(seed):
    rng = np.random.RandomState(seed)
    text = text_of(5000, seed)
    lo = rng.randint(0, 5200, size=300).astype(np.uint32)
    hi = (lo + rng.randint(-5, 400, size=300)).clip(0, 6000).astype(np.uint32)
    return text, lo, hi, rng.randint(0, 4, size=300).astype(np.uint8)


BATCHES = {"grid": grid_batch, "random_1": lambda: random_batch(1), "random_2": lambda: random_batch(2)}


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("complement", [True, False])
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_equals_the_model(name, complement, dev):
    text, lo, hi, rev = BATCHES[name]()
    eo, et = OM.oriented_rows(text, lo, hi, rev, complement)
    mk = to_dev if dev else (lambda x: x)
    offs, out = kh.oriented_rows(mk(text), mk(lo), mk(hi), mk(rev), complement)
    if dev:
        torch.cuda.synchronize()
        offs, out = offs.cpu().numpy(), out.cpu().numpy()
    assert [int(v) for v in offs.view(np.uint64)] == eo
    assert out.tobytes() == et
    if name == "grid" and complement:      # not vacuous: a reversed row differs from the forward one, N and '!' stay, the case is kept
        assert et != OM.oriented_rows(text, lo, hi, rev & 0, complement)[1] and et != OM.oriented_rows(text, lo, hi, rev, False)[1]


@pytest.mark.parametrize("dev", [False, True])
def test_a_short_cap_is_refused_with_the_count(dev):
    text, lo, hi, rev = random_batch(3)
    eo, et = OM.oriented_rows(text, lo, hi, rev, True)
    mk = to_dev if dev else (lambda x: x)
    ptr = (lambda t: t.data_ptr()) if dev else (lambda t: t.ctypes.data)
    host = (lambda t: t.cpu().numpy()) if dev else (lambda t: t)
    d = [mk(x) for x in (text, lo, hi, rev)]
    offs, out = mk(np.full(len(lo) + 1, 7, dtype=np.uint64)), mk(np.full(len(et), 0x55, dtype=np.uint8))
    n = C.c_uint64(99)
    args = (ptr(d[0]), len(text), ptr(d[1]), ptr(d[2]), ptr(d[3]), len(lo), 1, K.KH_MEM_DEVICE if dev else K.KH_MEM_HOST, ptr(offs))
    st = K.lib().kh_oriented_rows(*args, ptr(out), len(et) - 1, C.byref(n), 0, None)
    if dev:
        torch.cuda.synchronize()
    assert st == K.KH_ERR_INVALID and n.value == len(et)
    assert [int(v) for v in host(offs).view(np.uint64)] == eo and (host(out) == 0x55).all()
    st = K.lib().kh_oriented_rows(*args, None, 0, C.byref(n), 0, None)
    assert st == K.KH_OK and n.value == len(et)
    st = K.lib().kh_oriented_rows(*args, ptr(out), len(et), C.byref(n), 0, None)
    if dev:
        torch.cuda.synchronize()
    assert st == K.KH_OK and host(out).tobytes() == et
