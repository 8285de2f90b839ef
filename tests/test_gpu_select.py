"""GPU: kh_chain_select against the model of tests/select_model.py, bit for bit: all seven outputs, for host and for device memory.

One batch holds groups of 0, 1, 2, 3, 63, 64 chains (a wavefront per group), 65 and 200 (a workgroup, sorted and swept in LDS), one of
5000 -- past the LDS tile of 2048 chains (select_cases.TILE = KSEL_TILE), so it is radix-sorted and swept over scratch -- and a trailing
empty group: about 5.4e3 chains.  It runs under every score distribution with the interval shapes whose primaries are few (identical,
nested, random).  The model is quadratic in a group's primaries, so the two shapes that make most chains primary (disjoint, staircase)
take a 2100-chain group in its place -- still past the tile -- under two score distributions, and every distribution on the batch
without a large group."""
import ctypes as C
import functools
import itertools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import select_cases as SC  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
from select_model import NAMES, select_model  # noqa: E402
from stream_checks import to_dev  # noqa: E402

assert SC.BIG > SC.TILE and 2100 > SC.TILE
PAST_TILE = tuple(2100 if n == SC.BIG else n for n in SC.SIZES)
FEW, MANY = ("identical", "nested", "random"), ("disjoint", "staircase")


@functools.lru_cache(maxsize=None)
def case(sizes, score_kind, shape_kind):
    c = SC.batch(sizes, score_kind, shape_kind, seed=3)
    return c, select_model(*c)


def run(c, where, **kw):
    args = [to_dev(a) for a in c] if where == "device" else list(c)
    out = kh.select_chains(*args, **kw)
    return [x.cpu().numpy() if where == "device" else x for x in out]


def check(got, exp, what):
    for name, g, e in zip(NAMES, got, exp):
        g = g.view(e.dtype)
        assert g.shape == e.shape, (what, name)
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, "%s: %s differs at %s: got %s, expected %s" % (what, name, bad[:8], g[bad[:8]], e[bad[:8]])


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("shape_kind", FEW)
@pytest.mark.parametrize("score_kind", SC.SCORES)
def test_every_size_class(score_kind, shape_kind, where):
    c, exp = case(SC.SIZES, score_kind, shape_kind)
    assert 5000 < len(c[0]) < 7000
    check(run(c, where), exp, (score_kind, shape_kind, where))


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("shape_kind", MANY)
@pytest.mark.parametrize("score_kind", ["ties", "ascending"])
def test_many_primaries_past_the_tile(score_kind, shape_kind, where):
    c, exp = case(PAST_TILE, score_kind, shape_kind)
    assert (exp[3] & 1).sum() > 256                          # the list of primaries itself is longer than a batch of the sweep
    check(run(c, where), exp, (score_kind, shape_kind, where))


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("shape_kind", MANY)
@pytest.mark.parametrize("score_kind", SC.SCORES)
def test_many_primaries_up_to_the_tile(score_kind, shape_kind, where):
    c, exp = case(SC.SMALL_SIZES, score_kind, shape_kind)
    check(run(c, where), exp, (score_kind, shape_kind, where))


def test_every_parameter_triple():
    c, _ = case(SC.SMALL_SIZES, "ties", "random")
    for mask, pri, bn in itertools.product((0, 50, 100), (0, 80, 100), (0, 1, 5)):
        kw = dict(mask_pct=mask, pri_pct=pri, best_n=bn)
        exp = select_model(*c, **kw)
        for where in ("host", "device"):
            check(run(c, where, **kw), exp, (kw, where))


@pytest.mark.parametrize("n", [1, 40, 64, 65, 150, 2049])
def test_one_group_without_offsets(n):
    qs, qe, sc, cnt, _ = SC.batch((n,), "ties", "random", seed=11)
    exp = select_model(qs, qe, sc, cnt)
    assert len(exp[6]) == 1
    for where in ("host", "device"):
        check(run((qs, qe, sc, cnt), where), exp, (n, where))


def test_no_chains_in_device_memory():
    e = torch.zeros(0, dtype=torch.int32, device="cuda")
    c = kh.select_chains(e, e, e, e, torch.zeros(4, dtype=torch.int64, device="cuda"))
    assert c.best.cpu().tolist() == [-1, -1, -1] and all(x.numel() == 0 for x in c[:6])
    assert kh.select_chains(e, e, e, e).best.cpu().tolist() == [-1]


def test_a_second_call_gives_identical_bits():
    c, exp = case(SC.SIZES, "ties", "random")
    dev = [to_dev(a) for a in c]
    first = [x.cpu().numpy().tobytes() for x in kh.select_chains(*dev)]
    again = [x.cpu().numpy().tobytes() for x in kh.select_chains(*dev)]
    assert first == again


GUARD, FILL, PAD = 0xA5, 0x5A, 256


def test_garbage_offsets_in_device_memory_stay_inside_the_outputs():
    """offsets that are no ascending partition: the kernels clamp every group to [0, n); the status is KH_OK (nobody looked), the chains'
    outputs are unspecified, and the guard bands around all seven outputs come back unchanged"""
    c, _ = case(SC.SIZES, "ties", "random")
    n = len(c[0])
    rng = np.random.default_rng(9)
    offs = np.concatenate([np.array([0, 5000, 3, 2 ** 63, 100, n, 0, n + 5, 2 ** 32 + 1, 70, 2 ** 64 - 1, 64, 0], dtype=np.uint64),
                           rng.integers(0, 2 * n, 40).astype(np.uint64), np.array([17], dtype=np.uint64)])
    assert offs.dtype == np.uint64
    ng = len(offs) - 1
    ins = [to_dev(a) for a in c[:4]] + [to_dev(offs)]
    sizes = [(n, 4), (n, 4), (n, 1), (n, 1), (n, 4), (n, 4), (ng, 4)]
    bufs = []
    for count, width in sizes:
        raw = np.full(count * width + 2 * PAD, GUARD, dtype=np.uint8)
        raw[PAD:PAD + count * width] = FILL
        bufs.append(torch.from_numpy(raw).cuda())
    st = K.lib().kh_chain_select(*(t.data_ptr() for t in ins[:4]), n, ins[4].data_ptr(), ng, 50, 80, 5, K.KH_MEM_DEVICE,
                                 *(b.data_ptr() + PAD for b in bufs), 0, C.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    assert st == K.KH_OK
    torch.cuda.synchronize()
    for b, (count, width) in zip(bufs, sizes):
        raw = b.cpu().numpy()
        assert (raw[:PAD] == GUARD).all() and (raw[PAD + count * width:] == GUARD).all(), "guard words overwritten"
    # the same call with sound offsets afterwards is right: nothing the garbage left behind (scratch, pool) spoils it
    check(run(c, "device"), case(SC.SIZES, "ties", "random")[1], "after the garbage")
