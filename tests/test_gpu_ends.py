"""GPU: kh_chain_ends against the model of tests/ends_model.py, bit for bit: the four numbers, offsets and ops of every row, for host
arrays and for CUDA tensors.  The ends are built by hand (tests/ends_cases.py) on a reference of 4 000 random bases with k = 15: both
ends on both strands (the four readers), ends of 0, 1, 7, 8, 9 and 64 bases, seeds within 8 bytes of either end of either text, a
reference that runs out, 31 and 32 edits, N on either side, lower case, garbage indices and intervals behind guard words, no chains,
count-only then emit, a cap that is too small and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi  # noqa: E402
import ends_model as EM  # noqa: E402
from ends_cases import Ends, K, sub  # noqa: E402
from stream_checks import to_dev  # noqa: E402

NAMES = ("q", "r", "edits", "clip", "offsets", "ops")


def ins(p, b=b"G"):
    return lambda s: s[:p] + b + s[p:]


def dele(p):
    return lambda s: s[:p] + s[p + 1:]


def subs(*at):
    return lambda s: sub(s, *at)


def build(ref_base=0):
    B = Ends(11, 4000, ref_base)
    rng = B.rng
    for p in (1000, 1003, 2500):                                   # N in B: seeds are put next to these
        B.ref[p] = ord("N")
    B.ref[3000:3100] = bytes(B.ref[3000:3100]).lower()             # lower-case reference
    B.add(6, 5, 12, 0)                                             # first read: the head reads qtext[0:5] and rtext[0:6] downwards, byte by byte
    B.add(3, 9, 9, 1)                                              # reverse tail runs out of reference after 3 bases
    for rev in (0, 1):
        for h, t in ((0, 1), (1, 0), (7, 8), (8, 9), (9, 7), (64, 64), (0, 0)):      # exact ends of the lengths that matter to an 8-byte compare
            B.add(rng.randrange(100, 3800), h, t, rev)
        B.add(500, 30, 30, rev, head=subs(14), tail=subs(15))                        # one substitution, well inside
        B.add(600, 30, 30, rev, head=subs(2), tail=subs(27))                         # ... 3 bases from the far end: clips at cost >= 4 (the tie), not below
        B.add(700, 30, 30, rev, head=subs(3), tail=subs(26))                         # ... 4 from it: extends at cost 4 too
        B.add(800, 40, 40, rev, head=ins(20), tail=ins(20, b"TT"))
        B.add(900, 40, 40, rev, head=dele(20), tail=dele(19))
        B.add(1200, 40, 40, rev, head=ins(0), tail=ins(40))                          # an insertion as the read's very first / last base
        B.add(990, 12, 12, rev)                                                      # N in B on both sides (1000 and 1003 forward of the seed, none behind)
        B.add(1004, 12, 12, rev)
        B.add(2500 - 20 - K, 8, 40, rev)
        B.add(1500, 20, 20, rev, head=lambda s: s[:9] + b"N" + s[10:], tail=lambda s: s[:9] + b"n" + s[10:])      # N in A
        B.add(3020, 25, 25, rev, head=bytes.lower, tail=lambda s: sub(s, 7).lower())                            # lower case on both sides
        B.add(1700, 64, 66, rev, head=subs(*range(1, 63, 2)), tail=subs(*range(2, 64, 2)))                      # exactly 31 edits: reached
        B.add(1900, 66, 64, rev, head=subs(*range(1, 65, 2)), tail=subs(*range(0, 64, 2)))                      # 32: one more than any max_edits
        B.add(5, 20, 20, rev)                                      # the reference runs out before the read does (5 bases before the seed)
        B.add(4000 - K - 6, 20, 20, rev)                           # ... and 6 behind it; rtext is read upwards byte by byte
        B.add(4000 - K, 3, 3, rev)
        B.add(0, 3, 3, rev)
    for _ in range(12):                                            # random ends with random damage
        h, t = rng.randrange(0, 70), rng.randrange(0, 70)

        def damage(s):
            for _ in range(rng.randrange(0, 5)):
                p = rng.randrange(0, len(s) + 1)
                kind = rng.randrange(3)
                s = s[:p] + bytes([rng.choice(b"ACGT")]) + s[p + (kind != 1):] if kind < 2 else s[:p] + s[p + 1:]
            return s
        B.add(rng.randrange(80, 3800), h, t, rng.randrange(2), head=damage, tail=damage, gap=rng.randrange(0, 3))
    c = B.add(2000, 4, 2, 0)                                       # last read: the tail reads the last two bytes of qtext upwards
    # a chain of two seeds: its head belongs to the first, its tail to the second
    B.first[c - 1] = B.first[c - 2]; B.q_lo[c - 1] = B.q_lo[c - 2]
    return B


def model(arrs, ref_base, max_edits, cost):
    return EM.chain_ends_model(*arrs, K, ref_base, max_edits, cost)


def same(got, exp, what):
    for name, g, e in zip(NAMES, got, exp):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        assert np.array_equal(g.view(e.dtype), e), "%s: %s differs at %s" % (what, name, np.flatnonzero(g.view(e.dtype) != e)[:8] if len(g) == len(e) else "length")


@pytest.fixture(scope="module")
def batch():
    B = build()
    arrs = B.arrays()
    return B, arrs, {(me, cc): model(arrs, 0, me, cc) for me, cc in ((31, 4), (31, 1), (31, 255), (0, 4))}


def test_the_batch_covers_what_it_claims(batch):
    B, arrs, exp = batch
    q, r, e, clip, offs, ops = exp[(31, 1)]
    assert 60 <= len(B.first) and 4000 == len(arrs[1]) and max(len(r) for r in B.reads) <= 200
    assert e.max() == 31 and (clip > 0).any() and (clip == 0).any()
    rows = np.arange(len(q))
    for head in (0, 1):
        for rev in (0, 1):                                          # each of the four readers aligns something with an edit in it
            sel = (rows % 2 == 1 - head) & (np.array(B.rev)[np.array(B.first)[rows // 2]] == rev) & (e > 0)
            assert sel.any(), (head, rev)
    q4 = exp[(31, 4)]
    assert not np.array_equal(q4[0], q) and not np.array_equal(exp[(31, 255)][0], q4[0]) and exp[(0, 4)][2].max() == 0
    assert {1, 2, 7, 8} <= set(int(v) & 15 for v in ops)


@pytest.mark.parametrize("max_edits,cost", [(31, 4), (31, 1), (31, 255), (0, 4)])
def test_numpy_equals_the_model(batch, max_edits, cost):
    _, arrs, exp = batch
    got = kh.chain_ends(*arrs, K, 0, max_edits, cost)
    assert [x.dtype for x in got] == [np.uint32] * 4 + [np.uint64, np.uint32]
    same(got, exp[(max_edits, cost)], "numpy")


@pytest.mark.parametrize("max_edits,cost", [(31, 4), (31, 1), (0, 4)])
def test_tensors_equal_the_model(batch, max_edits, cost):
    _, arrs, exp = batch
    got = kh.chain_ends(*(to_dev(a) for a in arrs), K, 0, max_edits, cost)
    assert all(x.is_cuda for x in got) and [x.dtype for x in got] == [torch.int32] * 4 + [torch.int64, torch.int32]
    same(got, exp[(max_edits, cost)], "tensors")


def test_ref_base():
    B = build(ref_base=123457)
    arrs = B.arrays()
    exp = model(arrs, 123457, 31, 4)
    assert exp[0].any()
    same(kh.chain_ends(*arrs, K, 123457, 31, 4), exp, "ref_base, numpy")
    same(kh.chain_ends(*(to_dev(a) for a in arrs), K, 123457), exp, "ref_base, tensors")
    # the same anchors against a text that starts elsewhere: every seed that falls outside gives empty rows
    shifted = model(arrs, 123457 + 2000, 31, 4)
    assert (shifted[0] == 0).any() and shifted[0].any()
    same(kh.chain_ends(*arrs, K, 123457 + 2000), shifted, "ref_base shifted")


GUARD = 0x5A5A5A5A


def raw(arrs, m, nc, k=K, max_edits=31, cost=4, ref_base=0, cap=None, count_only=False):
    """the C call over device memory with guard words around every output -> (status, n_ops, outputs on the host)"""
    ins_ = [to_dev(a) for a in arrs]
    pad = 16
    outs = [torch.full((2 * nc + 2 * pad,), GUARD, dtype=torch.int32, device="cuda") for _ in range(4)]
    offs = torch.full((2 * nc + 1 + 2 * pad,), GUARD, dtype=torch.int64, device="cuda")
    n = C.c_uint64(77)
    f = _capi.lib().kh_chain_ends
    stream = torch.cuda.current_stream().cuda_stream

    def call(ops_ptr, cap_ops):
        return f(ins_[0].data_ptr(), arrs[0].size, ins_[1].data_ptr(), arrs[1].size, ref_base, *(t.data_ptr() for t in ins_[2:5]), m,
                 *(t.data_ptr() for t in ins_[5:9]), nc, k, max_edits, cost, _capi.KH_MEM_DEVICE, *(o[pad:].data_ptr() for o in outs), offs[pad:].data_ptr(),
                 ops_ptr, cap_ops, C.byref(n), 0, stream)

    st = call(None, 0)
    total = n.value
    ops = torch.full(((total if cap is None else cap) + 2 * pad,), GUARD, dtype=torch.int32, device="cuda")
    if st == _capi.KH_OK and not count_only:
        st = call(ops[pad:].data_ptr(), total if cap is None else cap)
    torch.cuda.synchronize()
    host = [o.cpu().numpy() for o in outs] + [offs.cpu().numpy(), ops.cpu().numpy()]
    for name, a in zip(NAMES, host):
        g = np.int64(GUARD) if a.dtype == np.int64 else np.int32(GUARD)
        assert (a[:pad] == g).all() and (a[len(a) - pad:] == g).all(), "guard words around %s" % name
    return st, n.value, [a[pad:len(a) - pad] for a in host]


def test_garbage_gives_empty_rows_and_touches_nothing_else(batch):
    B, arrs, _ = batch
    qt, rt, qpos, rpos, rev, first, last, lo, hi = (a.copy() for a in arrs)
    m, nc, nq = len(qpos), len(first), len(qt)
    first[0] = m; last[1] = 0xFFFFFFFF; first[2] = 0x80000000           # anchor indices outside [0, m)
    lo[3] = qpos[first[3]] + 1                                           # q_lo > q_f: the head; the tail stands
    hi[4] = qpos[last[4]] + K - 1                                        # q_l + k > q_hi: both (the seed leaves the read)
    hi[5] = nq + 1; hi[6] = 0xFFFFFFFF                                   # q_hi > nq
    lo[7] = 0xFFFFFFFF
    qpos[first[8]] = 0x80000000; rpos[first[9]] = 0xFFFFFFFF             # positions >= 2^31
    rpos[first[10]] = 4000 - K + 1; rpos[first[11]] = 4000 + 50          # the seed outside rtext
    g = (qt, rt, qpos, rpos, rev, first, last, lo, hi)
    exp = model(g, 0, 31, 4)
    for c in (4, 5, 6, 7, 8, 9, 10, 11):
        assert not exp[0][2 * c:2 * c + 2].any() and exp[4][2 * c] == exp[4][2 * c + 2], c
    assert exp[0][2] and not exp[0][3] and exp[4][3] == exp[4][4]        # chain 1: its head stands, no tail
    for c in (0, 2, 3):                                                  # no head; the tail stands where it has a base
        assert not exp[0][2 * c] and not exp[3][2 * c] and exp[4][2 * c] == exp[4][2 * c + 1] and (c == 3 or exp[0][2 * c + 1] or exp[3][2 * c + 1]), c
    st, n, got = raw(g, m, nc)
    assert st == _capi.KH_OK and n == len(exp[5])
    same(got, exp, "garbage, device")
    same(kh.chain_ends(*g, K), exp, "garbage, numpy")
    # ref_base beyond every position: the seeds lie below rtext
    st, n, got = raw(arrs, m, nc, ref_base=1 << 20)
    assert st == _capi.KH_OK and n == 0 and not any(a.any() for a in got[:5])
    # no anchors at all: every first / last is outside
    st, n, got = raw(arrs, 0, nc)
    assert st == _capi.KH_OK and n == 0 and not any(a.any() for a in got[:5])


def test_count_only_then_emit_and_a_cap_that_is_too_small(batch):
    _, arrs, exps = batch
    exp = exps[(31, 4)]
    m, nc, total = len(arrs[2]), len(arrs[5]), len(exps[(31, 4)][5])
    st, n, got = raw(arrs, m, nc, count_only=True)
    assert st == _capi.KH_OK and n == total
    same(got[:5], exp[:5], "count only")
    assert (got[5].view(np.uint32) == GUARD).all()                       # no row was written
    st, n, got = raw(arrs, m, nc)
    assert st == _capi.KH_OK and n == total
    same(got, exp, "count, then emit")
    st, n, got = raw(arrs, m, nc, cap=total - 1)
    assert st == _capi.KH_ERR_INVALID and n == total                     # refused with *n_ops set, the numbers and offsets written
    same(got[:5], exp[:5], "cap too small")
    assert (got[5].view(np.uint32) == GUARD).all()


def test_no_chains_and_refused_arguments(batch):
    _, arrs, _ = batch
    m = len(arrs[2])
    e = np.zeros(0, dtype=np.uint32)
    for mk in (lambda a: a, to_dev):
        got = kh.chain_ends(*(mk(a) for a in arrs[:5]), mk(e), mk(e), mk(e), mk(e), K)
        assert all(len(x) == 0 for x in got[:4]) and len(got[5]) == 0 and [int(v) for v in got[4]] == [0]
    empty = tuple(arrs[:5]) + (e, e, e, e)
    st, n, got = raw(empty, m, 0)
    assert st == _capi.KH_OK and n == 0 and got[4].tolist() == [0]
    # arguments the call refuses leave the outputs as they were
    nc = len(arrs[5])
    for kw in (dict(k=0), dict(k=65), dict(max_edits=32), dict(cost=0), dict(cost=256), dict(ref_base=(1 << 31) - 100)):
        st, n, got = raw(arrs, m, nc, **kw)
        assert st == _capi.KH_ERR_INVALID and n == 77, kw
        assert all((a.view(np.uint32 if a.dtype == np.int32 else np.uint64) == GUARD).all() for a in got), kw
    st, n, got = raw(arrs, (1 << 24) + 1, nc)
    assert st == _capi.KH_ERR_INVALID and n == 77
    with pytest.raises(ValueError):
        kh.chain_ends(*(to_dev(a) for a in arrs[:8]), arrs[8], K)        # mixed memory
