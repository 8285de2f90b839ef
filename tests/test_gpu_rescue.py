"""GPU: kh_mate_rescue against the model of tests/rescue_model.py, bit for bit: edits, rs, re, span, offsets and ops of every request, for
host arrays and for CUDA tensors.  The shapes are the smallest at which the kernels can go wrong: mates of 1, 2, 63, 64, 65, 127, 128,
129, 511 and 512 bases (every word count on either side of a word boundary; 513: not looked at), windows of 0, m - 1, m, m + 1 and
m + 31 bases and one the text's end clips, the end column first and last, d* of 0, 1, 31 and 32, N on either side, both strands, the
homopolymer tie, gaps at the first and last base, 65 and 130 requests of mixed word counts with garbage between them, ref_base != 0,
text views at odd byte offsets, count-only then emit and a cap that is too small."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi  # noqa: E402
import rescue_model as RM  # noqa: E402
from stream_checks import to_dev  # noqa: E402

NAMES = ("edits", "rs", "re", "span", "offsets", "ops")
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
GUARD = 0x5A5A5A5A


def revcomp(s):
    return bytes(reversed(s.translate(COMP)))


def rand(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def sub(s, *at):
    b = bytearray(s)
    for p in at:
        b[p] = {65: 67, 67: 71, 71: 84, 84: 65}.get(b[p] & 0xDF, 65)
    return bytes(b)


class Batch:
    """requests over one query text and one reference text: every request brings its own stretch of both"""

    def __init__(self, seed, ref_base=0):
        self.rng, self.ref_base = random.Random(seed), ref_base
        self.q, self.r, self.req = bytearray(b"GA"), bytearray(b"TTC"), []

    def add(self, R, window, rev=0, w_cut=(0, 0)):
        """R: the pattern in reference order; the mate goes into the query text as the sequencer would give it.  w_cut: bases of
        `window` left out of the request's window in front and behind (they stay in the text)"""
        mate = revcomp(R) if rev else R
        q_lo, w_lo = len(self.q), len(self.r)
        self.q += mate + rand(self.rng, self.rng.randrange(0, 3))
        self.r += window + rand(self.rng, self.rng.randrange(0, 3))
        self.req.append((q_lo, q_lo + len(mate), self.ref_base + w_lo + w_cut[0], self.ref_base + w_lo + len(window) - w_cut[1], rev))
        return len(self.req) - 1

    def raw(self, q_lo, q_hi, w_lo, w_hi, rev):
        self.req.append((q_lo, q_hi, w_lo, w_hi, rev))
        return len(self.req) - 1

    def arrays(self):
        cols = list(zip(*self.req)) if self.req else [[]] * 5
        return (np.frombuffer(bytes(self.q), dtype=np.uint8).copy(), np.frombuffer(bytes(self.r), dtype=np.uint8).copy(),
                *(np.array(c, dtype=np.uint32) for c in cols[:4]), np.array(cols[4], dtype=np.uint8))


def same(got, exp, what):
    for name, g, e in zip(NAMES, got, exp):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        assert g.shape == e.shape and np.array_equal(g.view(e.dtype), e), "%s: %s\n got %s\n exp %s" % (what, name, g.view(e.dtype)[:40], e[:40])


def check(B, max_edits=31):
    """both memories against the model -> the model's answer"""
    a = B.arrays()
    exp = RM.rescue_model(*a, B.ref_base, max_edits)
    for mk, what in ((lambda x: x, "numpy"), (to_dev, "device")):
        r = kh.rescue_mates(*(mk(x) for x in a), B.ref_base, max_edits)
        same((r.edits, r.rs, r.re, r.span, r.offsets, r.ops), exp, what)
        host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x      # noqa: E731
        assert np.array_equal(host(r.read).view(np.uint32), np.arange(len(a[2]), dtype=np.uint32)) and np.array_equal(host(r.rev), a[6])
    return exp


def planted(rng, m, W, at, edits=()):
    """a window of W random bases and the m bases at `at` of it with substitutions at `edits`"""
    win = rand(rng, W)
    return sub(win[at:at + m], *edits), win


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 127, 128, 129, 511, 512])
def test_every_word_count_and_window_length(m):
    B = Batch(100 + m)
    rng = B.rng
    for t, W in enumerate((0, m - 1, m, m + 1, m + 31)):
        if W >= m:
            R, win = planted(rng, m, W, rng.randrange(0, W - m + 1), [p for p in (m // 3, m - 1) if t % 2 and m > 2])
        else:
            R, win = rand(rng, m), rand(rng, W)
        B.add(R, win, rev=t & 1)
    R, win = planted(rng, m, m + 9, 9)                     # the fragment ends with the text: the window is clipped by the text's end
    B.add(R, win, rev=1)
    del B.r[B.req[-1][3]:]
    exp = check(B)
    assert exp[0][5] == 0 and (m < 16 or exp[2][5] == len(B.r))          # found; a mate long enough to be unique ends at the text's last base
    assert exp[0][0] == (m if m <= 31 else RM.OVER)                      # an empty window: m insertions
    assert (exp[0][2:5] >= 0).all() and (exp[0][2:5] <= 2).all()


def test_513_bases_are_not_looked_at():
    B = Batch(7)
    w = rand(B.rng, 600)
    B.add(w[10:523], w)
    B.add(w[10:522], w)
    exp = check(B)
    assert exp[0].tolist() == [RM.NONE, 0] and exp[4].tolist() == [0, 0, 1]


def test_end_column_first_and_last_both_strands():
    B = Batch(8)
    for rev in (0, 1):
        for m, W in ((40, 90), (100, 131), (200, 260)):
            w = rand(B.rng, W)
            B.add(w[:m], w, rev)                 # e = m: the first column a whole mate can end at
            B.add(w[W - m:], w, rev)             # e = W: the last column
    exp = check(B)
    a = B.arrays()
    assert (exp[0] == 0).all() and (exp[3] == 0).all()
    assert (exp[2][0::2] - a[4][0::2] == a[3][0::2] - a[2][0::2]).all() and (exp[2][1::2] == a[5][1::2]).all()


def test_distances_0_1_31_32_and_max_edits_0():
    B = Batch(9)
    m = 264
    w = rand(B.rng, m + 8)
    at31 = list(range(5, 5 + 8 * 31, 8))
    B.add(w[4:4 + m], w)
    B.add(sub(w[4:4 + m], 200), w, rev=1)
    B.add(sub(w[4:4 + m], *at31), w)
    B.add(sub(w[4:4 + m], *(at31 + [258])), w, rev=1)
    exp = check(B)
    assert exp[0].tolist() == [0, 1, 31, RM.OVER]
    assert (exp[4][1:] - exp[4][:-1]).tolist() == [1, 3, 63, 0]          # 2 d* + 1 runs
    exp = check(B, max_edits=0)
    assert exp[0].tolist() == [0, RM.OVER, RM.OVER, RM.OVER]
    exp = check(B, max_edits=1)
    assert exp[0].tolist() == [0, 1, RM.OVER, RM.OVER]


def test_n_in_the_mate_in_the_reference_and_facing():
    B = Batch(10)
    for rev in (0, 1):
        for m in (30, 70):
            w = rand(B.rng, m + 20)
            f = w[10:10 + m]
            B.add(f[:12] + b"N" + f[13:], w, rev)                                    # N in the mate
            B.add(f, w[:22] + b"N" + w[23:], rev)                                    # N in the reference
            B.add(f[:12] + b"N" + f[13:], w[:22] + b"n" + w[23:], rev)               # N facing N: no match
            B.add(f.lower(), w, rev)                                                 # lower case is a base
    exp = check(B)
    assert exp[0].reshape(-1, 4).tolist() == [[1, 1, 1, 0]] * 4


def test_homopolymer_tie_rule():
    B = Batch(11, ref_base=50)
    j = [B.add(b"A" * m, b"A" * W, rev) for rev in (0, 1) for m, W in ((20, 50), (64, 64), (65, 200), (130, 131))]
    exp = check(B)
    a = B.arrays()
    for t in j:
        m, W = int(a[3][t] - a[2][t]), int(a[5][t] - a[4][t])
        # e = m: the first column that attains 0; every later one attains it too; the start is on diagonal 0 (the smaller |d|)
        assert (exp[0][t], exp[2][t] - a[4][t], exp[3][t], exp[2][t] - exp[1][t]) == (0, m, W - m, m), t


def test_gaps_at_the_first_and_last_base():
    B = Batch(12)
    for rev in (0, 1):
        for m in (40, 100):
            w = rand(B.rng, m + 30)
            f = w[15:15 + m]
            other = lambda c: b"A" if c != ord("A") else b"C"      # noqa: E731
            B.add(other(w[14]) + f, w, rev)                        # a base in front of the fragment that the reference does not have
            B.add(f + other(w[15 + m]), w, rev)                    # ... behind it
            B.add(f[:1] + f[2:], w, rev)                           # the mate lacks the fragment's second base
            B.add(f[:-2] + f[-1:], w, rev)                         # ... its last but one
            B.add(f[:1] + b"G" + f[1:], w, rev)                    # an insertion behind the first base
            B.add(f[:-1] + b"G" + f[-1:], w, rev)                  # ... before the last
    exp = check(B)
    assert ((exp[0] >= 0) & (exp[0] <= 1)).all() and (exp[0] == 1).sum() >= 16


def mixed(B, n):
    rng = B.rng
    for t in range(n):
        if t % 9 == 4:                                             # garbage between good requests: -1, nothing outside the texts is read
            B.raw(*[(5, 5, 0, 40, 0), (9, 4, 0, 40, 1), (0, 1 << 30, 0, 40, 0), (0, 30, 1 << 31, (1 << 31) + 9, 0), (0, 30, 40, 10, 1),
                    (0, 30, 0xFFFFFFF0, 0xFFFFFFFF, 0), (0xFFFFFFFF, 3, 0, 5, 0)][t % 7])
            continue
        m = [1, 30, 64, 65, 100, 128, 129, 150, 193, 257][(t * 7) % 10]      # 1, 2, 3, 4 and 5 words side by side in one wave
        W = m + rng.randrange(0, 24)
        at = rng.randrange(0, W - m + 1)
        R, win = planted(rng, m, W, at, rng.sample(range(m), min(m, t % 4)))
        if t % 5 == 0 and m > 20:
            R = R[:m // 2] + R[m // 2 + 1:]                        # a deletion as well
        B.add(R, win, rev=t & 1, w_cut=(t % 3, 0))


@pytest.mark.parametrize("n,ref_base", [(65, 0), (130, 1000)])
def test_mixed_word_counts_garbage_and_ref_base(n, ref_base):
    B = Batch(n, ref_base)
    mixed(B, n)
    exp = check(B)
    assert (exp[0] == RM.NONE).sum() == len([t for t in range(n) if t % 9 == 4]) and (exp[0] >= 0).sum() > n // 2


def test_text_views_at_byte_offsets_equal_an_aligned_clone():
    B = Batch(13)
    mixed(B, 40)
    a = B.arrays()
    exp = RM.rescue_model(*a, 0, 31)
    dev = [to_dev(x) for x in a]
    for off in (1, 3, 7):
        views = []
        for t in dev[:2]:
            buf = torch.empty(t.numel() + 16, dtype=torch.uint8, device="cuda")
            base = (-buf.data_ptr()) % 8 + off
            v = buf[base:base + t.numel()]
            v.copy_(t)
            assert v.data_ptr() % 8 == off
            views.append(v)
        r = kh.rescue_mates(views[0], views[1], *dev[2:])
        same((r.edits, r.rs, r.re, r.span, r.offsets, r.ops), exp, "offset %d" % off)


def raw(a, cap=None, count_only=False, max_edits=31):
    """the C call over device memory with guarded outputs -> (status, n_ops, outputs)"""
    n = len(a[2])
    dev = [to_dev(x) for x in a]
    total = cap if cap is not None else 4096
    outs = [torch.full((n,), GUARD, dtype=torch.int32, device="cuda") for _ in range(4)]
    offs = torch.full((n + 1,), GUARD, dtype=torch.int64, device="cuda")
    ops = torch.full((max(total, 1),), GUARD, dtype=torch.int32, device="cuda")
    n_ops = C.c_uint64(12345)
    st = _capi.lib().kh_mate_rescue(dev[0].data_ptr(), len(a[0]), dev[1].data_ptr(), len(a[1]), 0, *(x.data_ptr() for x in dev[2:]), n, max_edits, _capi.KH_MEM_DEVICE,
                                    *(x.data_ptr() for x in outs), offs.data_ptr(), None if count_only else ops.data_ptr(), 0 if count_only else total, C.byref(n_ops),
                                    0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, n_ops.value, [x.cpu().numpy() for x in outs + [offs, ops]]


def test_count_only_then_emit_and_a_cap_that_is_too_small():
    B = Batch(14)
    mixed(B, 30)
    a = B.arrays()
    exp = RM.rescue_model(*a, 0, 31)
    total = len(exp[5])
    assert total > 30
    st, n, got = raw(a, count_only=True)
    assert st == _capi.KH_OK and n == total
    same(got[:5], exp[:5], "count only")
    assert (got[5].view(np.uint32) == GUARD).all()                       # no row was written
    st, n, got = raw(a, cap=total)
    assert st == _capi.KH_OK and n == total
    same(got, exp, "count, then emit")
    st, n, got = raw(a, cap=total - 1)
    assert st == _capi.KH_ERR_INVALID and n == total                     # refused with *n_ops set, the numbers and offsets written
    same(got[:5], exp[:5], "cap too small")
    assert (got[5].view(np.uint32) == GUARD).all()


def test_no_requests():
    e, t = np.zeros(0, dtype=np.uint32), np.frombuffer(b"ACGT", dtype=np.uint8).copy()
    for mk in (lambda x: x, to_dev):
        r = kh.rescue_mates(mk(t), mk(t), mk(e), mk(e), mk(e), mk(e), mk(np.zeros(0, dtype=np.uint8)))
        assert [int(v) for v in r.offsets] == [0] and all(len(x) == 0 for x in (r.edits, r.rs, r.re, r.span, r.ops))
