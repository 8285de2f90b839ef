"""GPU: kh_chain_cigars against the model of tests/cigar_model.py, bit for bit: offsets, ops, ins and dels, for host arrays and for CUDA
tensors.  pred and chain are built by hand (tests/edits_cases.py), the link array is the one a real kh_chain_edits call wrote over the
same inputs unless a test says otherwise.  The shapes are the smallest at which the kernels can go wrong: link lengths around the 8-base
words of the compare, an edit at either end of a link, the edge diagonals (|dq - dr| = 31) and the last level (31 edits) of the wavefront
pass, both strands, N and lower case, the ends of both texts, every way a row can be empty, link values that are not the distance, and
anchor counts of less than a wave, two waves and two workgroups."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import cigar_model as CM  # noqa: E402
from edits_cases import K, Batch, bases, other, revcomp, sub  # noqa: E402
from stream_checks import to_dev  # noqa: E402


def run_host(arrs, n_chains, k, link, ref_base=0):
    got = kh.chain_cigars(*arrs, n_chains, k, link, ref_base=ref_base)
    assert [x.dtype for x in got] == [np.uint64, np.uint32, np.uint32, np.uint32]
    return tuple(got)


def run_dev(arrs, n_chains, k, link, ref_base=0):
    got = kh.chain_cigars(*(to_dev(a) for a in arrs), n_chains, k, to_dev(link), ref_base=ref_base)
    assert all(t.is_cuda for t in got) and got.offsets.dtype == torch.int64 and all(t.dtype == torch.int32 for t in got[1:])
    torch.cuda.synchronize()
    return (got.offsets.cpu().numpy().view(np.uint64),) + tuple(t.cpu().numpy().view(np.uint32) for t in got[1:])


def real_link(arrs, n_chains, k, ref_base=0):
    return kh.chain_edits(*arrs, n_chains, k, ref_base=ref_base, max_edits=31)


def rows(offsets, ops):
    return [CM.text([(int(v) & 15, int(v) >> 4) for v in ops[int(offsets[i]):int(offsets[i + 1])]]) for i in range(len(offsets) - 1)]


def check(arrs, n_chains, k, link, ref_base, what):
    exp = CM.chain_cigars_model(*arrs, n_chains, k, link, ref_base)
    outs = []
    for name, run in (("host", run_host), ("device", run_dev)):
        got = run(arrs, n_chains, k, link, ref_base)
        assert np.array_equal(got[0], exp[0]), (what, name, [(i, a, b) for i, (a, b) in enumerate(zip(rows(got[0], got[1]), rows(exp[0], exp[1]))) if a != b][:6])
        assert np.array_equal(got[1], exp[1]), (what, name, [(i, a, b) for i, (a, b) in enumerate(zip(rows(got[0], got[1]), rows(exp[0], exp[1]))) if a != b][:6])
        assert np.array_equal(got[2], exp[2]) and np.array_equal(got[3], exp[3]), (what, name)
        outs.append(got)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(*outs)), (what, "host input and device input differ")
    return exp


# ---- link lengths around the 8-byte steps x what a link can hold, both strands
LENGTHS = [1, 7, 8, 9, 63, 64, 65, 300]


def build_shapes(ref_base):
    B = Batch(31, ref_base=ref_base)
    rng, want = B.rng, {}
    for rev in (0, 1):
        for L in LENGTHS:
            a, h = bases(rng, L), L // 2
            x = bytes([other(rng, a[h])])
            want[B.add([(a, a)], rev)] = "%d=" % L
            want[B.add([(a, sub(rng, a, [h]))], rev)] = None                      # one substitution
            want[B.add([(a, a[:h] + x + a[h:])], rev)] = None                     # one base more in the reference: D
            B.add([(a + x, a)], rev)                                              # one base more in the query, at the end: I
            want[B.add([(a, bytes([other(rng, a[0])]) + a)], rev)] = "1D%d=" % L  # an indel at either end
            want[B.add([(a, a + bytes([other(rng, a[-1])]))], rev)] = "%d=1D" % L
            want[B.add([(bytes([other(rng, a[0])]) + a, a)], rev)] = "1I%d=" % L
            want[B.add([(a + bytes([other(rng, a[-1])]), a)], rev)] = "%d=1I" % L
            want[B.add([(sub(rng, a, [0]), a)], rev)] = ("1X%d=" % (L - 1)) if L > 1 else "1X"
            want[B.add([(a, sub(rng, a, [L - 1]))], rev)] = ("%d=1X" % (L - 1)) if L > 1 else "1X"
        a, ins = bases(rng, 50), bases(rng, 31)
        B.add([(a, a[:25] + ins + a[25:])], rev)                 # dr - dq = +31: the top lane
        B.add([(a[:25] + ins + a[25:], a)], rev)                 # dr - dq = -31: lane 1
        B.add([(a, ins + a)], rev); B.add([(a + ins, a)], rev)
        a = bases(rng, 300)
        B.add([(a, sub(rng, a, [9 * t + 1 for t in range(31)]))], rev)                       # exactly 31 edits
        b = sub(rng, a, [17 + 19 * t for t in range(11)])
        for t in range(10):                                                                  # 11 substitutions, 10 insertions, 10 deletions
            b = b[:5 + 28 * t] + bytes([other(rng, b[5 + 28 * t])]) + b[5 + 28 * t:15 + 28 * t] + b[16 + 28 * t:]
        B.add([(a, b)], rev)
        a = bases(rng, 30)
        B.add([(a.lower(), a)], rev); B.add([(a, sub(rng, a, [4]).lower())], rev)
        B.add([(a[:10] + b"N" + a[11:], a)], rev); B.add([(a, a[:10] + b"N" + a[11:])], rev)
        B.add([(a[:10] + b"N" + a[11:], a[:10] + b"N" + a[11:])], rev)                       # N against N: 1X
        B.add([(b"N" * 9, b"N" * 9)], rev); B.add([(a, a[:12] + b"n" + a[12:])], rev)
        B.add([(b"AC", b"CA")], rev); B.add([(b"AAA", b"AA")], rev); B.add([(b"ACGTAC", b"ACTAC")], rev)
        pairs = []                                                                           # a chain of 40 links, every third with an edit
        for t in range(40):
            a = bases(rng, rng.randrange(3, 30))
            pairs.append((a, [a, sub(rng, a, [len(a) // 2]), a[:1] + a[2:]][t % 3]))
        B.add(pairs, rev)
    return B, want


@pytest.fixture(scope="module")
def shapes():
    out = {}
    for ref_base in (0, 100003):
        B, want = build_shapes(ref_base)
        arrs = B.arrays()
        out[ref_base] = (B, want, arrs)
    return out


@pytest.mark.parametrize("ref_base", [0, 100003])
def test_shapes_with_the_link_of_chain_edits(shapes, ref_base):
    B, want, arrs = shapes[ref_base]
    ed = real_link(arrs, B.n_chains, K, ref_base)
    assert (ed.link == 31).sum() >= 6 and (ed.over == 0).all()
    exp = check(arrs, B.n_chains, K, ed.link, ref_base, "shapes")
    text = rows(exp[0], exp[1])
    for i, s in want.items():
        assert s is None or text[i] == s, (i, s, text[i])
    assert "2X" in text and "2=1I" in text and "2=1I3=" in text      # the hand cases of the definition
    # per chain: X + I + D of its rows is the distance kh_chain_edits summed, I and D the chain arrays
    per = {op: np.zeros(B.n_chains, dtype=np.int64) for op in (CM.OP_X, CM.OP_I, CM.OP_D, CM.OP_EQ)}
    for a in range(len(arrs[2])):
        for v in exp[1][int(exp[0][a]):int(exp[0][a + 1])]:
            per[int(v) & 15][arrs[6][a]] += int(v) >> 4
    assert np.array_equal(per[CM.OP_X] + per[CM.OP_I] + per[CM.OP_D], ed.edits) and np.array_equal(per[CM.OP_I], exp[2]) and np.array_equal(per[CM.OP_D], exp[3])
    # every non-empty row walks its two strings from end to end
    qc, rc = CM._codes(arrs[0]), CM._codes(arrs[1])
    assert sum(1 for s in text if s) == (ed.link >= 0).sum()
    for a in np.flatnonzero(ed.link >= 0)[::7]:
        p = int(arrs[5][a])
        A = [int(c) for c in qc[int(arrs[2][p]):int(arrs[2][a])]]
        ri, rj = int(arrs[3][a]), int(arrs[3][p])
        lo, hi = (ri + K - ref_base, rj + K - ref_base) if arrs[4][a] else (rj - ref_base, ri - ref_base)
        Bc = CM._oriented(rc[lo:hi], int(arrs[4][a]))
        w = CM.apply_ops(A, Bc, CM.parse(text[a]))
        assert w is not None and w[:2] == (len(A), len(Bc)) and sum(w[2:]) == ed.link[a], (a, text[a])


# ---- anchor counts: none, one, two waves, two workgroups
@pytest.mark.parametrize("m", [0, 1, 65, 257])
def test_anchor_counts(m):
    B = Batch(37)
    rng = B.rng
    while len(B.qpos) < m:
        pairs = []
        for t in range(min(rng.randrange(1, 9), max(1, m - len(B.qpos) - 1))):
            a = bases(rng, rng.randrange(2, 40))
            pairs.append((a, [a, sub(rng, a, [1]), a[1:], a + b"G"][rng.randrange(4)]))
        B.add(pairs, rev=len(B.qpos) & 1)
    arrs = tuple(x[:m] if x.dtype != np.uint8 or i > 1 else x for i, x in enumerate(B.arrays()))
    nc = B.n_chains if m else 3
    ed = real_link(arrs, nc, K)
    exp = check(arrs, nc, K, ed.link, 0, "m = %d" % m)
    assert len(exp[0]) == m + 1 and (m < 2 or len(exp[1]) > m // 2)
    if m == 0:
        got = run_dev(arrs, nc, K, ed.link)
        assert got[0].tolist() == [0] and len(got[1]) == 0 and got[2].tolist() == [0, 0, 0] and got[3].tolist() == [0, 0, 0]


# ---- the ends of the texts, with a guard behind every device buffer
def edge_case(kind):
    """one link whose strings touch the ends of the texts.  "end": A ends where its seed is the last k bytes of qtext and B is the end
    (forward: the whole) of rtext; "start": a reverse link whose stretch starts at byte 0 of rtext"""
    B = Batch(41, k=K, ref_base=50)
    a = bases(B.rng, 20)
    b = a[:7] + a[8:]                                            # one base of A missing in B: 7=1I12= (or next to it, inside a run)
    B.q += a + bases(B.rng, K)
    if kind == "end_fwd":
        B.r += b
        B.qpos, B.rpos, B.rev = [0, 20], [50, 69], [0, 0]
    elif kind == "end_rev":
        B.r += bases(B.rng, K) + revcomp(b)
        B.qpos, B.rpos, B.rev = [0, 20], [69, 50], [1, 1]
    else:
        B.r += revcomp(b) + bases(B.rng, 3)
        B.qpos, B.rpos, B.rev = [0, 20], [50 - K + 19, 50 - K], [1, 1]
    B.pred, B.chain, B.n_chains = [-1, 0], [0, 0], 1
    return B.arrays()


@pytest.mark.parametrize("kind", ["end_fwd", "end_rev", "start_rev"])
def test_text_ends_and_guards(kind):
    from kmerhash_amd import _capi
    import ctypes as C
    arrs = edge_case(kind)
    ed = real_link(arrs, 1, K, 50)
    assert ed.link.tolist() == [-1, 1]
    exp = check(arrs, 1, K, ed.link, 50, kind)
    assert exp[0].tolist() == [0, 0, 3] and exp[2].tolist() == [1] and exp[3].tolist() == [0]
    # one byte less of either text: the link leaves the texts, the row is empty whatever link says
    for cut in ((1, 0), (0, 1)) if kind != "start_rev" else ((1, 0),):
        short = (arrs[0][:len(arrs[0]) - cut[0]], arrs[1][:len(arrs[1]) - cut[1]]) + arrs[2:]
        e2 = check(short, 1, K, ed.link, 50, kind + " cut")
        assert e2[0].tolist() == [0, 0, 0] and len(e2[1]) == 0
    if kind == "start_rev":                                      # the stretch would start one byte before rtext
        e2 = check(arrs, 1, K, ed.link, 51, kind + " low")
        assert e2[0].tolist() == [0, 0, 0]
    # device buffers with 64 guard elements behind each: the answer holds with them in place and no guard is written
    G = 64
    ins = []
    for a in arrs + (ed.link,):
        t = torch.full((a.size + G,), 65 if a.dtype == np.uint8 and a.size > 2 else 0, dtype=to_dev(a[:1]).dtype, device="cuda")
        t[:a.size] = to_dev(a)
        ins.append(t)
    offs = torch.full((3 + G,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    outs = [torch.full((n + G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for n in (3, 1, 1)]
    n = C.c_uint64()
    st = _capi.lib().kh_chain_cigars(ins[0].data_ptr(), arrs[0].size, ins[1].data_ptr(), arrs[1].size, 50, *(t.data_ptr() for t in ins[2:7]), 2, 1, K, ins[7].data_ptr(),
                                     _capi.KH_MEM_DEVICE, offs.data_ptr(), outs[0].data_ptr(), 3, C.byref(n), outs[1].data_ptr(), outs[2].data_ptr(), 0,
                                     torch.cuda.current_stream().cuda_stream)
    assert st == _capi.KH_OK and n.value == 3
    torch.cuda.synchronize()
    assert offs[:3].tolist() == [0, 0, 3] and outs[0][:3].cpu().numpy().view(np.uint32).tolist() == exp[1].tolist()
    assert outs[1][0].item() == 1 and outs[2][0].item() == 0
    assert (offs[3:] == 0x5A5A5A5A).all() and all((t[c:] == 0x5A5A5A5A).all() for t, c in zip(outs, (3, 1, 1)))
    for t, a in zip(ins, arrs + (ed.link,)):
        assert (t[a.size:] == (65 if a.dtype == np.uint8 and a.size > 2 else 0)).all()


# ---- rows that are empty, and input that contradicts itself
def test_empty_rows_and_inconsistent_input():
    B = Batch(43)
    rng = B.rng
    a = bases(rng, 25)
    for rev in (0, 1):
        for _ in range(10):
            B.add([(a, sub(rng, a, [5])), (a, a), (a, a[:9] + a[10:]), (a, a[:3] + b"T" + a[3:])], rev)
    ins32 = bases(rng, 32)
    B.add([(a, a[:5] + ins32 + a[5:])], 0)                         # |dq - dr| = 32: over in kh_chain_edits, an empty row here
    arrs = B.arrays()
    qt, rt, q, r, v, pred, chain = arrs
    m, nc = len(q), B.n_chains
    ed = real_link(arrs, nc, K)
    assert ed.link[m - 1] == -2
    check(arrs, nc, K, ed.link, 0, "consistent")
    # chain c is the anchors 5c .. 5c + 4; link values that are not the distance
    link = ed.link.copy()
    link[1] = 0                        # 0 where there is an edit (dq == dr): the run "25=", by definition without a look at the texts
    link[3] = 0                        # 0 with dq != dr: empty
    link[6] = 5; link[8] = 31          # too large: the alignment found at the smaller e
    link[11] = -1; link[12] = -2; link[13] = 40; link[14] = -2 ** 31; link[16] = 2 ** 31 - 1
    link[5 * 4 + 3] = 0                # (dq != dr)
    link[5 * 5 + 0] = 7                # a chain start: no link, whatever link says
    exp = check(arrs, nc, K, link, 0, "inconsistent link")
    text = rows(exp[0], exp[1])
    assert text[1] == "25=" and text[3] == "" and text[6] == "5=1X19=" and text[8] == rows(*CM.chain_cigars_model(*arrs, nc, K, ed.link)[:2])[8] != ""
    assert [text[i] for i in (11, 12, 13, 14, 16, 23, 25)] == [""] * 7
    # too small: a link with two edits asked for with 1
    B2 = Batch(44)
    b2 = bases(B2.rng, 40)
    B2.add([(b2, sub(B2.rng, b2, [3, 30]))])
    arrs2 = B2.arrays()
    for e, n_runs in ((1, 0), (2, 5), (3, 5)):
        exp2 = check(arrs2, 1, K, np.array([-1, e], dtype=np.int32), 0, "too small")
        assert len(exp2[1]) == n_runs
    # pred and chain out of range, unkept chains
    pred, chain = pred.copy(), chain.copy()
    pred[31] = -1; pred[32] = 32; pred[33] = m; pred[34] = 2 ** 31 - 1; pred[36] = -7; pred[37] = 40
    chain[41] = -1; chain[46] = nc; chain[47] = 2 ** 31 - 1; chain[50] = -1; chain[56] = 0
    bad = (qt, rt, q, r, v, pred, chain)
    exp = check(bad, nc, K, ed.link, 0, "pred and chain out of range")
    text = rows(exp[0], exp[1])
    assert [text[i] for i in (31, 32, 33, 34, 36, 37, 41, 46, 47, 50, 51, 56, 57)] == [""] * 13 and text[42] == "" and text[43] != ""
    # no chain kept at all: every row is empty and the call needs no chain rows
    got = run_dev(arrs, 0, K, ed.link)
    assert (got[0] == 0).all() and len(got[1]) == 0 and len(got[2]) == 0 and len(got[3]) == 0
    # positions beyond 2^31 and strings of 2^28 bases: empty rows, nothing is read
    far = (qt, rt, q, r.copy(), v, B.arrays()[5], B.arrays()[6])
    far[3][1] = 2 ** 31 + 5
    exp = check(far, nc, K, ed.link, 0, "far positions")
    assert rows(exp[0], exp[1])[1] == ""


# ---- call conventions
def test_count_only_too_small_a_capacity_and_refusals(shapes):
    from kmerhash_amd import _capi
    import ctypes as C
    B, want, arrs = shapes[0]
    link = real_link(arrs, B.n_chains, K).link
    exp = CM.chain_cigars_model(*arrs, B.n_chains, K, link)
    m, nc, total = len(link), B.n_chains, len(exp[1])
    f = _capi.lib().kh_chain_cigars
    for where, conv in ((_capi.KH_MEM_HOST, lambda a: a), (_capi.KH_MEM_DEVICE, to_dev)):
        ins = [conv(a) for a in arrs + (link,)]
        ptr = (lambda t: t.ctypes.data) if where == _capi.KH_MEM_HOST else (lambda t: t.data_ptr())
        host = (lambda t: t) if where == _capi.KH_MEM_HOST else (lambda t: t.cpu().numpy())
        stream = None if where == _capi.KH_MEM_HOST else torch.cuda.current_stream().cuda_stream

        def call(t_ops, cap, t_offs, t_ci, t_cd, n_out, **kw):
            a = dict(k=K, m=m, nc=nc, where=where, offs=ptr(t_offs), ci=ptr(t_ci), cd=ptr(t_cd), n=C.byref(n_out), link=ptr(ins[7]), qt=ptr(ins[0]))
            a.update(kw)
            return f(a["qt"], arrs[0].size, ptr(ins[1]), arrs[1].size, 0, *(ptr(t) for t in ins[2:7]), a["m"], a["nc"], a["k"], a["link"], a["where"], a["offs"],
                     None if t_ops is None else ptr(t_ops), cap, a["n"], a["ci"], a["cd"], 0, stream)

        def fresh():
            return (conv(np.full(total + 8, 0x5A5A5A5A, dtype=np.uint32)), conv(np.full(m + 1, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)),
                    conv(np.full(nc, 0x5A5A5A5A, dtype=np.uint32)), conv(np.full(nc, 0x5A5A5A5A, dtype=np.uint32)))
        # count only
        ops, offs, ci, cd = fresh()
        n = C.c_uint64(77)
        assert call(None, 0, offs, ci, cd, n) == _capi.KH_OK and n.value == total
        torch.cuda.synchronize()
        assert np.array_equal(host(offs).view(np.uint64), exp[0]) and np.array_equal(host(ci).view(np.uint32), exp[2]) and np.array_equal(host(cd).view(np.uint32), exp[3])
        # one run too few: an error, the count and the offsets all the same, the rows untouched
        ops, offs, ci, cd = fresh()
        n = C.c_uint64(77)
        assert call(ops, total - 1, offs, ci, cd, n) == _capi.KH_ERR_INVALID and n.value == total
        torch.cuda.synchronize()
        assert np.array_equal(host(offs).view(np.uint64), exp[0]) and (host(ops).view(np.uint32) == 0x5A5A5A5A).all()
        # exactly enough
        n = C.c_uint64(77)
        assert call(ops, total, offs, ci, cd, n) == _capi.KH_OK and n.value == total
        torch.cuda.synchronize()
        assert np.array_equal(host(ops).view(np.uint32)[:total], exp[1]) and (host(ops).view(np.uint32)[total:] == 0x5A5A5A5A).all()
        # the refusals: nothing is written
        ops, offs, ci, cd = fresh()
        n = C.c_uint64(77)
        for kw in (dict(k=0), dict(k=65), dict(m=2 ** 24 + 1), dict(where=7), dict(ci=None), dict(cd=None), dict(offs=None), dict(n=None), dict(link=None), dict(qt=None)):
            assert call(ops, total + 8, offs, ci, cd, n, **kw) == _capi.KH_ERR_INVALID, kw
        torch.cuda.synchronize()
        assert n.value == 77 and all((host(t).view(np.uint32) == 0x5A5A5A5A).all() for t in (ops, offs, ci, cd))


def test_python_refusals():
    t = b"ACGT" * 8
    q, r, v = np.arange(8, dtype=np.uint32), np.arange(8, dtype=np.uint32), np.zeros(8, dtype=np.uint8)
    pred, chain, link = np.arange(-1, 7, dtype=np.int32), np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
    with pytest.raises(ValueError, match="same memory"):
        kh.chain_cigars(t, t, q, r, v, pred, chain, 1, 4, to_dev(link))
    with pytest.raises(ValueError, match="one entry per anchor"):
        kh.chain_cigars(t, t, q, r, v, pred, chain, 1, 4, link[:7])
