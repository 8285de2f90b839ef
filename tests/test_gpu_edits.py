"""GPU: kh_chain_edits against the model of tests/edits_model.py, exactly: link, edits and over, for host arrays and for CUDA tensors.
pred and chain are built by hand (the chainer is not involved); the texts are random bases with planted edits.  The shapes are the
smallest at which the kernels can go wrong: link lengths around the 8-base words of the compare, the edge diagonals of the wavefront
pass, the ends of both texts, every way an anchor can have no link, and a worklist longer than the grid of the wavefront kernel."""
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import edits_model as EM  # noqa: E402
from edits_cases import K, Batch, bases, other, revcomp, sub  # noqa: E402
from stream_checks import to_dev  # noqa: E402

def run_host(arrs, n_chains, k, ref_base, max_edits):
    got = kh.chain_edits(*arrs, n_chains, k, ref_base=ref_base, max_edits=max_edits)
    assert got.link.dtype == np.int32 and got.edits.dtype == np.uint32 and got.over.dtype == np.uint32
    return got.link, got.edits, got.over


def run_dev(arrs, n_chains, k, ref_base, max_edits):
    got = kh.chain_edits(*(to_dev(a) for a in arrs), n_chains, k, ref_base=ref_base, max_edits=max_edits)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in got)
    torch.cuda.synchronize()
    return got.link.cpu().numpy(), got.edits.cpu().numpy().view(np.uint32), got.over.cpu().numpy().view(np.uint32)


def check(arrs, n_chains, k, ref_base, max_edits, exp, what):
    for name, run in (("host", run_host), ("device", run_dev)):
        link, edits, over = run(arrs, n_chains, k, ref_base, max_edits)
        bad = np.flatnonzero(link != exp[0])
        assert bad.size == 0, (what, name, max_edits, bad[:8].tolist(), link[bad[:8]].tolist(), exp[0][bad[:8]].tolist())
        assert np.array_equal(edits, exp[1]) and np.array_equal(over, exp[2]), (what, name, max_edits)


# ---- the word boundaries of the compare, indels, the edge diagonals, N and lower case: one batch, both strands, several max_edits
LENGTHS = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65]


def build_small(ref_base):
    B = Batch(11, ref_base=ref_base)
    rng, known = B.rng, {}
    for rev in (0, 1):
        for L in LENGTHS:
            a = bases(rng, L)
            known[B.add([(a, a)], rev)] = 0
            for p in sorted({0, L - 1, 7, 8, (L // 8) * 8 - 1, (L // 8) * 8} & set(range(L))):
                known[B.add([(a, sub(rng, a, [p]))], rev)] = 1
                known[B.add([(sub(rng, a, [p]), a)], rev)] = 1
        a = bases(rng, 40)
        known[B.add([(a, a[:20] + bytes([other(rng, a[20])]) + a[20:])], rev)] = 1        # one base more in the reference
        known[B.add([(a, a[:20] + a[21:])], rev)] = None                                   # one base less (1, or 0 inside a run)
        a = bases(rng, 50)
        ins = bases(rng, 32)
        B.add([(a, a[:25] + ins[:31] + a[25:])], rev)            # dr - dq = +31: the top lane
        B.add([(a[:25] + ins[:31] + a[25:], a)], rev)            # dr - dq = -31: lane 1
        B.add([(a, a[:25] + ins + a[25:])], rev)                 # +32: over
        B.add([(a[:25] + ins + a[25:], a)], rev)                 # -32: over
        a = bases(rng, 120)
        for n in (1, 5, 6, 31, 32):                              # exactly max_edits and one more, for max_edits 0, 5 and 31
            B.add([(a, sub(rng, a, [3 * t + 1 for t in range(n)]))], rev)
        a = bases(rng, 30)
        B.add([(a.lower(), a)], rev); B.add([(a, a.lower())], rev)
        B.add([(a[:10] + b"N" + a[11:], a)], rev); B.add([(a, a[:10] + b"N" + a[11:])], rev)
        B.add([(a[:10] + b"N" + a[11:], a[:10] + b"N" + a[11:])], rev)                     # N against N: one edit
        B.add([(a[:10] + b"n" + a[11:], a[:10] + b"R" + a[11:])], rev)
        B.add([(a, a[:29] + b"-")], rev); B.add([(b"N", b"N")], rev); B.add([(b"N" * 9, b"N" * 9)], rev)
        # a chain of 200 links, every seventh with one substitution
        pairs = []
        for t in range(200):
            a = bases(rng, rng.randrange(3, 30))
            pairs.append((a, sub(rng, a, [len(a) // 2]) if t % 7 == 0 else a))
        B.add(pairs, rev)
    return B, known


@pytest.fixture(scope="module")
def small():
    out = {}
    for ref_base in (0, 100003):
        B, known = build_small(ref_base)
        arrs = B.arrays()
        exp = {me: EM.chain_edits_model(*arrs, B.n_chains, K, ref_base, me, banded=(me == 31)) for me in (0, 5, 31)}
        out[ref_base] = (B, known, arrs, exp)
    return out


def test_the_model_sees_the_planted_edits(small):
    B, known, arrs, exp = small[0]
    link = exp[31][0]
    for i, d in known.items():
        assert d is None or link[i] == d, (i, d, link[i])
    assert (link == 31).sum() >= 4 and (link == EM.OVER).sum() >= 4            # the edge lanes; +-32 and 32 substitutions
    assert (exp[5][0] == 5).sum() >= 2 and (exp[0][0] == EM.OVER).sum() > (exp[5][0] == EM.OVER).sum() > (link == EM.OVER).sum()
    c200 = [c for c in range(B.n_chains) if B.chain.count(c) == 201]
    assert len(c200) == 2 and all(exp[31][1][c] == 29 and exp[31][2][c] == 0 for c in c200)      # ceil(200 / 7) links with one edit


@pytest.mark.parametrize("ref_base", [0, 100003])
@pytest.mark.parametrize("max_edits", [0, 5, 31])
def test_small_shapes(small, ref_base, max_edits):
    B, known, arrs, exp = small[ref_base]
    check(arrs, B.n_chains, K, ref_base, max_edits, exp[max_edits], "small shapes")


def test_long_links():
    B = Batch(12)
    rng = B.rng
    for rev in (0, 1):
        a = bases(rng, 5000)
        B.add([(a, a)], rev)
        B.add([(a, sub(rng, a, [10 + 160 * t for t in range(31)]))], rev)          # 31 substitutions spread over the link
        b = sub(rng, a, [17 + 330 * t for t in range(15)])
        for t in range(8):                                                          # 15 substitutions, 8 insertions and 8 deletions: 31
            b = b[:200 + 600 * t] + bytes([other(rng, b[200 + 600 * t])]) + b[200 + 600 * t:400 + 600 * t] + b[401 + 600 * t:]
        B.add([(a, b)], rev)
        B.add([(a, sub(rng, a, [10 + 150 * t for t in range(32)]))], rev)          # 32: over
    arrs = B.arrays()
    exp = EM.chain_edits_model(*arrs, B.n_chains, K, 0, 31, banded=True)
    assert exp[0][exp[0] != EM.NOLINK].tolist() == [0, 31, 31, EM.OVER] * 2
    check(arrs, B.n_chains, K, 0, 31, exp, "long links")


# ---- the ends of the texts, with a guard behind every device buffer
def edge_case(rev, cut_q, cut_r, low):
    """one link whose strings end exactly at the end of both texts (forward: B is the whole of rtext); cut_q / cut_r take the last byte
    off a text, low raises ref_base so that B's stretch would start one byte before rtext"""
    B = Batch(13 + rev, k=K, ref_base=50)
    a = bases(B.rng, 20)
    B.q += a + bases(B.rng, K)
    if rev:
        B.r += bases(B.rng, K) + revcomp(a)                       # the stretch [r_i + k, r_j + k) is the end of rtext
        B.qpos, B.rpos, B.rev, B.pred, B.chain, B.n_chains = [0, 20], [70, 50], [1, 1], [-1, 0], [0, 0], 1
    else:
        B.r += a                                                   # r_i - ref_base == nr: allowed, the forward bounds carry no + k
        B.qpos, B.rpos, B.rev, B.pred, B.chain, B.n_chains = [0, 20], [50, 70], [0, 0], [-1, 0], [0, 0], 1
    qt, rt, *rest = B.arrays()
    return (qt[:len(qt) - cut_q], rt[:len(rt) - cut_r], *rest), 50 + low * (K + 1 if rev else 1)


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("cut", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)])
def test_text_ends_and_guards(rev, cut):
    from kmerhash_amd import _capi
    arrs, ref_base = edge_case(rev, *cut)
    exp = EM.chain_edits_model(*arrs, 1, K, ref_base, 31)
    want = 0 if cut == (0, 0, 0) else EM.OVER
    assert exp[0].tolist() == [EM.NOLINK, want]
    check(arrs, 1, K, ref_base, 31, exp, "text ends")
    # device buffers with 64 guard elements behind each (valid bases behind the texts, zeros behind the arrays): the answers above hold
    # with them in place, and nothing is written past the end of an output or into a guard
    G = 64
    ins = []
    for a in arrs:
        t = torch.full((a.size + G,), 65 if a.dtype == np.uint8 and a.size > 2 else 0, dtype=to_dev(a[:1]).dtype, device="cuda")
        t[:a.size] = to_dev(a)
        ins.append(t)
    outs = [torch.full((n + G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for n in (2, 1, 1)]
    st = _capi.lib().kh_chain_edits(ins[0].data_ptr(), arrs[0].size, ins[1].data_ptr(), arrs[1].size, ref_base, *(t.data_ptr() for t in ins[2:]), 2, 1, K, 31,
                                    _capi.KH_MEM_DEVICE, *(t.data_ptr() for t in outs), 0, torch.cuda.current_stream().cuda_stream)
    assert st == _capi.KH_OK
    torch.cuda.synchronize()
    assert outs[0][:2].tolist() == [EM.NOLINK, want] and outs[1][0].item() == 0 and outs[2][0].item() == (1 if want == EM.OVER else 0)
    for t, n in zip(outs, (2, 1, 1)):
        assert (t[n:] == 0x5A5A5A5A).all()
    for t, a in zip(ins, arrs):
        assert (t[a.size:] == (65 if a.dtype == np.uint8 and a.size > 2 else 0)).all()


def test_anchors_without_a_link():
    B = Batch(17)
    rng = B.rng
    a = bases(rng, 25)
    for rev in (0, 1):
        for _ in range(8):
            B.add([(a, sub(rng, a, [5])), (a, a)], rev)
    qt, rt, q, r, v, pred, chain = B.arrays()
    m, nc = len(q), B.n_chains
    pred, chain = pred.copy(), chain.copy()
    # chain c is the anchors 3c, 3c + 1, 3c + 2
    pred[1] = -1                                                   # no predecessor
    pred[4] = 4; pred[7] = 8                                       # pred >= i
    pred[10] = m; pred[13] = m + 1000; pred[16] = 2 ** 31 - 1      # pred >= m
    pred[19] = -7
    chain[22] = -1; chain[25] = nc; chain[28] = 2 ** 31 - 1        # not kept / beyond the table
    chain[30] = -1                                                 # the predecessor of 31 is in no chain
    pred[34] = 0                                                   # a predecessor in another chain
    chain[37] = chain[36] = 0                                      # ... and one that moved into chain 0 with its successor: a link of chain 0
    arrs = (qt, rt, q, r, v, pred, chain)
    exp = EM.chain_edits_model(*arrs, nc, K, 0, 31)
    for i in (1, 4, 7, 10, 13, 16, 19, 22, 25, 28, 31, 34):
        assert exp[0][i] == EM.NOLINK
    assert exp[0][37] == 1 and exp[0][2] == 0 and exp[1][0] == 1
    check(arrs, nc, K, 0, 31, exp, "no link")
    # no chain kept at all: every anchor is NOLINK and the call needs no chain rows
    link, edits, over = run_dev(arrs, 0, K, 0, 31)
    assert (link == EM.NOLINK).all() and len(edits) == 0 and len(over) == 0


def test_worklist_longer_than_the_grid_and_identical_bytes():
    """more unsettled links than the wavefront kernel has waves (8 blocks of 4 per compute unit): the grid-stride loop over the
    device-side count; every link has one substitution, so the expected value needs no model (which checks the first 300)"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n_links = ncu * 8 * 4 + 1500
    rng = random.Random(19)
    L, k = 12, 4
    a = bases(rng, L)
    variants = [sub(rng, a, [p]) for p in range(L)]
    qt = (a + b"ACGT") * n_links
    rt = b"".join(variants[t % L] + b"ACGT" for t in range(n_links))
    step = L + k
    q = np.repeat(np.arange(n_links, dtype=np.uint32) * step, 2); q[1::2] += L
    pred = np.full(2 * n_links, -1, dtype=np.int32); pred[1::2] = np.arange(0, 2 * n_links, 2)
    chain = np.repeat(np.arange(n_links, dtype=np.int32) % 50, 2)
    arrs = (np.frombuffer(qt, dtype=np.uint8).copy(), np.frombuffer(rt, dtype=np.uint8).copy(), q, q.copy(), np.zeros(2 * n_links, dtype=np.uint8), pred, chain)
    head = tuple(x[:600] for x in arrs[2:])
    exp_head = EM.chain_edits_model(arrs[0], arrs[1], *head, 50, k, 0, 3)
    link = np.full(2 * n_links, EM.NOLINK, dtype=np.int32); link[1::2] = 1
    assert np.array_equal(exp_head[0], link[:600])
    edits = np.bincount(np.arange(n_links) % 50, minlength=50).astype(np.uint32)
    exp = (link, edits, np.zeros(50, dtype=np.uint32))
    check(arrs, 50, k, 0, 3, exp, "long worklist")
    one, two = run_dev(arrs, 50, k, 0, 3), run_dev(arrs, 50, k, 0, 3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))


def test_fuzz():
    rng = random.Random(23)
    B = Batch(23, ref_base=777)
    for t in range(2000):
        a = bytearray(bases(rng, rng.randrange(4, 60)))
        rate = rng.choice([0.0, 0.02, 0.05, 0.1, 0.15])
        b = bytearray()
        for c in a:
            u = rng.random()
            if u < rate / 3:
                continue
            if u < 2 * rate / 3:
                b.append(rng.choice(b"ACGT"))
            b.append(other(rng, c) if 2 * rate / 3 <= u < rate else c)
        if t % 50 == 0:
            a[len(a) // 2] = ord("N")
        if t % 9 == 0:
            a = bytearray(bytes(a).lower())
        B.add([(bytes(a), bytes(b) or b"A")], rev=t & 1)
    arrs = B.arrays()
    for me in (4, 15):
        exp = EM.chain_edits_model(*arrs, B.n_chains, K, 777, me, banded=True)
        lk = exp[0][exp[0] != EM.NOLINK]
        assert (lk == 0).sum() > 300 and (lk > 0).sum() > 300 and (me != 4 or (lk == EM.OVER).sum() > 20), (me, np.bincount(lk + 2))
        check(arrs, B.n_chains, K, 777, me, exp, "fuzz")
    one, two = run_dev(arrs, B.n_chains, K, 777, 15), run_dev(arrs, B.n_chains, K, 777, 15)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))
