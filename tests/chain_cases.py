"""TEST HELPER (not collected): anchor lists for the chaining tests -- collinear runs with jitter, segment lists, and the comparison of
kmerhash_amd.chain_anchors with the model of tests/chain_model.py on all seven outputs, for host and for device memory."""
import numpy as np

import chain_model as CM

FIELDS = ("score", "pred", "chain", "first", "last", "count", "cscore")


def collinear(rng, n, rev=0, q0=0, r0=1000, step=12, jitter=2, noise=0.0, span=4000):
    """n anchors along one diagonal of strand `rev`: query steps of 1..step, reference steps that differ by up to `jitter`; a share
    `noise` of them are random hits instead.  -> (q, r, v) lists in query order"""
    d = rng.integers(1, step + 1, n)
    e = np.maximum(1, d + rng.integers(-jitter, jitter + 1, n))
    q = q0 + np.cumsum(d)
    r = r0 + np.cumsum(e) if rev == 0 else r0 + n * (step + jitter) + 10 - np.cumsum(e)
    v = np.full(n, rev)
    hit = rng.random(n) < noise
    r = np.where(hit, rng.integers(0, span, n), r)
    v = np.where(hit, rng.integers(0, 2, n), v)
    return q.tolist(), r.tolist(), v.tolist()


def segment_list(rng, lengths, noise=0.0, shuffle=()):
    """one collinear run per entry of `lengths`, strands alternating -> (q, r, v, seg_offsets); the segments whose number is in `shuffle`
    get their anchors in random order"""
    q, r, v, seg = [], [], [], [0]
    for s, n in enumerate(lengths):
        a, b, c = collinear(rng, n, rev=s & 1, q0=int(rng.integers(0, 50)), noise=noise)
        if s in shuffle:
            p = rng.permutation(n)
            a, b, c = [a[i] for i in p], [b[i] for i in p], [c[i] for i in p]
        q += a; r += b; v += c
        seg.append(len(q))
    return q, r, v, seg


def arrays(q, r, v, seg=None):
    return (np.asarray(q, dtype=np.uint64).astype(np.uint32), np.asarray(r, dtype=np.uint64).astype(np.uint32), np.asarray(v, dtype=np.uint8),
            None if seg is None else np.asarray(seg, dtype=np.uint64))


def to_dev(a):
    import torch
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(np.ascontiguousarray(a).view(view) if view is not None else np.ascontiguousarray(a)).cuda()


def assert_same(got, exp, what=""):
    for name in FIELDS:
        g, e = getattr(got, name), getattr(exp, name)
        if not isinstance(g, np.ndarray):
            g = g.cpu().numpy()
        g = g.view(e.dtype) if g.dtype != e.dtype else g
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        bad = np.flatnonzero(g != e)
        assert bad.size == 0, (what, name, "first difference at %d: got %d, model %d (%d differ)" % (bad[0], g[bad[0]], e[bad[0]], bad.size))


def check(q, r, v, k, seg=None, where=("host", "device"), **params):
    """chain_anchors == model on all seven outputs, in each memory -> the model's result"""
    import kmerhash_amd as kh
    exp = CM.chain(q, r, v, k, seg, **params)
    aq, ar, av, aseg = arrays(q, r, v, seg)
    for w in where:
        if w == "host":
            got = kh.chain_anchors(aq, ar, av, k, aseg, **params)
            assert all(isinstance(x, np.ndarray) for x in got)
        else:
            got = kh.chain_anchors(to_dev(aq), to_dev(ar), to_dev(av), k, None if aseg is None else to_dev(aseg), **params)
            assert all(x.is_cuda for x in got)
        assert_same(got, exp, w)
    return exp
