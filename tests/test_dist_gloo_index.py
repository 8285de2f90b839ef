"""CPU: the sharded position index (kmerhash_amd.dist_index.ShardedKmerPositionIndex) on world sizes 2 and 3 over gloo.  The
device-specific pieces come from a test-local CPU backend -- IndexModel over the accumulated pairs as the local index, np_kmers_pos /
np_minimizers as text_pairs, the oracle hash for shard, np_csr_unpermute -- the role OracleBackend plays in tests/test_dist_gloo.py; the
exchange logic under test is the code the GPU ranks run over RCCL.  Everything is compared with ONE IndexModel over the pairs of all
ranks, exactly."""
import os
import socket
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

K = 15
M32 = np.uint64(0xFFFFFFFF)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _u64(t):
    return t.numpy().view(np.uint64)


class ModelIndex:
    """the local index of the CPU backend: the pairs given so far, answered by IndexModel"""

    def __init__(self, IndexModel):
        self.M = IndexModel
        self.clear()

    def clear(self):
        self.k, self.p = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)

    def model(self):
        return self.M(self.k, self.p)

    def append(self, keys, pos):
        self.k = np.concatenate([self.k, _u64(keys)])
        self.p = np.concatenate([self.p, pos.numpy().view(np.uint32)])
        return len(keys)

    def build(self, keys, pos):
        assert len(self.k) == 0
        return self.append(keys, pos)

    def size(self):
        return len(np.unique(self.k))

    def total(self):
        return len(self.k)

    def count(self, keys):
        return torch.from_numpy(self.model().count(_u64(keys)).view(np.int32).copy())

    def find(self, keys):
        offs, pos = self.model().find(_u64(keys))
        return torch.from_numpy(offs.astype(np.int64)), torch.from_numpy(pos.view(np.int32).copy())

    def _drop(self, m):
        out = len(np.unique(self.k[m])), int(m.sum())
        self.k, self.p = self.k[~m], self.p[~m]
        return out

    def erase(self, keys):
        return self._drop(np.isin(self.k, _u64(keys)))

    def erase_counts(self, lo, hi):
        uk, cnt = np.unique(self.k, return_counts=True)
        return self._drop(np.isin(self.k, uk[(cnt >= lo) & (cnt <= hi)]))

    def drop_above(self, max_occ):
        return self.erase_counts(max_occ + 1, 2 ** 32 - 1)


class ModelBackend:
    def __init__(self, O, w):
        from index_model import IndexModel, np_kmers_pos
        from minimizer_model import np_minimizers
        from csr_model import np_csr_unpermute
        self.O, self.w = O, w
        self.kmers_pos, self.minimizers, self.unpermute = np_kmers_pos, np_minimizers, np_csr_unpermute
        self.torch_device = torch.device("cpu")
        self.index = ModelIndex(IndexModel)

    def owner(self, k, p):
        from kmerhash_amd.dist import DIST_SEED
        if len(k) == 0:
            return np.zeros(0, dtype=np.int64)
        return (self.O.hash_batch(self.O.HASH_MURMUR3_X86, DIST_SEED, np.ascontiguousarray(k)) % np.uint64(p)).astype(np.int64)

    def shard(self, keys, vals, p):
        k = _u64(keys)
        r = self.owner(k, p)
        order = np.argsort(r, kind="stable")
        ok = torch.from_numpy(k[order].view(np.int64).copy())
        ov = torch.from_numpy(vals.numpy()[order].copy()) if vals is not None else None
        return ok, ov, np.bincount(r, minlength=p).tolist()

    def empty(self, n, dtype):
        return torch.empty(n, dtype=dtype)

    def pairs_np(self, text):
        text = np.asarray(text, dtype=np.uint8)
        return self.kmers_pos(text, K, True) if self.w is None else self.minimizers(text, K, self.w, True, "murmur", 42)

    def text_pairs(self, text, fastq=False):
        assert not fastq
        km, pos = self.pairs_np(text)
        return torch.from_numpy(km.view(np.int64).copy()), torch.from_numpy(pos.view(np.int32).copy())

    def csr_unpermute(self, counts_perm, pos_perm, origin):
        cp = counts_perm.numpy().view(np.uint32)
        if pos_perm is None:                                 # counts only: segments of length zero would do, the model wants real ones
            c, _, _ = self.unpermute(cp, np.zeros(int(cp.sum()), dtype=np.uint32), origin.numpy())
            return torch.from_numpy(c.view(np.int32).copy())
        _, offs, pos = self.unpermute(cp, pos_perm.numpy().view(np.uint32), origin.numpy())
        return torch.from_numpy(offs.astype(np.int64)), torch.from_numpy(pos.view(np.int32).copy())


def make_text(rank):
    """~20 000 bases of this rank: random, a few Ns, one poly-A stretch of 300 and one 2 000-base block every rank holds"""
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    rng = np.random.default_rng(1000 + rank)
    t = lut[rng.integers(0, 4, 20_000)].copy()
    t[3000 + 500 * rank: 5000 + 500 * rank] = lut[np.random.default_rng(77).integers(0, 4, 2000)]       # the shared block, at its own offset
    t[12_000 + 100 * rank: 12_300 + 100 * rank] = ord("A")
    t[rng.integers(0, 20_000, 5)] = ord("N")
    return t


def _delta(st, before):
    return {k: v - before[k] for k, v in st.collectives.items()}


def _run(rank, world, O, w):
    from index_model import IndexModel
    from kmerhash_amd.dist import ShardPeerError
    from kmerhash_amd.dist_index import ShardedKmerPositionIndex
    be = ModelBackend(O, w)
    st = ShardedKmerPositionIndex(be)
    assert st.local is be.index and st.p == world
    text, base = make_text(rank), rank << 20
    # ---- append_sequences in two batches
    halves = ((text[:10_000], base), (text[10_000:], base + 10_000))
    mine_k, mine_p = [], []
    for part, pb in halves:
        c0 = dict(st.collectives)
        km, pos = be.pairs_np(part)
        assert st.append_sequences(part, pos_base=pb) == len(km)
        assert _delta(st, c0) == {"counts": 1, "payload": 1, "votes": 3, "reduce": 0}, st.collectives
        mine_k.append(km)
        mine_p.append(pos + np.uint32(pb))
    allk, allp = [None] * world, [None] * world
    dist.all_gather_object(allk, np.concatenate(mine_k))
    dist.all_gather_object(allp, np.concatenate(mine_p))
    gk, gp = np.concatenate(allk), np.concatenate(allp)
    model = IndexModel(gk, gp)
    assert len(np.unique(gp >> np.uint32(20))) == world                   # every rank's coordinate space is in the index

    def check_content(gk, gp):
        """all local indexes together hold exactly the pairs (gk, gp), every key on the rank the dist hash names"""
        lk, lp = be.index.k, be.index.p
        assert (be.owner(lk, world) == rank).all()
        m = be.owner(gk, world) == rank
        a = np.lexsort((lp, lk))
        b = np.lexsort((gp[m], gk[m]))
        assert np.array_equal(lk[a], gk[m][b]) and np.array_equal(lp[a], gp[m][b])

    check_content(gk, gp)
    c0 = dict(st.collectives)
    assert st.size() == model.size() and st.total() == model.total() == len(gk)
    assert _delta(st, c0) == {"counts": 0, "payload": 0, "votes": 0, "reduce": 2}
    assert int(model.count(np.zeros(1, dtype=np.uint64))[0]) > 50 * world    # the poly-A key holds positions from every rank
    # ---- count / find in QUERY order: hits (own and other ranks'), misses, repeats, the poly-A key; one rank's batch is empty
    rng = np.random.default_rng(5 + rank)
    hits = gk[rng.integers(0, len(gk), 700)]
    q = np.concatenate([hits, rng.integers(0, 1 << 30, 300).astype(np.uint64), hits[:100], np.zeros(2, dtype=np.uint64), hits[:3]])
    q = q[rng.permutation(len(q))]
    if rank == 1:
        q = q[:0]
    tq = torch.from_numpy(q.view(np.int64).copy())
    c0 = dict(st.collectives)
    cnt = st.count(tq)
    assert _delta(st, c0) == {"counts": 1, "payload": 2, "votes": 2, "reduce": 0}, st.collectives
    assert cnt.dtype == torch.int32 and np.array_equal(cnt.numpy().view(np.uint32), model.count(q))
    c0 = dict(st.collectives)
    offs, pos = st.find(tq)
    assert _delta(st, c0) == {"counts": 2, "payload": 2, "votes": 2, "reduce": 0}, st.collectives
    eo, ep = model.find(q)
    assert offs.dtype == torch.int64 and np.array_equal(offs.numpy().astype(np.uint64), eo)
    assert np.array_equal(pos.numpy().view(np.uint32), ep)
    if rank != 1:
        assert (model.count(q) == 0).any() and (model.count(q) > 1).any() and int(eo[-1]) > 600
    assert np.array_equal(st.find(q)[0].numpy(), offs.numpy())            # numpy keys are taken as well
    # ---- find_sequences: a query text of this rank, sampled as the index samples
    qt = np.concatenate([make_text((rank + 1) % world)[2500:6500], text[11_900:12_500]])
    qk, qp = be.pairs_np(qt)
    c0 = dict(st.collectives)
    qpos, offs, pos = st.find_sequences(qt)
    assert _delta(st, c0) == {"counts": 2, "payload": 2, "votes": 2, "reduce": 0}
    eo, ep = model.find(qk)
    assert np.array_equal(qpos.numpy().view(np.uint32), qp) and len(qp) > 300
    assert np.array_equal(offs.numpy().astype(np.uint64), eo) and np.array_equal(pos.numpy().view(np.uint32), ep)
    # ---- erase: the global pair of counts, the model's content afterwards
    ek = np.concatenate([allk[rank][:400], allk[(rank + 1) % world][:200], rng.integers(0, 1 << 30, 50).astype(np.uint64)])
    alle = [None] * world
    dist.all_gather_object(alle, ek)
    gone = np.isin(gk, np.concatenate(alle))
    c0 = dict(st.collectives)
    assert st.erase(torch.from_numpy(ek.view(np.int64).copy())) == (len(np.unique(gk[gone])), int(gone.sum()))
    assert _delta(st, c0) == {"counts": 1, "payload": 1, "votes": 2, "reduce": 1}, st.collectives
    gk, gp = gk[~gone], gp[~gone]
    check_content(gk, gp)
    # ---- drop_above(50): a k-mer lives whole on its owner, its global occurrence count is local
    uk, ucnt = np.unique(gk, return_counts=True)
    gone = np.isin(gk, uk[ucnt > 50])
    assert gone.any()
    c0 = dict(st.collectives)
    assert st.drop_above(50) == (int((ucnt > 50).sum()), int(gone.sum()))
    assert _delta(st, c0) == {"counts": 0, "payload": 0, "votes": 0, "reduce": 1}
    gk, gp = gk[~gone], gp[~gone]
    check_content(gk, gp)
    assert st.erase_counts(3, 2) == (0, 0)                                # the empty range
    assert (st.size(), st.total()) == (len(np.unique(gk)), len(gk))
    # ---- a rank that fails locally, at every stage of every exchanging call: every rank raises (the failing one its own error, the
    #      others ShardPeerError), nobody hangs; a collective clear() and a new build work
    import time
    km, pos = be.pairs_np(text)
    ntot = [None] * world
    dist.all_gather_object(ntot, len(km))
    bad = world - 1
    for op in ("append", "count", "find", "erase"):
        for stage in (1, 2, 3, 4):
            if rank == bad:
                st._fail_stage = stage
            t0 = time.time()
            try:
                if op == "append":
                    st.append_sequences(text, pos_base=base)
                elif op == "count":
                    st.count(tq)
                elif op == "find":
                    st.find(tq)
                else:
                    st.erase(tq)
                raised = None
            except MemoryError:
                raised = "own"
            except ShardPeerError:
                raised = "peer"
            assert raised == ("own" if rank == bad else "peer"), (op, stage, rank, raised)
            assert time.time() - t0 < 60 and st._fail_stage == 0
            st.clear()
            assert st.total() == 0
            assert st.build_sequences(text, pos_base=base) == len(km)
            assert st.total() == sum(ntot)
    with pytest.raises((ValueError, ShardPeerError)):                     # build needs an empty index: refused on every rank
        st.build_sequences(text, pos_base=base)
    with pytest.raises((ValueError, ShardPeerError)):                     # 32-bit positions
        st.append_sequences(text, pos_base=2 ** 32 - 100 if rank == 0 else 0)
    assert st.total() == sum(ntot)
    for name in ("insert", "insert_counts", "value_histogram", "erase_values", "_query"):     # a table operation cannot be called on it
        assert not hasattr(st, name), name


def _worker(rank, world, port, q):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import oracle_py as O
        for w in (None, 10):                                  # all windows, then (10,15)-minimizers
            _run(rank, world, O, w)
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def collect(procs, q, seconds):
    """one result per process; a process that ends without one ends the wait"""
    import queue
    import time
    res, t0 = [], time.time()
    while len(res) < len(procs) and time.time() - t0 < seconds:
        try:
            res.append(q.get(timeout=0.5))
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs) or all(p.exitcode is not None for p in procs):
                break
        if any(isinstance(r, tuple) and r[1] != "ok" for r in res):
            break
    for p in procs:
        p.join(5 if len(res) == len(procs) else 0.1)
        if p.is_alive():
            p.kill()
    return res


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])      # 3: owner = hash % p (not a power of two)
def test_sharded_position_index_gloo(oracle, world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = collect(procs, q, 240)
    assert len(res) == world and all(r[1] == "ok" for r in res), res
