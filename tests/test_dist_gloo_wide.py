"""CPU: kmerhash_amd.dist.ShardedTable over a backend with 16-byte keys (key_words = 2: a batch of keys is an (n, 2) tensor, a key
is a row) on world size 2 and 3 over gloo.  The backend lives in this file: its local table is a Python dict keyed by (w0, w1), its
shard() a stable argsort by a fixed rank function of BOTH words.  The model is one dict per rank fed the ranks' batches in the
documented receive order -- piece, then source rank, then position -- so first-value-wins across ranks and pieces is checked, and a
layer that flattens the key rows (numel() instead of shape[0], 1-D receive buffers) cannot pass."""
import os
import socket

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def rank_of(k, p):
    """k: (n, 2) uint64 -> destination rank; both words matter (keys that differ in one word only land on different ranks)"""
    w0, w1 = k[:, 0], k[:, 1]
    h = (w0 * np.uint64(0x9E3779B97F4A7C15)) ^ (w1 * np.uint64(0xC2B2AE3D27D4EB4F) + (w1 >> np.uint64(29)))
    h ^= h >> np.uint64(31)
    return ((h >> np.uint64(7)) % np.uint64(p)).astype(np.int64)


def rows(k):
    """(n, 2) int64 tensor / uint64 array -> list of (w0, w1)"""
    if isinstance(k, torch.Tensor):
        assert k.dim() == 2 and k.shape[1] == 2, tuple(k.shape)
        k = k.contiguous().numpy().view(np.uint64)
    assert k.ndim == 2 and k.shape[1] == 2, k.shape
    return [tuple(r) for r in k.tolist()]


class DictTable:
    """the local table of a rank: {(w0, w1): value}; the members ShardedTable calls"""

    def __init__(self):
        self.d = {}
        self._feed = None

    def insert(self, k, v):
        new = 0
        for key, val in zip(rows(k), v.numpy().view(np.uint32).tolist()):
            if key not in self.d:
                self.d[key] = val
                new += 1
        return new

    def insert_reduce_plus(self, k, v=None):
        new = 0
        vv = v.numpy().view(np.uint32).tolist() if v is not None else None
        for i, key in enumerate(rows(k)):
            if key not in self.d:
                self.d[key] = 0
                new += 1
            self.d[key] = (self.d[key] + (vv[i] if vv is not None else 1)) & 0xFFFFFFFF
        return new

    def insert_begin(self, n_total, reduce_plus=False, repeatable=False):
        assert self._feed is None, "streamed insert already open"
        self._feed, self._total, self._plus = [], n_total, reduce_plus

    def insert_feed(self, k, v=None):
        assert k.dim() == 2 and k.shape[1] == 2, tuple(k.shape)
        self._feed.append((k.clone(), v.clone() if v is not None else None))

    def insert_abort(self):
        self._feed = None

    def insert_end(self):
        feed, self._feed = self._feed, None
        k = torch.cat([a for a, _ in feed]) if feed else torch.empty((0, 2), dtype=torch.int64)
        assert k.shape[0] == self._total, (k.shape, self._total)
        if self._plus:
            return self.insert_reduce_plus(k)
        return self.insert(k, torch.cat([b for _, b in feed]) if feed else torch.empty(0, dtype=torch.int32))

    def count(self, k):
        return torch.tensor([1 if key in self.d else 0 for key in rows(k)], dtype=torch.uint8)

    def find_values(self, k):
        r = rows(k)
        v = np.array([self.d.get(key, 0) for key in r], dtype=np.uint32)
        return torch.from_numpy(v.view(np.int32)), torch.tensor([1 if key in self.d else 0 for key in r], dtype=torch.uint8)

    def erase(self, k):
        ne = 0
        for key in rows(k):
            if self.d.pop(key, None) is not None:
                ne += 1
        return ne

    def size(self):
        return len(self.d)


class WideDictBackend:
    key_words = 2

    def __init__(self):
        self.torch_device = torch.device("cpu")
        self.table = DictTable()

    def shard(self, keys, vals, p):
        assert keys.dim() == 2 and keys.shape[1] == 2, tuple(keys.shape)
        k = keys.contiguous().numpy().view(np.uint64)
        r = rank_of(k, p)
        order = np.argsort(r, kind="stable")
        counts = np.bincount(r, minlength=p).tolist()
        ok = torch.from_numpy(k[order].view(np.int64).copy())
        ov = torch.from_numpy(vals.numpy()[order].copy()) if vals is not None else None
        return ok, ov, counts

    def shard_counts(self, keys, p):
        return self.shard(keys, None, p)[2]

    def empty(self, n, dtype):
        return torch.empty(n, dtype=dtype)


def _batches(world, n=6000, universe=4000):
    """every rank's batch: n draws (with repeats) from one universe of wide keys; many keys share w0 or w1 with another key"""
    rng = np.random.RandomState(4242)
    u = rng.randint(0, 1 << 62, size=(universe, 2)).astype(np.uint64)
    u[1::4, 0] = u[0::4, 0]          # same w0, different w1
    u[2::4, 1] = u[0::4, 1]          # same w1, different w0
    assert len(set(rows(u))) == universe
    out = []
    for r in range(world):
        idx = np.random.RandomState(100 + r).randint(0, universe, size=n)
        out.append((u[idx].copy(), (np.arange(n, dtype=np.uint32) + np.uint32(r * 1_000_000))))
    return u, out


def _model(batches, world, rank, chunks, plus=False, into=None):
    """the owner rank's table after ONE sharded insert: piece, then source rank, then position"""
    d = {} if into is None else into
    for i in range(chunks):
        for r in range(world):
            k, v = batches[r]
            n = len(k)
            a, b = n * i // chunks, n * (i + 1) // chunks
            kk, vv = k[a:b], v[a:b]
            m = rank_of(kk, world) == rank if len(kk) else np.zeros(0, dtype=bool)
            for key, val in zip(rows(kk[m]), vv[m].tolist()):
                if plus:
                    d[key] = (d.get(key, 0) + 1) & 0xFFFFFFFF
                else:
                    d.setdefault(key, val)
    return d


def _sum(x):
    t = torch.tensor([int(x)], dtype=torch.int64)
    dist.all_reduce(t)
    return int(t.item())


def _worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kmerhash_amd.dist import ShardedTable, ShardPeerError
        universe, batches = _batches(world)
        keys, vals = batches[rank]
        n = len(keys)
        tk = torch.from_numpy(keys.view(np.int64).copy())
        tv = torch.from_numpy(vals.view(np.int32).copy())
        distinct = len(set(k for b in batches for k in rows(b[0])))

        # ---- one-piece insert: return values, size, contents, first-wins across ranks
        st = ShardedTable(WideDictBackend())
        new = st.insert(tk, tv)
        assert st.collectives == {"counts": 1, "payload": 1, "votes": 3}, st.collectives
        assert _sum(new) == distinct
        assert st.local.d == _model(batches, world, rank, 1)
        assert st.size() == distinct

        # ---- queries: (permuted keys (n, 2), values, flags), aligned
        miss = np.random.RandomState(900 + rank).randint(0, 1 << 62, size=(1500, 2)).astype(np.uint64)
        miss[::3, 0] = keys[:500, 0]                     # half-matching misses: w0 of a stored key, another w1
        qk = np.concatenate([keys[:1500], miss])
        tq = torch.from_numpy(qk.view(np.int64).copy())
        first = {}
        for r in range(world):
            for key, v in zip(rows(batches[r][0]), batches[r][1].tolist()):
                first.setdefault(key, v)
        c0 = dict(st.collectives)
        pk, cnt = st.count(tq)
        assert st.collectives == {"counts": c0["counts"] + 1, "payload": c0["payload"] + 2, "votes": c0["votes"] + 1}, st.collectives
        assert tuple(pk.shape) == (len(qk), 2) and pk.dtype == tq.dtype and tuple(cnt.shape) == (len(qk),)
        pr = rows(pk)
        assert sorted(pr) == sorted(rows(qk))                                        # a permutation of the query ROWS
        owner = rank_of(pk.numpy().view(np.uint64), world)
        assert np.all(np.diff(owner) >= 0)                                           # grouped by owner rank
        exp = np.array([1 if key in first else 0 for key in pr], dtype=np.uint8)
        assert 0 < exp.sum() < len(exp)
        assert np.array_equal(cnt.numpy(), exp)
        pk2, fv, ff = st.find(tq)
        assert tuple(pk2.shape) == (len(qk), 2) and rows(pk2) == pr
        assert np.array_equal(ff.numpy(), exp)
        got = fv.numpy().view(np.uint32)
        assert all(got[i] == first[pr[i]] for i in np.nonzero(exp)[0])
        assert not got[exp == 0].any()

        # ---- three pieces: all counts in ONE exchange, one payload exchange per piece; piece-major first-wins
        chunks = 3
        sp = ShardedTable(WideDictBackend())
        new = sp.insert(tk, tv, chunks=chunks)
        assert sp.collectives == {"counts": 1, "payload": chunks, "votes": 3}, sp.collectives
        assert _sum(new) == distinct
        mp_ = _model(batches, world, rank, chunks)
        assert sp.local.d == mp_
        assert mp_ != _model(batches, world, rank, 1) or world == 1, "the batches do not tell piece-major from rank-major order"

        # ---- a rank with an empty batch (insert and find)
        se = ShardedTable(WideDictBackend())
        eb = [(b[0][:0], b[1][:0]) if r == 0 else b for r, b in enumerate(batches)]
        ek, ev = (tk[:0], tv[:0]) if rank == 0 else (tk, tv)
        new = se.insert(ek, ev, chunks=2)
        assert se.local.d == _model(eb, world, rank, 2)
        assert _sum(new) == se.size() == len(set(k for b in eb for k in rows(b[0])))
        pke, fve, ffe = se.find(tq[:0] if rank == 0 else tq)
        assert tuple(pke.shape) == ((0, 2) if rank == 0 else (len(qk), 2)) and ffe.shape[0] == fve.shape[0] == pke.shape[0]
        if rank != 0:
            held = set(k for b in eb for k in rows(b[0]))
            assert np.array_equal(ffe.numpy(), np.array([1 if key in held else 0 for key in rows(pke)], dtype=np.uint8))

        # ---- counting insert: duplicates inside a rank, across ranks and across pieces
        sc = ShardedTable(WideDictBackend())
        new = sc.insert_counts(tk, chunks=3)
        assert _sum(new) == distinct
        new2 = sc.insert_counts(tk[:2000], chunks=3)
        assert _sum(new2) == 0
        mc = _model(batches, world, rank, 3, plus=True)
        mc = _model([(b[0][:2000], b[1][:2000]) for b in batches], world, rank, 3, plus=True, into=mc)
        assert sc.local.d == mc
        assert _sum(sum(sc.local.d.values())) == world * (n + 2000)

        # ---- erase
        ne = st.erase(tk[:1000])
        gone = set(k for b in batches for k in rows(b[0][:1000]))
        assert _sum(ne) == len(gone)
        assert st.size() == distinct - len(gone)
        assert all(key not in st.local.d for key in gone)

        # ---- one injected failure in insert and in find: every rank raises, nobody hangs, the tables stay usable
        bad = world - 1
        for op, stage in (("insert", 3), ("find", 2)):
            sf = ShardedTable(WideDictBackend())
            if op == "find":
                sf.insert(tk, tv, chunks=2)
            if rank == bad:
                sf._fail_stage = stage
            try:
                if op == "insert":
                    sf.insert(tk, tv, chunks=3)
                else:
                    sf.find(tq)
                raised = None
            except MemoryError:
                raised = "own"
            except ShardPeerError:
                raised = "peer"
            assert raised == ("own" if rank == bad else "peer"), (op, stage, rank, raised)
            if op == "insert":
                assert sf.local_size() == 0 and sf.local._feed is None          # nothing inserted, no streamed insert left open
                sf.insert(tk, tv, chunks=3)
                assert sf.local.d == mp_
            else:
                _, fv2, ff2 = sf.find(tq)
                assert np.array_equal(ff2.numpy(), exp)
            assert sf.size() == distinct
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_table_wide_keys_gloo(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(30)
    assert all(r[1] == "ok" for r in res), res
