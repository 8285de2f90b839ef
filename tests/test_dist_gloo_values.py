"""CPU: the value-range members of kmerhash_amd.dist.ShardedTable and kmerhash_amd.kmers.ShardedKmerCounter on world size 2 and 3 over
gloo.  The backends live in this file, one per key width (key_words 1: a batch of keys is a 1-D tensor; key_words 2: rows of an (n, 2)
tensor): the local table is a Python dict with value_histogram / erase_values computed from the dict, shard() a stable argsort by a
fixed rank function.  ShardedTable.value_histogram must be the histogram of the UNION of the ranks' tables on every rank (one
all-reduce), erase_values purely local; ShardedKmerCounter.spectrum / drop_below likewise, including a rank whose local table is
empty (no key of the universe maps to it)."""
import os
import socket
from collections import Counter

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


def as_rows(k, words):
    """keys (1-D for words = 1, (n, 2) for words = 2; int64 tensor or uint64 array) -> list of hashable keys"""
    if isinstance(k, torch.Tensor):
        k = k.contiguous().numpy().view(np.uint64)
    if words == 1:
        assert k.ndim == 1, k.shape
        return k.tolist()
    assert k.ndim == 2 and k.shape[1] == 2, k.shape
    return [tuple(r) for r in k.tolist()]


def rank_of(k, p, words):
    w0 = k if words == 1 else k[:, 0]
    w1 = np.zeros_like(w0) if words == 1 else k[:, 1]
    h = (w0 * np.uint64(0x9E3779B97F4A7C15)) ^ (w1 * np.uint64(0xC2B2AE3D27D4EB4F) + (w1 >> np.uint64(29)))
    h ^= h >> np.uint64(31)
    return ((h >> np.uint64(7)) % np.uint64(p)).astype(np.int64)


def histogram_of(values, nbins):
    """the contract of kh_value_histogram on a list of values"""
    v = np.minimum(np.asarray(list(values), dtype=np.int64), nbins - 1)
    return np.bincount(v, minlength=nbins).astype(np.uint64)


class DictTable:
    """local table of a rank: {key: value}; the members ShardedTable / ShardedKmerCounter call"""

    def __init__(self, words):
        self.words = words
        self.d = {}
        self._feed = None

    def insert_reduce_plus(self, k, v=None):
        new = 0
        vv = v.numpy().view(np.uint32).tolist() if v is not None else None
        for i, key in enumerate(as_rows(k, self.words)):
            if key not in self.d:
                self.d[key] = 0
                new += 1
            self.d[key] = (self.d[key] + (vv[i] if vv is not None else 1)) & 0xFFFFFFFF
        return new

    def insert(self, k, v):
        new = 0
        for key, val in zip(as_rows(k, self.words), v.numpy().view(np.uint32).tolist()):
            if key not in self.d:
                self.d[key] = val
                new += 1
        return new

    def insert_begin(self, n_total, reduce_plus=False, repeatable=False):
        assert self._feed is None
        self._feed, self._total, self._plus = [], n_total, reduce_plus

    def insert_feed(self, k, v=None):
        self._feed.append((k.clone(), v.clone() if v is not None else None))

    def insert_abort(self):
        self._feed = None

    def insert_end(self):
        feed, self._feed = self._feed, None
        new = 0
        for k, v in feed:
            new += self.insert_reduce_plus(k, v) if self._plus else self.insert(k, v)
        return new

    def size(self):
        return len(self.d)

    def value_histogram(self, nbins=256):
        return histogram_of(self.d.values(), nbins)

    def erase_values(self, lo, hi):
        gone = [key for key, v in self.d.items() if lo <= v <= hi]
        for key in gone:
            del self.d[key]
        return len(gone)


class DictBackend:
    def __init__(self, words):
        self.key_words = words
        self.torch_device = torch.device("cpu")
        self.table = DictTable(words)

    def shard(self, keys, vals, p):
        k = keys.contiguous().numpy().view(np.uint64)
        r = rank_of(k, p, self.key_words)
        order = np.argsort(r, kind="stable")
        counts = np.bincount(r, minlength=p).tolist()
        ok = torch.from_numpy(k[order].view(np.int64).copy())
        ov = torch.from_numpy(vals.numpy()[order].copy()) if vals is not None else None
        return ok, ov, counts

    def shard_counts(self, keys, p):
        return self.shard(keys, None, p)[2]

    def empty(self, n, dtype):
        return torch.empty(n, dtype=dtype)


def _universe(world, words, leave_last_rank_empty):
    rng = np.random.RandomState(77 + words)
    u = rng.randint(1, 1 << 62, size=(1500,) if words == 1 else (1500, 2)).astype(np.uint64)
    if words == 2:
        u[1::4, 0] = u[0::4, 0]            # same w0, different w1
    if leave_last_rank_empty:
        u = u[rank_of(u, world, words) != world - 1]
    assert len(set(as_rows(u, words))) == len(u) > 300
    return u


def _draws(u, rank, n=3000):
    """a rank's batch: n draws with repeats, a few keys drawn very often (counts past the small histograms' last bin)"""
    rs = np.random.RandomState(500 + rank)
    idx = rs.randint(0, len(u), size=n)
    idx[: n // 6] = rs.randint(0, 5, size=n // 6)
    return u[idx].copy()


def _worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kmerhash_amd.dist import ShardedTable
        from kmerhash_amd.kmers import ShardedKmerCounter
        for words in (1, 2):
            # ---- ShardedTable: histogram of the union on every rank, local erase
            u = _universe(world, words, False)
            batches = [_draws(u, r) for r in range(world)]
            union = Counter(k for b in batches for k in as_rows(b, words))
            st = ShardedTable(DictBackend(words))
            st.insert_counts(torch.from_numpy(batches[rank].view(np.int64).copy()), chunks=2)
            assert st.size() == len(union)
            assert max(union.values()) > 64 and min(union.values()) == 1
            for nbins in (1, 8, 64, 1024):
                h = st.value_histogram(nbins)
                assert isinstance(h, np.ndarray) and h.dtype == np.uint64 and h.shape == (nbins,)
                assert np.array_equal(h, histogram_of(union.values(), nbins)), (words, nbins)
                assert int(h.sum()) == len(union)
            mine = {k: c for k, c in union.items() if rank_of(np.array([k], dtype=np.uint64).reshape((1,) if words == 1 else (1, 2)), world, words)[0] == rank}
            assert st.local.d == mine
            c0 = dict(st.collectives)
            ne = st.erase_values(2, 5)
            assert st.collectives == c0                                                  # no exchange
            assert ne == sum(1 for c in mine.values() if 2 <= c <= 5) > 0
            left = {k: c for k, c in union.items() if not 2 <= c <= 5}
            assert st.size() == len(left)
            assert np.array_equal(st.value_histogram(16), histogram_of(left.values(), 16))
            assert st.erase_values(2, 5) == 0 and st.erase_values(9, 3) == 0 and st.size() == len(left)

            # ---- ShardedKmerCounter: spectrum / drop_below; the last rank owns no key of this universe
            u = _universe(world, words, True)
            batches = [_draws(u, r) for r in range(world)]
            union = Counter(k for b in batches for k in as_rows(b, words))
            sk = ShardedTable(DictBackend(words))
            kc = ShardedKmerCounter(sk, k=31 if words == 1 else 63, kmer_fn=lambda km: km, chunks=2)
            b = torch.from_numpy(batches[rank].view(np.int64).copy())
            half = len(b) // 2
            kc.add_fastq(b[:half])
            kc.add_fastq(b[half:])
            assert (sk.local_size() == 0) == (rank == world - 1)
            for nbins in (4, 256):
                assert np.array_equal(kc.spectrum(nbins), histogram_of(union.values(), nbins)), (words, nbins)
            assert kc.spectrum(256)[0] == 0
            assert kc.drop_below(0) == 0 and kc.drop_below(-3) == 0 and kc.size() == len(union)
            exp_local = sum(1 for c in sk.local.d.values() if c < 3)
            dropped = kc.drop_below(3)
            assert dropped == exp_local and not any(c < 3 for c in sk.local.d.values())
            kept = {k_: c for k_, c in union.items() if c >= 3}
            assert kc.size() == len(kept) and 0 < len(kept) < len(union)
            t = torch.tensor([dropped], dtype=torch.int64)
            dist.all_reduce(t)
            assert int(t.item()) == len(union) - len(kept)
            if rank == world - 1:
                assert dropped == 0
            assert np.array_equal(kc.spectrum(32), histogram_of(kept.values(), 32))
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_value_histogram_and_erase_values_gloo(world):
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
