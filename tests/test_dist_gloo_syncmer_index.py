"""CPU: the sharded position index over closed syncmers on two ranks over gloo, with the test-local CPU backend of
tests/test_dist_gloo_index.py (IndexModel as the local index, the oracle hash for shard, np_csr_unpermute) and np_syncmers as text_pairs:
the sampled pairs of two texts with different pos_base land on the rank the dist hash names and find / find_sequences answer in QUERY
order.  The exchange logic under test is the code the GPU ranks run; the device parts (the syncmer kernels behind
IndexGpuBackend(s=...)) are covered by tests/test_gpu_dist_syncmer_index.py."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dist_gloo_index import ModelBackend, _free_port, collect, make_text  # noqa: E402

K, S = 15, 11


class SyncmerBackend(ModelBackend):
    """ModelBackend whose text_pairs samples closed syncmers, as IndexGpuBackend(s=...) does on the device"""

    def __init__(self, O):
        super().__init__(O, None)
        from syncmer_model import np_syncmers
        self.syncmers = np_syncmers

    def pairs_np(self, text):
        return self.syncmers(np.asarray(text, dtype=np.uint8), K, S, True, "murmur", 42)


def _run(rank, world, O):
    from index_model import IndexModel
    from kmerhash_amd.dist_index import ShardedKmerPositionIndex
    be = SyncmerBackend(O)
    st = ShardedKmerPositionIndex(be)
    assert st.p == world == 2
    text, base = make_text(rank), (rank + 1) << 20
    km, pos = be.pairs_np(text)
    all_windows = ModelBackend(O, None).pairs_np(text)[0]
    assert 0.3 * len(all_windows) < len(km) < 0.5 * len(all_windows)      # about 2 / (k - s + 1) = 0.4 of the windows
    c0 = dict(st.collectives)
    assert st.append_sequences(text, pos_base=base) == len(km)
    assert {n: v - c0[n] for n, v in st.collectives.items()} == {"counts": 1, "payload": 1, "votes": 3, "reduce": 0}
    allk, allp = [None] * world, [None] * world
    dist.all_gather_object(allk, km)
    dist.all_gather_object(allp, pos + np.uint32(base))
    gk, gp = np.concatenate(allk), np.concatenate(allp)
    model = IndexModel(gk, gp)
    assert sorted(np.unique(gp >> np.uint32(20)).tolist()) == [1, 2]      # both coordinate spaces are in the index
    # every pair on the rank the dist hash names, nothing lost, nothing twice
    lk, lp = be.index.k, be.index.p
    assert (be.owner(lk, world) == rank).all()
    m = be.owner(gk, world) == rank
    a, b = np.lexsort((lp, lk)), np.lexsort((gp[m], gk[m]))
    assert np.array_equal(lk[a], gk[m][b]) and np.array_equal(lp[a], gp[m][b]) and 0 < m.sum() < len(gk)
    assert (st.size(), st.total()) == (model.size(), model.total())
    # find in query order: own and the other rank's k-mers, misses, repeats
    rng = np.random.default_rng(5 + rank)
    hits = gk[rng.integers(0, len(gk), 500)]
    q = np.concatenate([hits, rng.integers(0, 1 << 30, 200).astype(np.uint64), hits[:50]])
    q = q[rng.permutation(len(q))]
    offs, fpos = st.find(torch.from_numpy(q.view(np.int64).copy()))
    eo, ep = model.find(q)
    assert np.array_equal(offs.numpy().astype(np.uint64), eo) and np.array_equal(fpos.numpy().view(np.uint32), ep) and int(eo[-1]) >= 550
    # find_sequences: the other rank's shared block and a stretch of this rank's text, sampled with the same rule
    qt = np.concatenate([make_text(1 - rank)[2500:6500], [10], text[15_000:15_600]]).astype(np.uint8)
    qk, qp = be.pairs_np(qt)
    qpos, offs, fpos = st.find_sequences(qt)
    eo, ep = model.find(qk)
    assert np.array_equal(qpos.numpy().view(np.uint32), qp) and len(qp) > 1000
    assert np.array_equal(offs.numpy().astype(np.uint64), eo) and np.array_equal(fpos.numpy().view(np.uint32), ep)
    # selection is a function of the k-mer: every sampled query k-mer cut from an indexed text is found, at its own place among others
    own = qp >= 4001
    want = (qp[own].astype(np.int64) - 4001) + 15_000 + base
    for i, wpos in zip(np.nonzero(own)[0], want):
        assert wpos in fpos.numpy().view(np.uint32)[int(eo[i]): int(eo[i + 1])]
    assert own.sum() > 150


def _worker(rank, world, port, q):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import oracle_py as O
        _run(rank, world, O)
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_syncmer_index_gloo(oracle):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = collect(procs, q, 240)
    assert len(res) == 2 and all(r[1] == "ok" for r in res), res
