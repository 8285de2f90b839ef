"""GPU: the sharded table over 16-byte keys with every RCCL call executed on the one GPU of the test box -- a process group of ONE rank
over "nccl" (= RCCL) with KH_DIST_FORCE_COLLECTIVES=1, as tests/test_gpu_dist_nccl.py does for 64-bit keys.  ShardedTable over
WideGpuBackend (kh_wide_shard_permute, the streamed wide insert, (n, 2) key buffers through the grouped exchanges) must give what a
plain hashmap_robinhood_doubling_wide gives; ShardedKmerCounter(k=63) what KmerCounter(k=63) gives."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _same_items(a, b):
    x, y = a.sorted_items(), b.sorted_items()
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def _worker(port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["KH_DIST_FORCE_COLLECTIVES"] = "1"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        import kmerhash_amd as kh
        from kmerhash_amd import dist as khd
        from kmerhash_amd import kmers as KM
        assert khd.FORCE_COLLECTIVES
        rng = np.random.default_rng(5)
        n = 4_500_000
        keys = rng.integers(0, 1 << 63, (n, 2), dtype=np.uint64)
        keys[1::2, 0] = keys[0::2, 0]                  # pairs of keys that differ in w1 only
        assert len(np.unique(keys[:200_000], axis=0)) == 200_000
        vals = np.arange(n, dtype=np.uint32)
        keys[n - 4000:] = keys[100:4100]               # late duplicates: the first value must win, across pieces
        dk = torch.from_numpy(keys.view(np.int64)).cuda()
        dv = torch.from_numpy(vals.view(np.int32)).cuda()
        st = khd.ShardedTable(khd.WideGpuBackend(0), timing=True)
        assert not st._single() and st.key_words == 2
        plain = kh.hashmap_robinhood_doubling_wide(128, 0.35, 0.8)
        assert st.insert(dk, dv, chunks=4) == plain.insert(dk, dv) == n - 4000
        assert st.collectives == {"counts": 1, "payload": 4, "votes": 3}, st.collectives
        assert {"count_pass", "permute", "exchange", "feed", "build"} <= set(st.timings())
        assert st.size() == plain.size() and st.local.capacity() == plain.capacity()
        assert np.array_equal(st.local.export_info(), plain.export_info())
        assert _same_items(st.local, plain)
        # queries over RCCL: the permuted order of ONE rank is the input order; results are (keys (n, 2), values, flags)
        miss = rng.integers(0, 1 << 63, (300_000, 2), dtype=np.uint64)
        miss[::2, 0] = keys[:150_000, 0]               # misses that share w0 with a stored key
        q1 = np.concatenate([keys[:900_000], miss])
        q1 = q1[rng.permutation(len(q1))]
        dq = torch.from_numpy(q1.view(np.int64)).cuda()
        c0 = dict(st.collectives)
        pk, fv, ff = st.find(dq)
        st.synchronize()
        assert st.collectives == {"counts": c0["counts"] + 1, "payload": c0["payload"] + 2, "votes": c0["votes"] + 1}, st.collectives
        pv, pf = plain.find_values(dq)
        assert tuple(pk.shape) == (len(q1), 2) and torch.equal(pk, dq) and torch.equal(ff, pf) and torch.equal(fv[ff == 1], pv[pf == 1])
        assert int(pf.sum()) == 900_000
        pk2, cnt = st.count(dq)
        st.synchronize()
        assert torch.equal(pk2, dq) and torch.equal(cnt, plain.count(dq)) and torch.equal(cnt, pf)
        assert st.erase(dq) == plain.erase(dq) == 900_000
        assert st.size() == plain.size()
        assert np.array_equal(st.local.export_info(), plain.export_info()) and _same_items(st.local, plain)
        # counting insert through the same path
        sc = khd.ShardedTable(khd.WideGpuBackend(0, hash="farm"))
        pc = kh.hashmap_robinhood_doubling_wide(128, 0.35, 0.8, hash="farm")
        assert sc.insert_counts(dk, chunks=3) == pc.insert_reduce_plus(dk)
        assert sc.insert_counts(dk[:1_000_000], chunks=2) == pc.insert_reduce_plus(dk[:1_000_000]) == 0
        assert np.array_equal(sc.local.export_info(), pc.export_info()) and _same_items(sc.local, pc)
        # one injected local failure per operation: raised, nothing left half-open, the table usable afterwards
        for op, stage in (("insert", 3), ("find", 2), ("count", 1), ("erase", 4)):
            st._fail_stage = stage
            with pytest.raises(MemoryError):
                if op == "insert":
                    st.insert(dk[:200_000], dv[:200_000], chunks=2)
                elif op == "find":
                    st.find(dq)
                    st.synchronize()
                elif op == "count":
                    st.count(dq)
                    st.synchronize()
                else:
                    st.erase(dq[:1000])
            assert st.size() == plain.size()
        assert st.insert(dk[:200_000], dv[:200_000], chunks=2) == plain.insert(dk[:200_000], dv[:200_000])
        assert np.array_equal(st.local.export_info(), plain.export_info()) and _same_items(st.local, plain)
        # the distributed k-mer counter at k = 63 against the single-GPU counter on the same text
        text = KM.synthetic_fastq(4000, read_len=150, genome_len=200_000, seed=3)
        kc = KM.ShardedKmerCounter(khd.ShardedTable(khd.WideGpuBackend(0, hash="farm")), k=63, chunks=3)
        one = KM.KmerCounter(k=63, hash="farm")
        half = text.index(b"\n@r2000\n") + 1
        dtext = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in (text[:half], text[half:])]
        nk = sum(kc.add_fastq(t) for t in dtext)
        assert nk == one.add_fastq(text) > 0
        assert kc.size() == one.table.size()
        assert _same_items(kc.st.local, one.table)
        with pytest.raises(ValueError):
            KM.ShardedKmerCounter(khd.ShardedTable(khd.WideGpuBackend(0)), k=31)
        with pytest.raises(ValueError):
            KM.ShardedKmerCounter(khd.ShardedTable(khd.GpuBackend(0)), k=63)
        q.put("ok")
    except Exception:  # pragma: no cover
        import traceback
        q.put("FAIL: " + traceback.format_exc())
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_sharded_wide_table_over_rccl_one_rank_forced_collectives():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    res = q.get(timeout=500)
    p.join(60)
    assert res == "ok", res
