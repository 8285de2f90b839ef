"""CPU, gloo world 2, k = 63: ShardedKmerCounter sizes the local tables of a WIDE counter from a HyperLogLog estimate -- every rank
feeds the estimator its 16-byte k-mers through hll.update_wide, the registers are merged by an all-reduce(max), every rank reserves
its share of the global estimate before it inserts (hyperloglog64.hpp:477-489; robinhood_offset_hashmap_ptr.hpp:2512-2535).  The
device pieces are replaced: the backend is the 16-byte-key dict backend of tests/test_dist_gloo_wide.py, the k-mers are a Python-int
statement of the 128-bit definition, the estimator is the oracle HLL fed the CPU hashes of the 16-byte keys.  The code under test is
kmerhash_amd.kmers.ShardedKmerCounter over kmerhash_amd.dist.ShardedTable."""
import os
import socket
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

K, READ_LEN, N_READS, MAX_LOAD = 63, 100, 600, 0.8
CODE = {ord(c): i for i, c in enumerate("ACGT")}
M64 = (1 << 64) - 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def py_kmers128_fastq(text, k):
    """canonical 128-bit k-mers of the sequence lines of FASTQ text, in order -> (n, 2) uint64 {w0 = V mod 2^64, w1 = V >> 64}: V has the
    first base most significant, A0 C1 G2 T3; any other byte ends a run; canonical = min(V, revcomp_k(V)) as integers"""
    mask = (1 << (2 * k)) - 1
    out = []
    for line in bytes(text).split(b"\n")[1::4]:
        fw = rc = run = 0
        for b in line:
            c = CODE.get(b)
            if c is None:
                fw = rc = run = 0
                continue
            fw = ((fw << 2) | c) & mask
            rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)))
            run += 1
            if run >= k:
                v = min(fw, rc)
                out.append((v & M64, v >> 64))
    return np.array(out, dtype=np.uint64).reshape(-1, 2)


def notional_capacity(n):
    """the capacity a doubling table needs to hold n elements at MAX_LOAD, starting from 128"""
    cap = 128
    while cap * MAX_LOAD < n:
        cap *= 2
    return cap


def _worker(rank, world, port, q):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import oracle_py as O
        from kmerhash_amd import hll as HL
        from kmerhash_amd import kmers as KM
        from kmerhash_amd.dist import ShardedTable
        from test_dist_gloo_wide import WideDictBackend, rank_of, rows
        fq = KM.synthetic_fastq(N_READS * world, READ_LEN, 9_000, seed=11, n_rate=0.002)      # one file; every rank takes its share of the reads
        recs = fq.split(b"\n")
        per = 4 * N_READS
        mine = b"\n".join(recs[rank * per:(rank + 1) * per]) + b"\n"
        kmer_fn = lambda text: torch.from_numpy(py_kmers128_fastq(text, K).view(np.int64).copy())

        class Hll:
            """stands in for the GPU estimator: update_wide = the oracle HLL over the CPU hashes of the 16-byte keys"""
            precision = 12
            est_error_rate = 1.04 / 64.0

            def __init__(s):
                s.o = O.OracleHLL(12, 0, O.HASH_FARM, 43)
                s.fed = 0

            def update_wide(s, km):
                assert km.dim() == 2 and km.shape[1] == 2, tuple(km.shape)
                s.o.update_via_hashval(O.hash16_batch(O.HASH_FARM, 43, km.numpy().view(np.uint64)))
                s.fed += km.shape[0]

            def update(s, km):
                raise AssertionError("a wide counter must feed its estimator through update_wide")

            def registers(s):
                return s.o.registers()

        be = WideDictBackend()
        reserved = []                                          # (elements reserved for, local size at that moment)
        be.table.reserve = lambda n: reserved.append((int(n), be.table.size()))
        hl = Hll()
        kc = KM.ShardedKmerCounter(ShardedTable(be), K, True, kmer_fn=kmer_fn, chunks=2, reserve_from_estimate=True, hll=hl)
        myk = py_kmers128_fastq(mine, K)
        assert kc.add_fastq(mine) == len(myk) == hl.fed > N_READS * (READ_LEN - K + 1) // 2

        # the merged registers are those of ONE estimator fed every rank's k-mers; all ranks computed the same global estimate
        allmine = [None] * world
        dist.all_gather_object(allmine, myk)
        one = O.OracleHLL(12, 0, O.HASH_FARM, 43)
        for a in allmine:
            one.update_via_hashval(O.hash16_batch(O.HASH_FARM, 43, a))
        g_est = HL.estimate_global(hl)
        assert g_est == one.estimate() == HL.estimate_from_registers(one.registers(), 12)
        ests = [None] * world
        dist.all_gather_object(ests, g_est)
        assert ests == [g_est] * world
        allk = np.concatenate(allmine)
        uk, cnt = np.unique(allk, axis=0, return_counts=True)
        assert abs(g_est - len(uk)) < 0.08 * len(uk)
        # reserved its share -- before anything was inserted -- for at least estimate / world elements: a capacity of that / max_load
        assert len(reserved) == 1 and reserved[0][1] == 0, reserved
        assert reserved[0][0] == int(g_est / world * (1.0 + hl.est_error_rate))
        assert notional_capacity(reserved[0][0]) >= g_est / world / MAX_LOAD

        # the counts: every k-mer of the whole file on its owner rank
        owner = rank_of(uk, world)
        exp = {key: int(c) for key, c in zip(rows(uk[owner == rank]), cnt[owner == rank].tolist())}
        assert be.table.d == exp
        assert kc.size() == len(uk) and kc.total_kmers == len(myk)
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_wide_kmer_counter_reserves_from_estimate_gloo(oracle):
    world = 2
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
