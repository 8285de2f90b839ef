"""GPU: the sharded position index on the one GPU of the test box.
(a) two ranks share the GPU over gloo (host-staged exchanges, as tests/test_gpu_dist_rehearsal.py): kh_shard_permute with positions as
    values, the local kh_index_append of what arrived, the multimap query path and kh_csr_unpermute are the code RCCL ranks run; checked
    against ONE IndexModel over the pairs of both ranks, the local exports against a single-GPU index of the owned pairs, byte for byte;
(b) the same with 16-byte k-mers (WideIndexGpuBackend, k = 41) against tests/wide_index_model.py;
(c) one rank over RCCL with KH_DIST_FORCE_COLLECTIVES=1, so that every new exchange has run through RCCL once;
(d) a plain KmerPositionIndex launches the kernels it launched before (no k_csr_* kernel)."""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dist_gloo_index import collect  # noqa: E402

K = 15
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def make_text(rank, n, poly_a):
    """n bases of this rank: random, a few Ns, one poly-A stretch and one 2 000-base block every rank holds"""
    rng = np.random.default_rng(2000 + rank)
    t = LUT[rng.integers(0, 4, n)].copy()
    t[1000 + 700 * rank: 3000 + 700 * rank] = LUT[np.random.default_rng(78).integers(0, 4, 2000)]
    a = n // 2 + 300 * rank
    t[a: a + poly_a] = ord("A")
    t[rng.integers(0, n, 6)] = ord("N")
    return t


def dev_keys(k):
    return torch.from_numpy(np.ascontiguousarray(k).view(np.int64).copy()).cuda()


def queries(rng, gk, n_hit, n_miss):
    hits = gk[rng.integers(0, len(gk), n_hit)]
    q = np.concatenate([hits, rng.integers(0, 1 << 30, n_miss).astype(np.uint64), hits[: n_hit // 8], np.zeros(2, dtype=np.uint64)])
    return q[rng.permutation(len(q))]


def _narrow(rank, world, dist):
    from oracle import oracle_py as O
    from index_model import IndexModel, np_kmers_pos
    from minimizer_model import np_minimizers
    import kmerhash_amd as kh
    from kmerhash_amd.dist import DIST_SEED
    from kmerhash_amd.index import SORT_TILE
    owner = lambda k: (O.hash_batch(O.HASH_MURMUR3_X86, DIST_SEED, np.ascontiguousarray(k)) % np.uint64(world)).astype(np.int64)
    text, base = make_text(rank, 60_000, 5000), rank << 20
    assert 5000 > SORT_TILE                                   # the owner of the poly-A key takes the segment-radix path
    for w in (None, 10):
        pairs = (lambda t: np_kmers_pos(t, K, True)) if w is None else (lambda t: np_minimizers(t, K, w, True, "murmur", 42))
        st = kh.ShardedKmerPositionIndex(kh.IndexGpuBackend(0, k=K, w=w))
        km, pos = pairs(text)
        assert st.build_sequences(text, pos_base=base) == len(km)
        assert st.collectives == {"counts": 1, "payload": 1, "votes": 3, "reduce": 0}, st.collectives
        allk, allp = [None] * world, [None] * world
        dist.all_gather_object(allk, km)
        dist.all_gather_object(allp, pos + np.uint32(base))
        gk, gp = np.concatenate(allk), np.concatenate(allp)
        model = IndexModel(gk, gp)
        assert (st.size(), st.total()) == (model.size(), model.total())
        # the local index IS the single-GPU index of the owned pairs built in one batch
        m = owner(gk) == rank
        single = kh.KmerPositionIndex(k=K, w=w)
        single.build(gk[m], gp[m])
        for a, b in zip(st.local.export(), single.export()):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        single.close()
        assert (st.local.size(), st.local.total()) == (len(np.unique(gk[m])), int(m.sum()))
        if owner(np.zeros(1, dtype=np.uint64))[0] == rank:
            assert int(model.count(np.zeros(1, dtype=np.uint64))[0]) > 2 * SORT_TILE
        # count / find / find_sequences in query order
        rng = np.random.default_rng(9 + rank)
        q = queries(rng, gk, 3000, 1000)
        if rank == 1:
            q = q[:0] if w is None else q[:1]
        cnt = st.count(dev_keys(q))
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), model.count(q))
        offs, fpos = st.find(dev_keys(q))
        eo, ep = model.find(q)
        assert np.array_equal(offs.cpu().numpy().astype(np.uint64), eo) and np.array_equal(fpos.cpu().numpy().view(np.uint32), ep)
        qt = np.concatenate([make_text(1 - rank, 60_000, 5000)[500:4500], text[29_500:31_000]])
        qk, qp = pairs(qt)
        qpos, offs, fpos = st.find_sequences(qt)
        eo, ep = model.find(qk)
        assert np.array_equal(qpos.cpu().numpy().view(np.uint32), qp)
        assert np.array_equal(offs.cpu().numpy().astype(np.uint64), eo) and np.array_equal(fpos.cpu().numpy().view(np.uint32), ep)
        # erase and drop_above: the model's global totals
        ek = np.concatenate([allk[rank][:2000], allk[1 - rank][500:1500]])
        alle = [None] * world
        dist.all_gather_object(alle, ek)
        gone = np.isin(gk, np.concatenate(alle))
        assert st.erase(dev_keys(ek)) == (len(np.unique(gk[gone])), int(gone.sum()))
        gk, gp = gk[~gone], gp[~gone]
        uk, ucnt = np.unique(gk, return_counts=True)
        gone = np.isin(gk, uk[ucnt > 50])
        assert st.drop_above(50) == (int((ucnt > 50).sum()), int(gone.sum())) and gone.sum() > 2 * SORT_TILE
        gk, gp = gk[~gone], gp[~gone]
        assert (st.size(), st.total()) == (len(np.unique(gk)), len(gk))
        model = IndexModel(gk, gp)
        offs, fpos = st.find(dev_keys(q))
        eo, ep = model.find(q)
        assert np.array_equal(offs.cpu().numpy().astype(np.uint64), eo) and np.array_equal(fpos.cpu().numpy().view(np.uint32), ep)
        st.local.close()


def _wide(rank, world, dist):
    from wide_index_model import WideIndexModel, kmers128_pos_model
    import kmerhash_amd as kh
    text, base = make_text(rank, 20_000, 300), rank << 20
    km, pos = kmers128_pos_model(text, 41, True)
    pos = pos + np.uint32(base)
    st = kh.ShardedKmerPositionIndex(kh.WideIndexGpuBackend(0, k=41))
    half = len(km) // 2
    for a, b in ((0, half), (half, len(km))):
        assert st.append(dev_keys(km[a:b]), torch.from_numpy(pos[a:b].view(np.int32).copy()).cuda()) == b - a
    allk, allp = [None] * world, [None] * world
    dist.all_gather_object(allk, km)
    dist.all_gather_object(allp, pos)
    gk, gp = np.concatenate(allk), np.concatenate(allp)
    model = WideIndexModel(gk, gp)
    assert (st.size(), st.total()) == (model.size(), model.total())
    # every key whole on one rank: the local CSR is the model's for the keys this rank holds, and no key is on two ranks
    lk, lo, lp = st.local.export()
    here = np.isin(np.array(model._rank(gk)), np.array(model._rank(lk)))
    eo, ep = WideIndexModel(gk[here], gp[here]).export_in_key_order(lk)
    assert np.array_equal(lo, eo) and np.array_equal(lp, ep)
    held = [None] * world
    dist.all_gather_object(held, set(map(tuple, lk.tolist())))
    assert not (held[0] & held[1]) and len(held[0]) + len(held[1]) == model.size() and held[0] and held[1]
    rng = np.random.default_rng(19 + rank)
    q = np.concatenate([gk[rng.integers(0, len(gk), 1500)], rng.integers(0, 1 << 40, (300, 2)).astype(np.uint64), gk[:50]])
    q = q[rng.permutation(len(q))]
    cnt = st.count(dev_keys(q))
    assert np.array_equal(cnt.cpu().numpy().view(np.uint32), model.count(q))
    offs, fpos = st.find(dev_keys(q))
    eo, ep = model.find(q)
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), eo) and np.array_equal(fpos.cpu().numpy().view(np.uint32), ep)
    assert int(eo[-1]) >= 1550
    st.local.close()


def _gloo_worker(rank, world, port, q, part):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        (_narrow if part == "narrow" else _wide)(rank, world, dist)
        q.put((rank, "ok"))
    except Exception:  # pragma: no cover
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("part", ["narrow", "wide"])
def test_two_ranks_share_the_gpu(oracle, part):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q, part)) for r in range(2)]
    for p in procs:
        p.start()
    res = collect(procs, q, 240)
    assert len(res) == 2 and all(r[1] == "ok" for r in res), res


def _rccl_worker(port, q):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["KH_DIST_FORCE_COLLECTIVES"] = "1"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        from index_model import IndexModel, np_kmers_pos
        import kmerhash_amd as kh
        from kmerhash_amd import dist as khd
        assert khd.FORCE_COLLECTIVES
        text = make_text(0, 60_000, 5000)
        km, pos = np_kmers_pos(text, K, True)
        pos = pos + np.uint32(77)
        st = kh.ShardedKmerPositionIndex(kh.IndexGpuBackend(0, k=K), timing=True)
        assert not st._single()
        assert st.build_sequences(text, pos_base=77) == len(km)
        assert st.collectives == {"counts": 1, "payload": 1, "votes": 3, "reduce": 0}, st.collectives
        model = IndexModel(km, pos)
        assert (st.size(), st.total()) == (model.size(), model.total())
        rng = np.random.default_rng(3)
        qk = queries(rng, km, 3000, 1000)
        c0 = dict(st.collectives)
        offs, fpos = st.find(dev_keys(qk))
        assert {k: v - c0[k] for k, v in st.collectives.items()} == {"counts": 2, "payload": 2, "votes": 2, "reduce": 0}
        eo, ep = model.find(qk)
        assert np.array_equal(offs.cpu().numpy().astype(np.uint64), eo) and np.array_equal(fpos.cpu().numpy().view(np.uint32), ep)
        assert np.array_equal(st.count(dev_keys(qk)).cpu().numpy().view(np.uint32), model.count(qk))
        assert {"permute", "exchange", "local_query", "unpermute"} <= set(st.timings())
        gone = np.isin(km, qk)
        assert st.erase(dev_keys(qk)) == (len(np.unique(km[gone])), int(gone.sum()))
        assert (st.size(), st.total()) == (len(np.unique(km[~gone])), int((~gone).sum()))
        st._fail_stage = 3                                   # a local failure is raised and leaves the index usable after clear()
        with pytest.raises(MemoryError):
            st.find(dev_keys(qk))
        st.clear()
        assert st.build_sequences(text) == len(km) and st.total() == len(km)
        q.put("ok")
    except Exception:  # pragma: no cover
        import traceback
        q.put("FAIL: " + traceback.format_exc())
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_one_rank_over_rccl_forced_collectives():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), q))
    p.start()
    res = collect([p], q, 240)
    assert res == ["ok"], res


def test_the_single_gpu_index_launches_what_it_launched_before():
    import kmerhash_amd as kh
    from index_model import np_kmers_pos
    km, pos = np_kmers_pos(make_text(0, 20_000, 300), K, True)
    ix = kh.KmerPositionIndex(k=K)
    try:
        ix.profile_enable(True)
        index_kernels = lambda: {n for n in ix.profile() if n.startswith(("k_index_", "kw_index_", "k_csr_"))}
        ix.build(km[:15_000], pos[:15_000])
        build = {"k_index_rank", "k_index_scan", "k_index_scatter", "k_index_tile_sort", "k_index_seg_radix"}
        assert index_kernels() == build
        ix.find(km[:1000])
        find = build | {"k_index_lookup", "k_index_gather"}
        assert index_kernels() == find
        ix.append(km[15_000:], pos[15_000:])
        assert index_kernels() == find | {"k_index_stamp", "k_index_rank_carry", "k_index_count_pairs", "k_index_move"}
        assert not any("csr" in n for n in ix.profile())
    finally:
        ix.close()
