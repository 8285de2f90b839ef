"""GPU: the stranded sharded position index, one rank over RCCL with KH_DIST_FORCE_COLLECTIVES=1 (every exchange runs through RCCL once,
as in tests/test_gpu_dist_syncmer_index.py): IndexGpuBackend(s=11, stranded=True) and WideIndexGpuBackend(k=63, s=31, stranded=True) stamp
this rank's pairs with its pos_base before the exchange -- the local export equals the single-GPU stranded index fed the same texts, the
sharded find returns the stamped values of the model, and a coordinate beyond 2^31 is refused."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.multiprocessing as mp  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dist_gloo_index import collect  # noqa: E402
from test_gpu_dist_index import _free_port, make_text  # noqa: E402


def _rccl_worker(port, q, wide):
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
        from index_model import IndexModel
        from wide_index_model import WideIndexModel
        from strand_model import np_stamp
        from syncmer_model import np_syncmers
        import kmerhash_amd as kh
        k, s = (63, 31) if wide else (15, 11)
        be = kh.WideIndexGpuBackend(0, k=k, s=s, stranded=True) if wide else kh.IndexGpuBackend(0, k=k, s=s, stranded=True)
        assert be.stranded and be.index.stranded and (be.index.s, be.index.w) == (s, None)
        st = kh.ShardedKmerPositionIndex(be)
        assert not st._single()
        text = make_text(0, 8000, 200)
        parts = ((text[:3500], 77), (text[3500:], 1_000_000))
        single = (kh.WideKmerPositionIndex if wide else kh.KmerPositionIndex)(k=k, s=s, stranded=True)
        km, pos = [], []
        for part, base in parts:
            pk, pp = np_syncmers(part, k, s, True, "murmur", 42, wide)
            c0 = dict(st.collectives)
            assert st.append_sequences(part, pos_base=base) == len(pk) > (40 if wide else 500)
            assert {n: v - c0[n] for n, v in st.collectives.items()} == {"counts": 1, "payload": 1, "votes": 3, "reduce": 0}, st.collectives
            km.append(pk); pos.append(np_stamp(part, pp, k, base))
            single.append_sequences(part, pos_base=base)
        km, pos = np.concatenate(km), np.concatenate(pos)
        assert (pos & 1).any() and not (pos & 1).all()
        # the local export is the single-GPU stranded index's, byte for byte, and the model's
        assert all(a.tobytes() == b.tobytes() for a, b in zip(st.local.export(), single.export()))
        model = (WideIndexModel if wide else IndexModel)(km, pos)
        keys, offs, got = st.local.export()
        eo, ep = model.export_in_key_order(keys)
        assert np.array_equal(offs, eo) and np.array_equal(got, ep)
        # the sharded find returns stamped values; the query's own offsets stay plain
        qt = np.concatenate([text[1000:2000], [ord("N")], text[5000:5600]]).astype(np.uint8)
        qk, qp = np_syncmers(qt, k, s, True, "murmur", 42, wide)
        qpos, foffs, fpos = st.find_sequences(qt)
        mo, mp_ = model.find(qk)
        assert np.array_equal(qpos.cpu().numpy().view(np.uint32), qp)
        assert np.array_equal(foffs.cpu().numpy().astype(np.uint64), mo) and np.array_equal(fpos.cpu().numpy().view(np.uint32), mp_)
        assert int(mo[-1]) > (10 if wide else 100)
        # a stamped coordinate has 31 bits: refused on every rank, nothing appended
        total = st.total()
        try:
            st.append_sequences(text[:100], pos_base=2 ** 31 - 50)
            raise AssertionError("pos_base + len(text) > 2^31 was accepted")
        except ValueError as e:
            assert "2^31" in str(e)
        assert st.total() == total
        single.close()
        st.local.close()
        q.put("ok")
    except Exception:  # pragma: no cover
        import traceback
        q.put("FAIL: " + traceback.format_exc())
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("wide", [False, True])
def test_one_rank_over_rccl_forced_collectives(wide):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), q, wide))
    p.start()
    res = collect([p], q, 240)
    assert res == ["ok"], res
