"""GPU: the sharded position index over closed syncmers, one rank over RCCL with KH_DIST_FORCE_COLLECTIVES=1 (every exchange runs through
RCCL once, as in tests/test_gpu_dist_index.py), both backends with s: append_sequences with pos_base in two batches and find_sequences,
against the numpy model (tests/syncmer_model.py) and the index models over the model's pairs."""
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
        from syncmer_model import np_syncmers
        import kmerhash_amd as kh
        k, s = (40, 20) if wide else (15, 11)
        be = kh.WideIndexGpuBackend(0, k=k, s=s) if wide else kh.IndexGpuBackend(0, k=k, s=s)
        assert (be.index.s, be.index.w) == (s, None)
        st = kh.ShardedKmerPositionIndex(be)
        assert not st._single()
        text = make_text(0, 30_000, 300)
        parts = ((text[:14_000], 77), (text[14_000:], 77 + 14_000 + 5))
        km, pos = [], []
        for part, base in parts:
            pk, pp = np_syncmers(part, k, s, True, "murmur", 42, wide)
            c0 = dict(st.collectives)
            assert st.append_sequences(part, pos_base=base) == len(pk) > 1000
            assert {n: v - c0[n] for n, v in st.collectives.items()} == {"counts": 1, "payload": 1, "votes": 3, "reduce": 0}, st.collectives
            km.append(pk); pos.append(pp + np.uint32(base))
        km, pos = np.concatenate(km), np.concatenate(pos)
        model = (WideIndexModel if wide else IndexModel)(km, pos)
        assert (st.size(), st.total()) == (model.size(), model.total())
        qt = np.concatenate([text[2000:5000], [ord("N")], make_text(1, 30_000, 300)[20_000:23_000], [10], text[13_900:14_200]]).astype(np.uint8)
        qk, qp = np_syncmers(qt, k, s, True, "murmur", 42, wide)
        qpos, offs, fpos = st.find_sequences(qt)
        eo, ep = model.find(qk)
        assert np.array_equal(qpos.cpu().numpy().view(np.uint32), qp) and len(qp) > 300
        assert np.array_equal(offs.cpu().numpy().astype(np.uint64), eo) and np.array_equal(fpos.cpu().numpy().view(np.uint32), ep)
        assert int(eo[-1]) > 200                                 # the stretches copied from the indexed text are found
        st.clear()
        assert st.build_sequences(text) == len(np_syncmers(text, k, s, True, "murmur", 42, wide)[1]) == st.total()
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
