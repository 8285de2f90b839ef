"""GPU: kh_anchor_targets bit for bit against tests/targets_model.py, in host and in device memory, over the cases of
tests/targets_cases.py: segments of 0, 1, 63, 64, 65, 129 and 300 anchors in one batch for tables of 1, 2, 64, 65,
KH_TARGETS_STAGED_MAX and KH_TARGETS_STAGED_MAX + 1 targets (the LDS path and the L2 path), anchors on a target's first base, on the
last place a seed fits, one past it, in a spacer and at 2^31 and beyond; a read of 65 anchors on 65 targets; reads on one target, which
keep their order; no segment array; a descending table, which gives the ids the header's loop gives.  Broken offsets are
KH_ERR_INVALID; two calls give identical bytes."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
import targets_cases as TC  # noqa: E402
from stream_checks import to_dev  # noqa: E402

CASES = TC.cases()
MODELS = {}
OUT = (("qpos", "q", np.uint32), ("rpos", "r", np.uint32), ("rev", "v", np.uint8), ("tid", "tid", np.uint32), ("src", "src", np.uint32),
       ("offsets", "g_off", np.uint64), ("seg", "g_seg", np.uint32), ("target", "g_tid", np.uint32))


def model(name):
    if name not in MODELS:
        MODELS[name] = CASES[name].model()
    return MODELS[name]


def run(case, dev, seg="case"):
    mk = to_dev if dev else (lambda a: a)
    seg = case.seg if isinstance(seg, str) else seg
    g = kh.group_anchors(mk(case.qpos), mk(case.rpos), mk(case.rev), (mk(case.t_start), mk(case.t_end)), case.k, None if seg is None else mk(seg))
    if dev:
        torch.cuda.synchronize()
    return {f: (getattr(g, f).cpu().numpy() if dev else getattr(g, f)).view(dt) for f, _, dt in OUT}


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_model(name, dev):
    case, exp = CASES[name], model(name)
    assert exp["ok"]
    got = run(case, dev)
    for f, mf, dt in OUT:
        assert got[f].dtype == dt and got[f].tolist() == exp[mf], f
    again = run(case, dev)
    assert all(got[f].tobytes() == again[f].tobytes() for f, _, _ in OUT), "a second call gives other bytes"
    if name == "identity":
        assert got["src"].tolist() == list(range(len(case.qpos))) and np.array_equal(got["qpos"], case.qpos) and np.array_equal(got["rpos"], case.rpos)


def test_targets_object_and_pair_agree():
    rng = np.random.RandomState(4)
    T = kh.Targets(["t%d" % i for i in range(30)], rng.randint(50, 90, size=30), spacer=40)
    r = rng.randint(0, int(T.ends[-1]) + 50, size=500).astype(np.uint32)
    q, v = np.arange(500, dtype=np.uint32), np.zeros(500, dtype=np.uint8)
    offs = np.array([0, 100, 500], dtype=np.uint64)
    a = kh.group_anchors(q, r, v, T, 15, offs)
    b = kh.group_anchors(q, r, v, (T.starts, T.ends), 15, offs)
    c = kh.group_anchors(to_dev(q), to_dev(r), to_dev(v), T, 15, to_dev(offs))
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.cpu().numpy().tobytes()
    # what locate says of an anchor's first and last base is what the call says of the anchor
    src = a.src.astype(np.int64)
    t0, t1 = T.locate(r[src])[0], T.locate(r[src].astype(np.int64) + 14)[0]
    tid = a.tid.astype(np.int64)
    assert np.array_equal(np.where(tid == kh.TARGET_NONE, -1, tid), np.where(t0 == t1, t0, -1))
    # locate on the device gives what it gives on the host
    dt, dl = T.locate(to_dev(r))
    ht, hl = T.locate(r)
    assert dt.dtype == torch.int64 and np.array_equal(dt.cpu().numpy(), ht) and np.array_equal(dl.cpu().numpy(), hl)
    assert T.to(0)[0] is T.to(0)[0] and T.to(0)[0].is_cuda


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_broken_offsets_are_refused_after_the_kernels(dev):
    case = CASES["sizes_nt64"]
    m = len(case.qpos)
    for name, offs in TC.broken_offsets(m).items():
        with pytest.raises(kh.KhError, match="KH_ERR_INVALID.*seg_offsets do not ascend"):
            run(case, dev, np.array(offs, dtype=np.uint64))
    got = run(case, dev)                                         # the next call is sound
    assert got["src"].tolist() == model("sizes_nt64")["src"]


def test_no_anchors():
    e32, e8 = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8)
    T = (np.array([0], dtype=np.uint32), np.array([100], dtype=np.uint32))
    g = kh.group_anchors(e32, e32, e8, T, 15, np.zeros(3, dtype=np.uint64))
    assert g.offsets.tolist() == [0] and all(len(x) == 0 for x in g[:5]) and len(g.seg) == 0 and len(g.target) == 0
    g = kh.group_anchors(to_dev(e32), to_dev(e32), to_dev(e8), tuple(to_dev(x) for x in T), 15)
    torch.cuda.synchronize()
    assert g.offsets.cpu().tolist() == [0] and g.offsets.dtype == torch.int64 and g.tid.dtype == torch.int32 and len(g.seg) == 0
