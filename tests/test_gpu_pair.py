"""GPU: kh_pair_chains equals the model of tests/pair_model.py on every output array -- for every named case of tests/pair_cases.py, in
host memory (numpy) and in device memory (tensors), and for one random table of 2 000 pairs whose groups have 0, 1, 2, 5, 63, 64, 65 or
200 chains and whose scores tie often.  Device offsets that do not ascend leave guard words around every output intact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from pair_cases import CASES, random_table  # noqa: E402
from pair_model import NAMES, pair_model  # noqa: E402
from stream_checks import to_dev  # noqa: E402


def model(a):
    a = dict(a)
    return pair_model(a.pop("rs"), a.pop("re"), a.pop("rev"), a.pop("score"), a.pop("read_offsets"), a.pop("tid"), a.pop("use"), a.pop("mapq"), **a)


def on_device(a):
    return {k: to_dev(v) if isinstance(v, np.ndarray) else v for k, v in a.items()}


def host(x, like):
    return x.cpu().numpy().view(like.dtype) if isinstance(x, torch.Tensor) else x


def compare(got, want, what):
    for field, g, w in zip(NAMES, got, want):
        g = host(g, w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, field, g.dtype, g.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, field, bad[:5], g[bad[:5]], w[bad[:5]])


@pytest.mark.parametrize("name", sorted(CASES))
def test_named_case_equals_the_model(name):
    want = model(CASES[name])
    compare(kh.pair_chains(**CASES[name]), want, (name, "numpy"))
    got = kh.pair_chains(**on_device(CASES[name]))
    assert all(isinstance(g, torch.Tensor) and g.is_cuda for g in got)
    compare(got, want, (name, "tensors"))


@pytest.fixture(scope="module")
def table():
    a = random_table()
    return a, model(a)


def test_random_table_in_host_memory(table):
    a, want = table
    assert int(want[3].sum()) > 0 and int((want[5] > 1).sum()) > 100      # proper pairs, and pairs with a choice
    compare(kh.pair_chains(**a), want, "random, numpy")


def test_random_table_in_device_memory(table):
    a, want = table
    compare(kh.pair_chains(**on_device(a)), want, "random, tensors")


def test_random_table_without_the_optional_arrays(table):
    a, _ = table
    b = dict(a, tid=None, use=None, mapq=None)
    compare(kh.pair_chains(**on_device(b)), model(b), "random, no tid / use / mapq")


def test_bad_device_offsets_touch_nothing_outside_the_outputs(table):
    a, _ = table
    n, n_reads = len(a["rs"]), len(a["read_offsets"]) - 1
    rng = np.random.default_rng(3)
    offs = a["read_offsets"].copy()
    offs[rng.integers(0, n_reads + 1, size=300)] = rng.integers(0, 2 ** 40, size=300).astype(np.uint64)      # descending, far beyond n, anything
    offs[5] = np.uint64(2 ** 64 - 1)
    G = 64
    dts = (np.int32, np.uint8, np.int32, np.uint8, np.int32, np.uint32)
    sizes = (n_reads, n_reads, n_reads, n_reads // 2, n_reads // 2, n_reads // 2)
    outs = [torch.full((G + m + G,), 0x5A, dtype=kh._call.TORCH_DTYPE[dt], device="cuda") for dt, m in zip(dts, sizes)]
    d = on_device(dict(a, read_offsets=offs))
    st = kh._capi.lib().kh_pair_chains(d["rs"].data_ptr(), d["re"].data_ptr(), d["rev"].data_ptr(), d["score"].data_ptr(), d["tid"].data_ptr(), d["use"].data_ptr(),
                                       d["mapq"].data_ptr(), n, d["read_offsets"].data_ptr(), n_reads, 100, 2500, 3, kh._capi.KH_MEM_DEVICE,
                                       *(o.data_ptr() + G * o.element_size() for o in outs), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == kh._capi.KH_OK
    torch.cuda.synchronize()
    for o, m in zip(outs, sizes):
        h = o.cpu().numpy()
        assert (h[:G] == 0x5A).all() and (h[G + m:] == 0x5A).all()
    rows = outs[0].cpu().numpy()[G:G + n_reads]
    assert ((rows >= -1) & (rows < n)).all()
