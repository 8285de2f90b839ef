"""GPU: kh_sam_lines against its model (tests/samtext_model.py) byte for byte, offsets included, in host and in device memory: 0, 1, 65
and 257 lines (more than one wave and more than one block of either pass); CSR rows of length 0, 1, 7, 8, 9, 63, 64, 65 and 300 in
every text field, so that lines and pieces start on every residue mod 8; the extremes of every numeric column; all kinds of RNEXT,
RNAME -1, every tag mask, row indexes outside their CSR; the QUAL, MD and cs CSRs present or absent in all combinations; the count-only
call; the refusal of a short capacity, which leaves the output untouched."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
import samtext_cases as SC  # noqa: E402
import samtext_model as SM  # noqa: E402
from stream_checks import to_dev  # noqa: E402

_model = {}


def model(n, seed, absent=()):
    """the expected CSR of a case, computed once"""
    key = (n, seed, tuple(absent))
    if key not in _model:
        csrs, cols = SC.lines(n, seed, absent)
        h = lambda pair: None if pair is None else ([int(x) for x in pair[0]], pair[1].tobytes())      # noqa: E731
        _model[key] = SM.sam_lines(*(h(csrs[x]) for x in SC.CSRS), cols)
    return _model[key]


def run(n, seed, absent, dev):
    csrs, cols = SC.lines(n, seed, absent)
    put = to_dev if dev else (lambda a: a)
    offs, text = kh.sam_lines_text(*(None if csrs[x] is None else tuple(put(a) for a in csrs[x]) for x in SC.CSRS), [put(cols[c]) for c in SC.COLUMNS])
    if dev:
        assert offs.is_cuda and text.is_cuda and offs.dtype == torch.int64 and text.dtype == torch.uint8
        offs, text = offs.cpu().numpy(), text.cpu().numpy()
    return [int(v) for v in offs.view(np.uint64)], text.tobytes()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n", [0, 1, 65, 257])
def test_lines_equal_the_model(n, dev):
    eo, et = model(n, 3 + n)
    go, gt = run(n, 3 + n, (), dev)
    assert go == eo
    assert gt == et
    if n == 257:      # the case is what its docstring says: every residue, every mask, '=' and '*', rows outside, negative numbers
        csrs, cols = SC.lines(n, 3 + n)
        assert {o % 8 for o in eo} == set(range(8)) and set(range(16)) <= set(cols["tags"].tolist())
        assert (cols["rnext"] == -2).any() and (cols["rname"] == -1).any() and (cols["seq"] == 2 ** 31 - 1).any() and (cols["tlen"] == -2 ** 31).any()
        assert (cols["flag"] == 2 ** 32 - 1).any() and (cols["pos"] == 2 ** 32 - 1).any() and (cols["s2"] == -1).any()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("absent", [c for r in range(1, 4) for c in itertools.combinations(("qual", "md", "cs"), r)], ids="-".join)
def test_absent_csrs(absent, dev):
    assert run(65, 11, absent, dev) == model(65, 11, absent)


def test_no_csr_at_all_prints_stars():
    absent = SC.CSRS
    eo, et = model(65, 12, absent)
    assert run(65, 12, absent, True) == (eo, et) and et.split(b"\n")[0].split(b"\t")[0] == b"*"


def raw_call(csrs, cols, out_offsets, out_text, cap, dev):
    keep = []

    def ptr(a):
        if a is None:
            return None
        keep.append(to_dev(a) if dev and isinstance(a, np.ndarray) else a)
        return keep[-1].data_ptr() if dev else keep[-1].ctypes.data
    args = []
    for x in SC.CSRS:
        o, t = csrs[x]
        args += [ptr(o), ptr(t), len(o) - 1, len(t)]
    args += [ptr(cols[c]) for c in SC.COLUMNS]
    n = C.c_uint64(77)
    st = K.lib().kh_sam_lines(*args, len(cols["name"]), K.KH_MEM_DEVICE if dev else K.KH_MEM_HOST, ptr(out_offsets), ptr(out_text), cap, C.byref(n), 0, None)
    torch.cuda.synchronize()
    return st, n.value


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_count_only_and_a_short_capacity(dev):
    csrs, cols = SC.lines(65, 21)
    eo, et = model(65, 21)
    mk = (lambda a: to_dev(a)) if dev else (lambda a: a)
    back = (lambda a: a.cpu().numpy()) if dev else (lambda a: a)
    offs = mk(np.full(66, 7, dtype=np.uint64))
    st, n = raw_call(csrs, cols, offs, None, 0, dev)
    assert st == K.KH_OK and n == len(et) and [int(v) for v in back(offs).view(np.uint64)] == eo
    offs, out = mk(np.full(66, 7, dtype=np.uint64)), mk(np.full(len(et), 7, dtype=np.uint8))
    st, n = raw_call(csrs, cols, offs, out, len(et) - 1, dev)
    assert st == K.KH_ERR_INVALID and n == len(et) and [int(v) for v in back(offs).view(np.uint64)] == eo and (back(out) == 7).all()
    out = mk(np.full(len(et) + 8, 7, dtype=np.uint8))
    st, n = raw_call(csrs, cols, offs, out, len(et) + 8, dev)
    assert st == K.KH_OK and n == len(et) and back(out)[:len(et)].tobytes() == et and (back(out)[len(et):] == 7).all()
