"""GPU: kh_cigar_text against tests/records_model.cigar_text byte for byte, host and device memory: every digit count (lengths 1, 9, 10,
99, 100, ... 10^8, 2^28 - 1), every op code 0..15, empty rows at the start, in the middle and at the end, one row, 70 000 rows (more
than one scan tile), offsets that start beyond 0, descend or pass the runs (clamped), the count-only call and a short out_text."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import _capi as K  # noqa: E402
import records_model as RM  # noqa: E402
from stream_checks import to_dev  # noqa: E402

LENGTHS = [1, 9] + [x for p in range(1, 9) for x in (10 ** p, 10 ** (p + 1) - 1)][:-1] + [10 ** 8, 2 ** 28 - 1, 0]


def csr(rows):
    offs = np.zeros(len(rows) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(r) for r in rows])
    return offs, np.array([v for r in rows for v in r], dtype=np.uint32)


def all_cases():
    rng = np.random.RandomState(5)
    every = [(n << 4) | o for n in LENGTHS for o in range(16)]
    big_rows = [[int(v) for v in rng.randint(0, 2 ** 32, size=rng.randint(0, 4), dtype=np.uint64)] for _ in range(70000)]
    out = {"every_length_and_op_one_row": csr([every]), "one_run_per_row": csr([[v] for v in every]),
           "empty_rows": csr([[], [], every[:5], [], every[5:40], [], []]), "rows_70000": csr(big_rows), "only_empty_rows": csr([[], []])}
    offs, ops = csr([every[i:i + 7] for i in range(0, 140, 7)])
    out["starts_beyond_zero"] = (offs[3:].copy(), ops)
    d = offs.copy(); d[5:9] = d[5:9][::-1].copy()
    out["descending"] = (d, ops)
    b = offs.copy(); b[12:] += np.uint64(2 ** 40)
    out["beyond"] = (b, ops)
    return out


CASES = all_cases()


@pytest.fixture(scope="module")
def models():
    return {name: RM.cigar_text(*c) for name, c in CASES.items()}


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_model_byte_for_byte(models, name, dev):
    offs, ops = CASES[name]
    eo, et = models[name]
    mk = to_dev if dev else (lambda a: a)
    toff, text = kh.cigar_text(mk(offs), mk(ops))
    if dev:
        torch.cuda.synchronize()
        assert toff.dtype == torch.int64 and text.dtype == torch.uint8
        toff, text = toff.cpu().numpy(), text.cpu().numpy()
    assert [int(v) for v in toff.view(np.uint64)] == eo, name
    assert text.tobytes() == et, name


def test_the_model_prints_what_percent_d_prints(models):
    offs, ops = CASES["every_length_and_op_one_row"]
    eo, et = models["every_length_and_op_one_row"]
    assert et.decode() == "".join("%d%s" % (int(v) >> 4, ("MIDNSHP=X" + "?" * 7)[int(v) & 15]) for v in ops)
    assert sorted({len(RM.run_text(int(v))) for v in ops}) == list(range(2, 11))


@pytest.mark.parametrize("dev", [False, True])
def test_count_only_and_a_short_buffer(models, dev):
    offs, ops = CASES["empty_rows"]
    eo, et = models["empty_rows"]
    mk = to_dev if dev else (lambda a: a)
    o, p = mk(offs), mk(ops)
    ptr = lambda x: x.data_ptr() if dev else x.ctypes.data      # noqa: E731
    for cap, with_text, want in ((0, False, K.KH_OK), (len(et) - 1, True, K.KH_ERR_INVALID), (len(et), True, K.KH_OK)):
        toff = mk(np.full(len(offs), 7, dtype=np.uint64))
        text = mk(np.full(max(cap, 1), 0x55, dtype=np.uint8))
        n = C.c_uint64(99)
        st = K.lib().kh_cigar_text(ptr(o), len(offs) - 1, ptr(p), len(ops), K.KH_MEM_DEVICE if dev else K.KH_MEM_HOST, ptr(toff), ptr(text) if with_text else None, cap,
                                   C.byref(n), 0, None)
        if dev:
            torch.cuda.synchronize()
            toff, text = toff.cpu().numpy(), text.cpu().numpy()
        assert (st, n.value) == (want, len(et))
        assert [int(v) for v in toff.view(np.uint64)] == eo
        assert text.tobytes() == (et if with_text and want == K.KH_OK else b"\x55" * max(cap, 1))
