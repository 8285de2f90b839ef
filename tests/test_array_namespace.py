"""The array namespace of the mapper's glue (kmerhash_amd/_xp.py) on the host: every operation on a numpy column and on the same bits as
a CPU tensor, element for element.  The torch statement is the one a device Mapping runs; here it runs on CPU tensors, so the
signed / unsigned handling is checked without a GPU.  No library call: milliseconds."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from kmerhash_amd import _xp  # noqa: E402

NP, TT = _xp.NUMPY, _xp.Torch(torch.device("cpu"))
U32 = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 5, 0x80000000], dtype=np.uint32)
I32 = np.array([-1, -2, 0, 7, -1], dtype=np.int32)
OFFS = np.array([0, 3, 3, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5], dtype=np.int64)      # ascending, up to 16 entries, past 2^32
EMPTY = {dt: np.zeros(0, dtype=dt) for dt in (np.uint32, np.int32, np.int64, np.uint8)}


def tensor(a):
    """the same bits as a CPU tensor: uint32 as int32, uint64 as int64"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype)).copy())


def same(a, t, np_dtype=None):
    """a numpy result and a torch result hold the same bits (and, asked for, the documented container dtypes)"""
    assert isinstance(a, np.ndarray) and isinstance(t, torch.Tensor)
    if np_dtype is not None:
        assert a.dtype == np_dtype and t.dtype == {np.uint32: torch.int32, np.int32: torch.int32, np.uint8: torch.uint8, np.uint64: torch.int64,
                                                   np.int64: torch.int64}[np_dtype]
    b = t.numpy()
    assert a.shape == b.shape and a.astype(np.int64).tolist() == (b.view(a.dtype) if a.dtype.itemsize == b.dtype.itemsize and a.dtype != bool else b).astype(np.int64).tolist()


def test_widening_reads_uint32_bits_and_leaves_signed_columns_alone():
    w = TT.widen(tensor(U32))
    assert w.dtype == torch.int64 and w.tolist() == [0, 1, 2147483647, 2147483648, 4294967295, 5, 2147483648]
    assert int(TT.widen(tensor(np.array([0x80000000], dtype=np.uint32)))[0]) == 2147483648      # not a negative number
    same(NP.widen(U32), w, np.int64)
    same(NP.widen(U32.view(np.int32)), w, np.int64)                      # a host column may hold the bits as int32 too
    s = TT.signed(tensor(I32))
    assert s.tolist() == [-1, -2, 0, 7, -1] and int(TT.signed(tensor(np.array([-1], dtype=np.int32)))[0]) == -1
    same(NP.signed(I32), s, np.int64)
    same(NP.widen(OFFS), TT.widen(tensor(OFFS)), np.int64)              # a 64-bit column is taken as it stands: nothing is masked
    assert TT.widen(tensor(OFFS)).tolist() == OFFS.tolist()
    same(NP.signed(np.array([0, 200, 255], dtype=np.uint8)), TT.signed(tensor(np.array([0, 200, 255], dtype=np.uint8))), np.int64)
    for dt in (np.uint32, np.int32):
        same(NP.widen(EMPTY[dt]), TT.widen(tensor(EMPTY[dt])), np.int64)
        same(NP.signed(EMPTY[dt]), TT.signed(tensor(EMPTY[dt])), np.int64)


@pytest.mark.parametrize("np_dtype", [np.uint32, np.int32, np.uint8, np.uint64])
def test_narrowing_gives_the_containers_the_c_calls_take(np_dtype):
    wide = {np.uint32: NP.widen(U32), np.int32: NP.signed(I32), np.uint8: np.array([0, 1, 255, 1], dtype=np.int64), np.uint64: OFFS}[np_dtype]
    same(NP.narrow(wide, np_dtype), TT.narrow(tensor(wide), np_dtype), np_dtype)
    same(NP.narrow(EMPTY[np.int64], np_dtype), TT.narrow(tensor(EMPTY[np.int64]), np_dtype), np_dtype)
    if np_dtype is np.uint32:      # there and back: the bits of the column; -1 wraps to the bits of 0xFFFFFFFF
        assert NP.narrow(wide, np_dtype).tolist() == U32.tolist() and TT.narrow(tensor(wide), np_dtype).numpy().view(np.uint32).tolist() == U32.tolist()
        minus = np.array([-1, 3], dtype=np.int64)
        same(NP.narrow(minus, np.uint32), TT.narrow(tensor(minus), np.uint32), np.uint32)
        assert NP.narrow(minus, np.uint32).tolist() == [0xFFFFFFFF, 3]
    if np_dtype is np.uint8:       # a boolean mask narrows to 0 / 1
        mask = np.array([True, False, True])
        same(NP.narrow(mask, np.uint8), TT.narrow(torch.from_numpy(mask), np.uint8), np.uint8)


def test_host_columns_and_placing():
    for a in (U32, I32, OFFS, OFFS.astype(np.uint64), np.array([1, 0, 255], dtype=np.uint8), EMPTY[np.uint32]):
        t = TT.place(a)
        assert isinstance(t, torch.Tensor) and t.device.type == "cpu" and NP.place(a) is a
        same(a, t)
        assert TT.col(t, a.dtype.type) is t                               # a tensor column is used where it is
        back = NP.col(t, a.dtype.type)                                    # the host reads its bits as the dtype asked for
        assert back.dtype == a.dtype and back.tolist() == a.tolist()
    assert NP.col([], np.uint32).dtype == np.uint32 and len(NP.col([], np.uint32)) == 0
    assert NP.col(U32.view(np.int32), np.uint32).tolist() == U32.tolist()


@pytest.mark.parametrize("right", [False, True])
def test_searchsorted_over_offsets_past_2_32(right):
    for hay, needles in ((OFFS, np.array([0, 1, 3, 4, 2 ** 31, 2 ** 32, 2 ** 32 + 6, -1], dtype=np.int64)), (OFFS, EMPTY[np.int64]), (EMPTY[np.int64], OFFS),
                         (NP.widen(np.sort(U32)), NP.widen(U32))):
        same(NP.searchsorted(hay, needles, right), TT.searchsorted(tensor(hay), tensor(needles), right), np.int64)
    # a host CSR is uint64: searched as the int64 it fits, not through float64
    assert NP.searchsorted(OFFS.astype(np.uint64), np.array([2 ** 32], dtype=np.int64), right).tolist() == [6 if right else 5]


def test_elementwise_and_constructors():
    a, b = NP.widen(U32), NP.widen(U32[::-1].copy())
    ta, tb = tensor(a), tensor(b)
    mask = a > b
    same(NP.where(mask, a, b), TT.where(torch.from_numpy(mask), ta, tb), np.int64)
    same(NP.minimum(a, b), TT.minimum(ta, tb), np.int64)
    same(NP.maximum(a, b), TT.maximum(ta, tb), np.int64)
    s = NP.signed(I32)
    same(NP.maximum(s, 0), TT.maximum(tensor(s), 0), np.int64)           # a scalar bound: the clamp of an index
    same(NP.minimum(s, 0), TT.minimum(tensor(s), 0), np.int64)
    assert NP.maximum(s, 0).tolist() == [0, 0, 0, 7, 0]
    for n in (0, 1, 16):
        same(NP.arange(n), TT.arange(n), np.int64)
        same(NP.full(n, 2 ** 32), TT.full(n, 2 ** 32), np.int64)
        same(NP.full(n, -1), TT.full(n, -1), np.int64)
        same(NP.full(n, 0, np.uint32), TT.full(n, 0, np.uint32), np.uint32)
        same(NP.full(n, 1, np.uint8), TT.full(n, 1, np.uint8), np.uint8)
    same(NP.concat([a, OFFS, EMPTY[np.int64]]), TT.concat([ta, tensor(OFFS), tensor(EMPTY[np.int64])]), np.int64)
    same(NP.concat([EMPTY[np.int64], EMPTY[np.int64]]), TT.concat([tensor(EMPTY[np.int64])] * 2), np.int64)


def test_indexing_nonzero_and_length():
    a = NP.widen(U32)
    ta = tensor(a)
    idx = np.array([6, 0, 3, 3], dtype=np.int64)
    same(a[idx], ta[tensor(idx)], np.int64)
    same(a[EMPTY[np.int64]], ta[tensor(EMPTY[np.int64])], np.int64)
    same(NP.arange(6) ^ 1, TT.arange(6) ^ 1, np.int64)                   # the partner of a mate
    for mask in (a >= 2 ** 31, a < 0, np.zeros(0, dtype=bool)):
        col, tcol = (a, ta) if len(mask) else (EMPTY[np.int64], tensor(EMPTY[np.int64]))
        sel, tsel = NP.nonzero(mask), TT.nonzero(torch.from_numpy(mask))
        same(sel, tsel, np.int64)
        same(col[sel], tcol[tsel], np.int64)
        assert len(sel) == len(tsel) == int(mask.sum())
    assert len(ta) == len(a) == 7


def test_the_namespace_of_a_column():
    assert _xp.namespace_of(U32) is NP and _xp.namespace_of([1, 2]) is NP
    assert _xp.namespace_of(tensor(U32)) is NP, "a CPU tensor goes through numpy"
    assert NP.host and not TT.host and TT.device == torch.device("cpu")
