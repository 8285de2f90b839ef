"""The Python call scaffold (kmerhash_amd/_call.py) on the host: argument buffers, the same-memory / same-length check, the output
allocator and its dtype table, the handle base class.  No GPU, no library call: milliseconds."""
import ctypes as C

import numpy as np
import pytest

from kmerhash_amd import _call as S
from kmerhash_amd import _capi as K

try:
    import torch
except Exception:  # pragma: no cover
    torch = None
needs_torch = pytest.mark.skipif(torch is None, reason="torch is not installed")


def read_back(b, dtype):
    """the n * words entries behind a host buffer's pointer"""
    words = b.obj.size // b.n if b.n else 1
    return np.ctypeslib.as_array(C.cast(b.ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(b.n * words,)).copy()


def test_buffer_over_host_containers():
    vals = [5, 2 ** 63 + 1, 7]
    for x in (vals, np.array(vals, dtype=np.uint64), np.repeat(np.array(vals, dtype=np.uint64), 2)[::2]):
        b = S._Buf(x, np.uint64)
        assert (b.n, b.where, b.device, b.dev) == (3, K.KH_MEM_HOST, None, False) and b.obj.flags.c_contiguous and b.obj.dtype == np.uint64
        assert b.ptr == b.obj.ctypes.data and read_back(b, np.uint64).tolist() == vals
    arr = np.array(vals, dtype=np.uint64)
    assert S._Buf(arr, np.uint64).obj is arr, "a contiguous array of the right dtype is not copied"
    strided = np.repeat(arr, 2)[::2]
    assert not strided.flags.c_contiguous and S._Buf(strided, np.uint64).obj is not strided
    assert S._Buf(np.array([1, 2], dtype=np.int64), np.uint32).obj.dtype == np.uint32


def test_text_buffer():
    for x in (b"ACGT", bytearray(b"ACGT"), np.frombuffer(b"ACGT", dtype=np.uint8), np.frombuffer(b"AxCxGxTx", dtype=np.uint8)[::2]):
        b = S._Buf.text(x)
        assert (b.n, b.where) == (4, K.KH_MEM_HOST) and b.obj.dtype == np.uint8 and read_back(b, np.uint8).tobytes() == b"ACGT"
    empty = S._Buf.text(b"")
    assert empty.n == 0 and empty.ptr_or_null is None and S._Buf.text(b"A").ptr_or_null == S._Buf.text(b"A").ptr is not None


@needs_torch
def test_cpu_tensor_goes_through_numpy():
    t = torch.tensor([[1, -2], [3, 4], [5, 6]], dtype=torch.int64)
    for x in (t, t[::2]):
        b = S._Buf(x, np.uint64)
        assert type(b.obj) is np.ndarray and b.where == K.KH_MEM_HOST and b.device is None and b.n == x.numel()
        assert read_back(b, np.uint64).tolist() == x.numpy().astype(np.uint64).ravel().tolist()
    assert S._Buf.text(torch.tensor([65, 67], dtype=torch.uint8)).obj.tobytes() == b"AC"
    w = S._Buf.keys(t, 2)
    assert w.n == 3 and type(w.obj) is np.ndarray and w.obj.shape == (3, 2)
    assert S._is_tensor(t) and not S._is_tensor(np.zeros(1))


def test_key_buffers_count_keys():
    rows = np.arange(10, dtype=np.uint64).reshape(5, 2)
    assert S._Buf.keys(rows.ravel()).n == 10 and S._Buf.keys(rows.ravel(), 1).n == 10
    assert S._Buf.keys(rows, 1).n == 10, "64-bit keys: every entry is a key, whatever the shape (pair arrays go this way)"
    w = S._Buf.keys(rows, 2)
    assert w.n == 5 and w.obj.size == 10 and read_back(w, np.uint64).tolist() == list(range(10))
    assert S._Buf.keys(rows[::2], 2).n == 3 and S._Buf.keys(np.zeros((0, 2), dtype=np.uint64), 2).n == 0
    assert S._Buf.keys(rows.astype(np.int64).tolist(), 2).obj.dtype == np.uint64


@pytest.mark.parametrize("bad", [np.zeros(4, dtype=np.uint64), np.zeros((2, 3), dtype=np.uint64), np.zeros((2, 2, 2), dtype=np.uint64), [1, 2]])
def test_wide_keys_refuse_other_shapes(bad):
    with pytest.raises(ValueError, match=r"wide keys: expected shape \(n, 2\), got \(") as e:
        S._Buf.keys(bad, 2)
    assert str(np.asarray(bad).shape) in str(e.value)
    if torch is not None:
        with pytest.raises(ValueError, match=r"wide keys: expected shape \(n, 2\)"):
            S._Buf.keys(torch.from_numpy(np.asarray(bad, dtype=np.int64)), 2)


def test_same_memory_and_length_refusals():
    a, b, c = S._Buf([1, 2, 3], np.uint64), S._Buf([1, 2, 3], np.uint32), S._Buf([1, 2], np.uint32)
    S.check_same("m", a, b)
    S.check_same("m", a, None, b, None)          # absent optional arguments do not count
    S.check_same("m", a)
    S.check_same("m", a, c, length=False)
    with pytest.raises(ValueError, match="^the caller's words$"):
        S.check_same("the caller's words", a, b, c)
    far = S._Buf([1, 2, 3], np.uint32)
    far.where = K.KH_MEM_DEVICE                  # (what a CUDA tensor would say)
    with pytest.raises(ValueError, match="^elsewhere$"):
        S.check_same("elsewhere", a, far)
    with pytest.raises(ValueError, match="^elsewhere$"):
        S.check_same("elsewhere", a, b, far, length=False)
    S.check_same("m", a, far, memory=False)
    with pytest.raises(ValueError):
        S.check_same("m", a, c, memory=False)


@pytest.mark.parametrize("np_dtype", [np.uint64, np.uint32, np.int32, np.uint8])
@pytest.mark.parametrize("shape", [0, 7, (3, 2), (0, 2)])
def test_allocator_on_the_host(np_dtype, shape):
    like = S._Buf([1], np.uint64)
    for zero in (False, True):                   # host outputs are zeroed either way
        a, ptr = S.alloc(like, shape, np_dtype, zero=zero)
        assert type(a) is np.ndarray and a.dtype == np_dtype and a.shape == (shape if isinstance(shape, tuple) else (shape,))
        assert not a.any() and a.flags.c_contiguous and ptr == a.ctypes.data
    a, ptr = S.alloc(S.HOST, shape, np_dtype, empty=True)
    assert (ptr is None) == (a.size == 0) and (a.size == 0 or ptr == a.ctypes.data)
    assert S.alloc(S.HOST, shape, np_dtype)[1] is not None, "without the flag a zero-length output still has a pointer to pass"


@needs_torch
def test_dtype_table_pairs_equal_element_sizes():
    assert set(S.TORCH_DTYPE) == {np.uint64, np.uint32, np.int32, np.uint8}
    for np_dtype, torch_dtype in S.TORCH_DTYPE.items():
        assert torch.empty(0, dtype=torch_dtype).element_size() == np.dtype(np_dtype).itemsize, (np_dtype, torch_dtype)
    assert S.TORCH_DTYPE[np.uint64] is torch.int64 and S.TORCH_DTYPE[np.uint32] is torch.int32
    assert S.TORCH_DTYPE[np.int32] is torch.int32 and S.TORCH_DTYPE[np.uint8] is torch.uint8


def test_stream_rule_and_status_check_on_the_host():
    assert S.stream_of(S._Buf([1], np.uint64), 0) is None and S.stream_of(S.HOST, 0) is None
    S.check(K.KH_OK, "kh_anything")
    with pytest.raises(K.KhError, match="KH_ERR_INVALID: kh_anything") as e:
        S.check(K.KH_ERR_INVALID, "kh_anything")
    assert e.value.status == K.KH_ERR_INVALID and type(e.value) is K.KhError


class FakeRows:
    """stands in for the loaded library: a count-scan-emit entry point that records its calls, reports `count` rows and, given room,
    fills them with 1, 2, 3, ...; statuses: one per call"""

    def __init__(self, count, statuses=(K.KH_OK, K.KH_OK), itemsize=4):
        self.count, self.statuses, self.itemsize, self.calls = count, list(statuses), itemsize, []

    def kh_fake_rows(self, *args):
        self.calls.append(args)
        lead, (out, cap, n), rest = args[:3], args[3:6], args[6:]
        n._obj.value = self.count
        if out is not None and cap >= self.count:
            C.memmove(out, np.arange(1, self.count + 1, dtype={4: np.uint32, 1: np.uint8}[self.itemsize]).ctypes.data, self.count * self.itemsize)
        return self.statuses[len(self.calls) - 1]


def two_pass_with(monkeypatch, fake, np_dtype, trail=()):
    monkeypatch.setattr(K, "lib", lambda: fake)
    return S.two_pass("kh_fake_rows", ("lead", 7, None), S.HOST, np_dtype, 3, trail=trail)


@pytest.mark.parametrize("np_dtype,trail", [(np.uint32, ()), (np.uint8, ()), (np.uint32, (0x1111, 0x2222))])
def test_two_pass_counts_allocates_and_emits(monkeypatch, np_dtype, trail):
    fake = FakeRows(5, itemsize=np.dtype(np_dtype).itemsize)
    out = two_pass_with(monkeypatch, fake, np_dtype, trail)
    assert type(out) is np.ndarray and out.dtype == np_dtype and out.tolist() == [1, 2, 3, 4, 5]
    first, second = fake.calls
    assert first[:3] == second[:3] == ("lead", 7, None), "the leading arguments of both passes"
    assert first[3] is None and first[4] == 0, "the count pass: a null output, capacity 0"
    assert second[3] == out.ctypes.data and second[4] == 5, "the emit pass: the exact allocation and the count as capacity"
    assert first[5]._obj is second[5]._obj and second[5]._obj.value == 5
    # what follows the triple: the trailing arguments (kh_chain_cigars: its two counter arrays), then device and stream
    assert first[6:] == second[6:] == trail + (3, None)


@pytest.mark.parametrize("np_dtype", [np.uint32, np.uint8])
def test_two_pass_makes_one_call_when_nothing_is_counted(monkeypatch, np_dtype):
    fake = FakeRows(0)
    out = two_pass_with(monkeypatch, fake, np_dtype)
    assert len(fake.calls) == 1 and fake.calls[0][3] is None and fake.calls[0][4] == 0
    assert type(out) is np.ndarray and out.dtype == np_dtype and out.shape == (0,), "empty, of the right dtype, in host memory"


@pytest.mark.parametrize("statuses,n_calls", [((K.KH_ERR_INVALID, K.KH_OK), 1), ((K.KH_OK, K.KH_ERR_INVALID), 2)])
def test_two_pass_raises_the_status_of_either_pass(monkeypatch, statuses, n_calls):
    fake = FakeRows(5, statuses)
    with pytest.raises(K.KhError, match="KH_ERR_INVALID: kh_fake_rows") as e:
        two_pass_with(monkeypatch, fake, np.uint32)
    assert e.value.status == K.KH_ERR_INVALID and len(fake.calls) == n_calls


@needs_torch
def test_two_pass_takes_memory_and_stream_from_the_buffer(monkeypatch):
    """a device buffer: the output is allocated where it lives and the stream rule is asked for that buffer and the call's device
    (no GPU: the allocator and the stream rule are stood in for)"""
    fake, asked = FakeRows(0), []
    far = S._Buf.memory()
    far.where, far.device = K.KH_MEM_DEVICE, "cuda:3"
    monkeypatch.setattr(K, "lib", lambda: fake)
    monkeypatch.setattr(S, "stream_of", lambda like, device: asked.append((like, device)) or 0xABC)
    monkeypatch.setattr(S, "alloc", lambda like, shape, np_dtype: asked.append((like, shape, np_dtype)) or ("the tensor", 0x5000))
    assert S.two_pass("kh_fake_rows", ("lead", 7, None), far, np.uint8, 3) == "the tensor"
    assert asked == [(far, 3), (far, 0, np.uint8)] and fake.calls[0][6:] == (3, 0xABC)


class FakeLib:
    """stands in for the loaded library: counts destroy calls, answers one status"""

    def __init__(self, status=K.KH_OK):
        self.status, self.destroyed, self.adopted = status, [], 0

    def kh_fake_create(self, href, *args):
        href._obj.value = 0x1000
        return self.status

    def kh_fake_destroy(self, h):
        self.destroyed.append(h.value)

    def kh_fake_last_error(self, h):
        return b"what the library said"

    def kh_fake_size(self, h, ref):
        ref._obj.value = 41
        return self.status


class Fake(S._Handle):
    PREFIX = "kh_fake_"
    STATUS_ERRORS = {K.KH_ERR_FULL: K.KhLogicError, K.KH_ERR_RETRY: K.KhRetry}


def test_handle_base_close_and_del():
    half = Fake.__new__(Fake)                    # __init__ raised before the handle existed
    half.close()
    half.__del__()
    h = Fake.__new__(Fake)
    h._L, h._h = FakeLib(), C.c_void_p(0x1000)
    assert h._fn("destroy").__self__ is h._L and h._scalar("size") == 41
    h.close()
    h.close()
    h.__del__()
    assert h._L.destroyed == [0x1000] and not h._h.value, "destroy once, however often close is called"
    never = Fake.__new__(Fake)
    never._L, never._h = FakeLib(), C.c_void_p()          # create failed: a null handle is not destroyed
    never.close()
    assert never._L.destroyed == []


def test_handle_base_status_check():
    h = Fake.__new__(Fake)
    h._L, h._h = FakeLib(), C.c_void_p(0x1000)
    h._chk(K.KH_OK)
    for st, exc in ((K.KH_ERR_INVALID, K.KhError), (K.KH_ERR_FULL, K.KhLogicError), (K.KH_ERR_RETRY, K.KhRetry)):
        with pytest.raises(K.KhError, match="what the library said") as e:
            h._chk(st)
        assert type(e.value) is exc and e.value.status == st
    with pytest.raises(K.KhError, match="kh_fake_update$"):          # a handle that keeps no last error names the call
        h._chk(K.KH_ERR_INVALID, "kh_fake_update")
    h._adopt_stream(S._Buf([1], np.uint64), None)          # host arguments: the handle's stream is left alone (FakeLib has no set_stream)
    h._h = C.c_void_p()
