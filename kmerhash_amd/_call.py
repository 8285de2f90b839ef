"""The one scaffold of a Python call across the C-ABI: argument buffers, outputs, the stream rule, the status check, the two-pass call of
the count-scan-emit entry points, the count-then-emit call of the samplers and the base class of the handles.  table, wide, index, hll, kmers and seqs cross the C-ABI through it alone.

numpy arrays (and bytes) are host memory, torch CUDA tensors device memory; a CPU tensor goes through numpy.  torch is optional and
plumbing only: device buffers and the handle of the current stream."""
import ctypes as C

import numpy as np

from . import _capi as K
from ._capi import KhError

try:  # torch is optional for host-array use
    import torch
except Exception:  # pragma: no cover
    torch = None

# the dtype pairing: numpy dtype of a host container -> torch dtype of the device container that holds the same bits
TORCH_DTYPE = {} if torch is None else {np.uint64: torch.int64, np.uint32: torch.int32, np.int32: torch.int32, np.uint8: torch.uint8}


def _is_tensor(x):
    return torch is not None and isinstance(x, torch.Tensor)


class _Buf:
    """pointer + memory kind of one batch argument: obj (the contiguous container, kept alive), ptr, n (entries), where, device"""

    def __init__(self, x, np_dtype):
        if _is_tensor(x):
            if not x.is_cuda:
                x = x.cpu().numpy()
            else:
                if x.element_size() != np.dtype(np_dtype).itemsize:
                    raise TypeError("tensor element size %d, expected %d" % (x.element_size(), np.dtype(np_dtype).itemsize))
                self.obj = x.contiguous()
                self.ptr = self.obj.data_ptr()
                self.n = self.obj.numel()
                self.where = K.KH_MEM_DEVICE
                self.device = self.obj.device
                return
        a = np.ascontiguousarray(x, dtype=np_dtype)
        self.obj = a
        self.ptr = a.ctypes.data
        self.n = a.size
        self.where = K.KH_MEM_HOST
        self.device = None

    @classmethod
    def text(cls, x):
        """bytes / bytearray / uint8 array / uint8 tensor"""
        return cls(np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else x, np.uint8)

    @classmethod
    def keys(cls, x, words=1):
        """a key batch of `words` 64-bit words per key ((n, words)-shaped when words > 1); n counts keys"""
        if words == 1:
            return cls(x, np.uint64)
        if not (_is_tensor(x) and x.is_cuda):
            x = np.asarray(x.cpu().numpy() if _is_tensor(x) else x)
        if len(x.shape) != 2 or x.shape[1] != words:
            raise ValueError("wide keys: expected shape (n, %d), got %s" % (words, tuple(x.shape)))
        b = cls(x, np.uint64)
        b.n //= words
        return b

    @classmethod
    def memory(cls, device=None):
        """no argument, only a place for outputs: the host, or cuda:device"""
        b = cls.__new__(cls)
        b.obj, b.ptr, b.n = None, None, 0
        b.where, b.device = (K.KH_MEM_HOST, None) if device is None else (K.KH_MEM_DEVICE, torch.device("cuda", device))
        return b

    @property
    def dev(self):
        return self.where == K.KH_MEM_DEVICE

    @property
    def ptr_or_null(self):
        """what the calls that refuse a pointer to nothing take for an empty batch"""
        return self.ptr if self.n else None


HOST = _Buf.memory()


def check_same(msg, *bufs, memory=True, length=True):
    """the same-memory / same-length check of a call's batch arguments (None: an optional one that is absent): ValueError(msg) unless
    all live in the same memory (with `memory`) and hold equally many entries (with `length`)"""
    first, *rest = [b for b in bufs if b is not None]
    for b in rest:
        if (memory and b.where != first.where) or (length and b.n != first.n):
            raise ValueError(msg)


def alloc(like, shape, np_dtype, zero=False, empty=False):
    """an output where `like` lives -> (container, pointer).  Host arrays are always zeroed, device tensors only with `zero` (a fill is a
    launch on the caller's stream).  empty: a null pointer for a zero-length output."""
    if like.where == K.KH_MEM_DEVICE:
        t = (torch.zeros if zero else torch.empty)(shape, dtype=TORCH_DTYPE[np_dtype], device=like.device)
        return t, (None if empty and t.numel() == 0 else t.data_ptr())
    a = np.zeros(shape, dtype=np_dtype)
    return a, (None if empty and a.size == 0 else a.ctypes.data)


def stream_of(like, device):
    """the stream rule: device input -> the handle of torch's current stream on the call's `device` argument; host input -> None"""
    return torch.cuda.current_stream(device).cuda_stream if like.where == K.KH_MEM_DEVICE else None


def check(st, name):
    """status of a handle-free call -> KhError naming the entry point"""
    if st != K.KH_OK:
        raise KhError(st, name)


def two_pass(fn_name, lead, like, np_dtype, device, trail=()):
    """a count-scan-emit entry point called twice: the count pass with a null output and capacity 0, an allocation of the exact size
    where `like` lives, the emit pass -- skipped when the count is zero -> the output.  lead: the arguments before the (out, cap, n)
    triple; trail: those between the triple and (device, stream), as kh_chain_cigars has them"""
    fn, n, stream = getattr(K.lib(), fn_name), C.c_uint64(), stream_of(like, device)
    check(fn(*lead, None, 0, C.byref(n), *trail, device, stream), fn_name)
    out, ptr = alloc(like, n.value, np_dtype)
    if n.value:
        check(fn(*lead, ptr, n.value, C.byref(n), *trail, device, stream), fn_name)
    return out


def count_then_emit(fn_name, words, text, params, device):
    """the sampled front ends (kh_minimizers_from_* / kh_syncmers*_from_*): a count pass, an exact allocation, the emit pass -- skipped
    when nothing was picked -> (k-mers of `words` 64-bit words, positions)"""
    b = _Buf.text(text)
    stream, fn, n_out = stream_of(b, device), getattr(K.lib(), fn_name), C.c_uint64()
    args = (b.ptr, b.n, *params, b.where)
    check(fn(*args, None, None, 0, C.byref(n_out), device, stream), fn_name)
    m = n_out.value
    km, kptr = alloc(b, m if words == 1 else (m, words), np.uint64)
    pos, pptr = alloc(b, m, np.uint32)
    if m:
        check(fn(*args, kptr, pptr, m, C.byref(n_out), device, stream), fn_name)
    return km, pos


class _Handle:
    """an object of the library behind the C entry points PREFIX + name: create / destroy, the status check, the stream rule"""
    PREFIX = None
    WORDS = 1                     # 64-bit words per key
    STATUS_ERRORS = {}            # statuses that raise a subclass of KhError

    def _create(self, *args, hint=" (is a GPU visible and the HIP library built?)"):
        self._L = K.lib()
        self._h = C.c_void_p()
        st = self._fn("create")(C.byref(self._h), *args)
        if st != K.KH_OK:
            self._h = C.c_void_p()
            raise KhError(st, "%screate failed%s" % (self.PREFIX, hint))

    def _fn(self, name):
        return getattr(self._L, self.PREFIX + name)

    def _chk(self, st, what=None):
        """what: the message of a handle that keeps no last error"""
        if st != K.KH_OK:
            raise self.STATUS_ERRORS.get(st, KhError)(st, what or self._fn("last_error")(self._h).decode())

    def _adopt_stream(self, *bufs):
        """the handle's work goes to torch's current stream on its device when a device argument is involved (None: an absent one)"""
        for b in bufs:
            if b is not None and b.where == K.KH_MEM_DEVICE:
                self._fn("set_stream")(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
                return

    def _scalar(self, name):
        v = C.c_uint64()
        self._chk(self._fn(name)(self._h, C.byref(v)))
        return v.value

    def _profile(self):
        buf = C.create_string_buffer(1 << 16)
        self._chk(self._fn("profile_dump")(self._h, buf, len(buf)))
        prof = {}
        for line in buf.value.decode().splitlines():
            name, launches, ms = line.split()
            prof[name] = (int(launches), float(ms))
        return prof

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
