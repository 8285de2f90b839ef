"""fsc::hyperloglog64<T, Hash, precision> on the GPU (reference hyperloglog64.hpp:142-475) over the C-ABI."""
import ctypes as C

import numpy as np

from . import _capi as K
from .table import _Buf, _hash_id, torch


def estimate_from_registers(registers, precision=12):
    """internal_estimate (hyperloglog64.hpp:201-236) on host registers (uint8[2^precision]); needs no GPU"""
    regs = np.ascontiguousarray(registers, dtype=np.uint8)
    if regs.size != (1 << precision):
        raise ValueError("expected %d registers" % (1 << precision))
    d = C.c_double()
    st = K.lib().kh_hll_estimate_registers(regs.ctypes.data, precision, C.byref(d))
    if st != K.KH_OK:
        raise K.KhError(st, "kh_hll_estimate_registers")
    return d.value


def estimate_global(hll, group=None):
    """estimate_global (hyperloglog64.hpp:482-484): the estimate over the registers of ALL ranks, merged with an all-reduce(max)
    (merge_distributed :477-479; RCCL when the process group's backend is nccl).  `hll`: anything with registers() -> uint8 array and
    .precision.  Collective."""
    import torch.distributed as dist
    regs = np.ascontiguousarray(hll.registers(), dtype=np.uint8)
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        t = torch.from_numpy(regs.copy())
        if dist.get_backend(group) == "nccl":
            t = t.cuda()
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        regs = t.cpu().numpy()
    return estimate_from_registers(regs, hll.precision)


def estimate_average_per_rank(hll, group=None):
    """estimate_average_per_rank (hyperloglog64.hpp:487-489): the global estimate divided by the number of ranks (hashed keys spread
    evenly): what a rank's local table must hold"""
    import torch.distributed as dist
    p = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    return estimate_global(hll, group) / float(p)


class hyperloglog64:
    def __init__(self, precision=12, ignore_msb=0, hash="murmur3avx64", seed=43, device=0):
        self._L = K.lib()
        self._h = C.c_void_p()
        self.precision = precision
        self.device = device
        st = self._L.kh_hll_create(C.byref(self._h), precision, ignore_msb, _hash_id(hash), seed, device)
        if st != K.KH_OK:
            self._h = C.c_void_p()
            raise K.KhError(st, "kh_hll_create failed")

    # est_error_rate (hyperloglog64.hpp:262): 1.04 / 2^(precision/2)
    @property
    def est_error_rate(self):
        return 1.04 / float(1 << (self.precision >> 1))

    def _chk(self, st, what):
        if st != K.KH_OK:
            raise K.KhError(st, what)

    def _stream(self, b):
        """a call with a device argument runs on torch's current stream (the argument is ready in that stream's order).  merge, clear,
        registers and estimate have none and do not adopt it: they run on the stream of the last such call, in call order behind it --
        kh_hll_set_stream waits for the old stream when it switches, kh_hll_merge for the other estimator's."""
        if b.where == K.KH_MEM_DEVICE and torch is not None:
            self._L.kh_hll_set_stream(self._h, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    def update(self, keys):
        b = _Buf(keys, np.uint64, 8)
        self._stream(b)
        self._chk(self._L.kh_hll_update(self._h, b.ptr, b.n, b.where), "kh_hll_update")

    def update_via_hashval(self, hashes):
        b = _Buf(hashes, np.uint64, 8)
        self._stream(b)
        self._chk(self._L.kh_hll_update_via_hashval(self._h, b.ptr, b.n, b.where), "kh_hll_update_via_hashval")

    def update_wide(self, keys):
        """16-byte keys: (n, 2) numpy uint64 array or CUDA int64 tensor ({w0, w1} per key; a device tensor must be 16-byte aligned).
        The registers afterwards equal update_via_hashval(hash_batch_wide(keys)) with the estimator's hash and seed."""
        from .wide import _keys
        b = _keys(keys)
        self._stream(b)
        self._chk(self._L.kh_hll_update_wide(self._h, b.ptr, b.n // 2, b.where), "kh_hll_update_wide")

    def _from_text(self, fn, text, k, canonical):
        if isinstance(text, (bytes, bytearray)):
            text = np.frombuffer(text, dtype=np.uint8)
        b = _Buf(text, np.uint8, 1)
        self._stream(b)
        n = C.c_uint64()
        self._chk(getattr(self._L, fn)(self._h, b.ptr, b.n, k, 1 if canonical else 0, b.where, C.byref(n)), fn)
        return n.value

    def update_from_sequence(self, seq, k, canonical=True):
        """one pass text -> k-mers -> hash -> registers, no k-mer written (k = 1..64; bytes / uint8 array on the host or a uint8 CUDA
        tensor at any byte alignment).  The registers afterwards equal update(kmers_from_sequence(seq, k, canonical)) for k <= 32 and
        update_wide(kmers128_from_sequence(seq, k, canonical)) for k > 32.  Returns the number of valid windows."""
        return self._from_text("kh_hll_update_from_sequence", seq, k, canonical)

    def update_from_fastq(self, text, k, canonical=True):
        """update_from_sequence over raw FASTQ text (whole 4-line records): only the sequence lines yield k-mers"""
        return self._from_text("kh_hll_update_from_fastq", text, k, canonical)

    def text_grid(self, n):
        """the number of persistent workgroups the text passes launch for a text of n bytes: one per tile of TEXT_TILE start positions,
        at most TEXT_WGS_PER_CU per compute unit; workgroup g handles tiles g, g + grid, g + 2 grid, ..."""
        cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        return max(1, min((int(n) + self.TEXT_TILE - 1) // self.TEXT_TILE, self.TEXT_WGS_PER_CU * cus))

    TEXT_TILE = 4096          # KH_KM_TILE
    TEXT_WGS_PER_CU = 4       # KH_HLL_TEXT_WGS_PER_CU

    def merge(self, other):
        self._chk(self._L.kh_hll_merge(self._h, other._h), "kh_hll_merge")

    def clear(self):
        self._chk(self._L.kh_hll_clear(self._h), "kh_hll_clear")

    def registers(self):
        out = np.zeros(1 << self.precision, dtype=np.uint8)
        self._chk(self._L.kh_hll_registers(self._h, out.ctypes.data), "kh_hll_registers")
        return out

    def estimate(self):
        d = C.c_double()
        self._chk(self._L.kh_hll_estimate(self._h, C.byref(d)), "kh_hll_estimate")
        return d.value

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.kh_hll_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
