"""fsc::hyperloglog64<T, Hash, precision> on the GPU (reference hyperloglog64.hpp:142-475) over the C-ABI."""
import ctypes as C

import numpy as np

from . import _capi as K
from ._call import HOST, _Buf, _Handle, alloc, check, torch
from .table import _hash_id


def estimate_from_registers(registers, precision=12):
    """internal_estimate (hyperloglog64.hpp:201-236) on host registers (uint8[2^precision]); needs no GPU"""
    regs = _Buf(np.asarray(registers), np.uint8)
    if regs.n != (1 << precision):
        raise ValueError("expected %d registers" % (1 << precision))
    d = C.c_double()
    check(K.lib().kh_hll_estimate_registers(regs.ptr, precision, C.byref(d)), "kh_hll_estimate_registers")
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


class hyperloglog64(_Handle):
    PREFIX = "kh_hll_"

    def __init__(self, precision=12, ignore_msb=0, hash="murmur3avx64", seed=43, device=0):
        self.precision = precision
        self.device = device
        self._create(precision, ignore_msb, _hash_id(hash), seed, device, hint="")

    # est_error_rate (hyperloglog64.hpp:262): 1.04 / 2^(precision/2)
    @property
    def est_error_rate(self):
        return 1.04 / float(1 << (self.precision >> 1))

    # A call with a device argument runs on torch's current stream (_adopt_stream: the argument is ready in that stream's order).  merge,
    # clear, registers and estimate have none and do not adopt it: they run on the stream of the last such call, in call order behind it --
    # kh_hll_set_stream waits for the old stream when it switches, kh_hll_merge for the other estimator's.  The estimator keeps no last
    # error: every status check names its entry point.

    def update(self, keys):
        b = _Buf.keys(keys)
        self._adopt_stream(b)
        self._chk(self._L.kh_hll_update(self._h, b.ptr, b.n, b.where), "kh_hll_update")

    def update_via_hashval(self, hashes):
        b = _Buf.keys(hashes)
        self._adopt_stream(b)
        self._chk(self._L.kh_hll_update_via_hashval(self._h, b.ptr, b.n, b.where), "kh_hll_update_via_hashval")

    def update_wide(self, keys):
        """16-byte keys: (n, 2) numpy uint64 array or CUDA int64 tensor ({w0, w1} per key; a device tensor must be 16-byte aligned).
        The registers afterwards equal update_via_hashval(hash_batch_wide(keys)) with the estimator's hash and seed."""
        b = _Buf.keys(keys, 2)
        self._adopt_stream(b)
        self._chk(self._L.kh_hll_update_wide(self._h, b.ptr, b.n, b.where), "kh_hll_update_wide")

    def _from_text(self, fn, text, k, canonical):
        b = _Buf.text(text)
        self._adopt_stream(b)
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
        regs, ptr = alloc(HOST, 1 << self.precision, np.uint8)
        self._chk(self._L.kh_hll_registers(self._h, ptr), "kh_hll_registers")
        return regs

    def estimate(self):
        d = C.c_double()
        self._chk(self._L.kh_hll_estimate(self._h, C.byref(d)), "kh_hll_estimate")
        return d.value
