"""The array namespace of the mapper's glue (kmerhash_amd.mapper, sam, targets): the few array operations that turn one stage's columns
into the next stage's arguments, stated once for numpy arrays (NUMPY) and once for torch tensors on one device (Torch(device)), so that
every glue step is written once over a namespace argument.  Only what the glue uses is here; this is no general array API.

The two differ in the one thing that is easy to get wrong.  A host column of unsigned 32-bit numbers is a uint32 array; the device
column of the same bits is an int32 tensor.  widen() reads either as the unsigned numbers they stand for (a mask after .long()),
signed() widens a column that is signed (pairs.row, a chain number) or stays below 2^31 (a query offset, an anchor index) and masks
nothing; narrow() goes back to the container of the same bits that the C calls take (_call.TORCH_DTYPE holds the pairing).
Fancy indexing, comparison, arithmetic, & | ^ and len() are the containers' own."""
import numpy as np

from ._call import TORCH_DTYPE, _is_tensor, torch


class _Numpy:
    host = True                   # columns live in host memory: a check may read a value without a wait

    def col(self, x, np_dtype):
        """a column as given (array, list or tensor -- copied to the host) -> the array of its bits read as np_dtype"""
        return (x.cpu().numpy() if _is_tensor(x) else np.asarray(x)).view(np_dtype) if len(x) else np.zeros(0, dtype=np_dtype)

    def widen(self, x):
        """uint32 bits (a uint32 or int32 column; any other integer column as it stands) -> int64"""
        a = np.asarray(x)
        return (a.view(np.uint32) if a.dtype == np.int32 else a).astype(np.int64)

    def signed(self, x):
        return np.asarray(x).astype(np.int64)

    def narrow(self, x, np_dtype):
        """int64 or bool -> the container of np_dtype's bits (a negative number wraps)"""
        return np.asarray(x).astype(np_dtype)

    def place(self, a):
        """a host array -> this namespace's container of the same bits"""
        return a

    def searchsorted(self, a, v, right=False):
        return np.searchsorted(np.asarray(a).astype(np.int64, copy=False), np.asarray(v).astype(np.int64, copy=False), side="right" if right else "left")

    where, minimum, maximum = staticmethod(np.where), staticmethod(np.minimum), staticmethod(np.maximum)

    def arange(self, n):
        return np.arange(n, dtype=np.int64)

    def full(self, n, v, np_dtype=np.int64):
        return np.full(n, v, dtype=np_dtype)

    def concat(self, parts):
        return np.concatenate(parts)

    def nonzero(self, mask):
        return np.flatnonzero(mask)

    def prefix(self, x):
        """counts or a mask -> their exclusive prefix sums and the total: int64, one entry more"""
        return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(np.asarray(x), dtype=np.int64)])

    def ints(self, values):
        """0-d results (a sum, a min, a max) -> Python ints"""
        return [int(v) for v in values]


class Torch:
    host = False                  # reading a value is a wait for the stream: the glue asks for none beyond the documented ones

    def __init__(self, device):
        self.device = device

    def col(self, x, np_dtype):
        return x

    def widen(self, x):
        return x.long() & 0xFFFFFFFF if x.dtype == torch.int32 else x.long()

    def signed(self, x):
        return x.long()

    def narrow(self, x, np_dtype):
        return x.to(TORCH_DTYPE[np_dtype])

    def place(self, a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype))).to(self.device)

    def searchsorted(self, a, v, right=False):
        return torch.searchsorted(a, v, right=right)

    def where(self, c, a, b):
        return torch.where(c, a, b)

    def minimum(self, a, b):
        return torch.minimum(a, b) if _is_tensor(b) else a.clamp(max=b)

    def maximum(self, a, b):
        return torch.maximum(a, b) if _is_tensor(b) else a.clamp(min=b)

    def arange(self, n):
        return torch.arange(n, dtype=torch.int64, device=self.device)

    def full(self, n, v, np_dtype=np.int64):
        return torch.full((n,), int(v), dtype=TORCH_DTYPE.get(np_dtype, torch.int64), device=self.device)

    def concat(self, parts):
        return torch.cat(parts)

    def nonzero(self, mask):
        return torch.nonzero(mask).ravel()

    def prefix(self, x):
        return torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), torch.cumsum(x.long(), 0)])

    def ints(self, values):
        """... gathered into one small tensor and read once: the one wait of a glue step that must look at its numbers"""
        return torch.stack([v.long().reshape(()) for v in values]).tolist() if values else []


NUMPY = _Numpy()


def namespace_of(x):
    """the namespace of a column: a CUDA tensor gives torch on its device; anything else, a CPU tensor included, goes through numpy"""
    return Torch(x.device) if _is_tensor(x) and x.is_cuda else NUMPY
