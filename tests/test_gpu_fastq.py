"""GPU: kh_fastq_records, kh_pack_rows and read_fastq against tests/fastq_model.py, bit for bit: every case of tests/fastq_cases.py
on host arrays and on device tensors, with and without the mate suffix stripped; columns with more room than records keep their
pre-fill beyond the records, a call with too little room writes nothing but the count; the unaligned path (the text viewed at byte
offsets 1..7 of its buffer); for every well-formed case the k-mers of the packed reads are the k-mers kh_kmers_from_fastq finds in the
raw text, at the positions the record columns give them.  pack_rows: every row length around the wave step at every alignment pair,
every kind of separator, rows out of the text, stores clamped at the end of out, two calls interleaving into one buffer; bytes no row
covers keep their pre-fill."""
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
from kmerhash_amd import kmers as KM  # noqa: E402
import fastq_cases as FC  # noqa: E402
import fastq_model as FM  # noqa: E402
from stream_checks import to_dev  # noqa: E402

_MODEL = {}


def model(case, strip):
    """the model's answer, computed once per (case, strip) and shared"""
    if (case, strip) not in _MODEL:
        _MODEL[case, strip] = FM.fastq_records(FC.CASES[case].text, 1 if strip else 0)
    return _MODEL[case, strip]


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def as_rows(r):
    cols = [host(c).view(np.uint32).tolist() for c in r[:5]] + [host(r.status).tolist()]
    return list(zip(*cols)) if len(cols[0]) else []


def view_at(raw, offset, dev):
    """the text as a view that starts `offset` bytes into its buffer"""
    buf = np.zeros(len(raw) + 16, dtype=np.uint8)
    buf = to_dev(buf) if dev else buf
    at = (offset - (buf.data_ptr() if dev else buf.ctypes.data)) % 8
    view = buf[at:at + len(raw)]
    view[:] = to_dev(np.frombuffer(raw, dtype=np.uint8)) if dev else np.frombuffer(raw, dtype=np.uint8)
    return view


@pytest.mark.parametrize("dev", [False, True], ids=["numpy", "tensors"])
@pytest.mark.parametrize("strip", [False, True], ids=["as_written", "strip_mate"])
@pytest.mark.parametrize("case", sorted(FC.CASES))
def test_records_equal_the_model(case, strip, dev):
    raw = FC.CASES[case].text
    rows, n_bad, tail = model(case, strip)
    text = to_dev(np.frombuffer(raw, dtype=np.uint8)) if dev else raw
    r = kh.fastq_records(text, strip_mate=strip)
    assert as_rows(r) == rows and (r.n_bad, r.tail_lines) == (n_bad, tail)
    assert all((c.is_cuda and c.dtype == torch.int32) if dev else c.dtype == np.uint32 for c in r[:5]) and (r.status.dtype == (torch.uint8 if dev else np.uint8))


@pytest.mark.parametrize("dev", [False, True], ids=["numpy", "tensors"])
@pytest.mark.parametrize("case", FC.ALIGN_CASES)
def test_records_of_a_text_at_any_byte_offset(case, dev):
    raw = FC.CASES[case].text
    rows, n_bad, tail = model(case, False)
    for offset in range(1, 8):
        text = view_at(raw, offset, dev)
        assert len(text) == len(raw) and (text.data_ptr() if dev else text.ctypes.data) % 8 == offset
        r = kh.fastq_records(text)
        assert as_rows(r) == rows and (r.n_bad, r.tail_lines) == (n_bad, tail), offset
        got = kh.read_fastq(text, strict=False)
        assert host(got.seq).tobytes() == FM.read_fastq([raw])["seq"], offset


def raw_call(text, cap, dev, count_only=False):
    """kh_fastq_records through ctypes over pre-filled columns of `cap` entries -> (status, counts, columns)"""
    mk = to_dev if dev else (lambda a: a)
    t = mk(np.frombuffer(text, dtype=np.uint8).copy())
    cols = [mk(np.full(cap, 0xABABABAB, dtype=np.uint32)) for _ in range(5)] + [mk(np.full(cap, 0xAB, dtype=np.uint8))]
    p = lambda x: x.data_ptr() if dev else x.ctypes.data      # noqa: E731
    n, bad, tail = C.c_uint64(77), C.c_uint64(77), C.c_uint32(77)
    ptrs = [None] * 6 if count_only else [p(c) for c in cols]
    st = K.lib().kh_fastq_records(p(t), len(text), 0, 1 if dev else 0, *ptrs, 0 if count_only else cap, C.byref(n), C.byref(bad), C.byref(tail), 0,
                                  torch.cuda.current_stream().cuda_stream if dev else None)
    torch.cuda.synchronize()
    return st, (n.value, bad.value, tail.value), [host(c).view(np.uint32 if i < 5 else np.uint8) for i, c in enumerate(cols)]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", ["many", "length_mismatch", "tail2", "only_newlines"])
def test_room_beyond_the_records_keeps_its_prefill_and_too_little_room_writes_nothing(case, dev):
    raw = FC.CASES[case].text
    rows, n_bad, tail = model(case, False)
    n = len(rows)
    assert raw_call(raw, 0, dev, count_only=True)[:2] == (K.KH_OK, (n, n_bad, tail))
    st, counts, cols = raw_call(raw, n + 37, dev)
    assert st == K.KH_OK and counts == (n, n_bad, tail)
    assert [tuple(int(c[i]) for c in cols) for i in range(n)] == rows
    assert all((c[n:] == (0xABABABAB if c.dtype == np.uint32 else 0xAB)).all() for c in cols)
    for cap in (n - 1, n // 2, 1):
        st, counts, cols = raw_call(raw, cap, dev)
        assert st == K.KH_ERR_INVALID and counts == (n, 77, 77), cap
        assert all((c == (0xABABABAB if c.dtype == np.uint32 else 0xAB)).all() for c in cols), cap


@pytest.mark.parametrize("dev", [False, True], ids=["numpy", "tensors"])
@pytest.mark.parametrize("case", sorted(n for n, c in FC.CASES.items() if c.good and c.recs))
def test_kmers_of_the_packed_reads_are_the_kmers_of_the_fastq_text(case, dev):
    k = 5
    raw = FC.CASES[case].text
    rows = model(case, False)[0]
    text = to_dev(np.frombuffer(raw, dtype=np.uint8)) if dev else raw
    reads = kh.read_fastq(text)
    km_s, pos_s = (host(x) for x in KM.kmers_from_sequence(reads.seq, k, with_positions=True))
    km_f, pos_f = (host(x) for x in KM.kmers_from_fastq(text, k, with_positions=True))
    assert np.array_equal(km_s, km_f) and len(km_f) == sum(max(0, r[3] - r[2] - k + 1) for r in rows)
    starts, pos_s, pos_f = host(reads.read_starts), pos_s.view(np.uint32).astype(np.int64), pos_f.view(np.uint32).astype(np.int64)
    s = np.searchsorted(starts, pos_s, side="right") - 1                     # the read of every window of the packed text
    seq_lo, seq_hi = (np.array([r[i] for r in rows], dtype=np.int64) for i in (2, 3))
    assert np.array_equal(pos_f, seq_lo[s] + pos_s - starts[s])               # ... is the record its position in the raw text lies in
    assert ((pos_f >= seq_lo[s]) & (pos_f <= seq_hi[s] - k)).all()


@pytest.mark.parametrize("dev", [False, True], ids=["numpy", "tensors"])
def test_read_fastq_equals_the_model(dev):
    mk = (lambda b: to_dev(np.frombuffer(b, dtype=np.uint8))) if dev else (lambda b: b)
    one, two, r1, r2 = FC.pair_texts()
    for texts, kw in [([FC.CASES[c].text], dict(strict=False)) for c in sorted(FC.CASES)] + [([one, two], dict()), ([one, two], dict(strip_mate=False, strict=False)),
                                                                                            ([one, FC.write(r2[:-3])], dict(strict=False))]:
        want = FM.read_fastq(texts, kw.get("strip_mate"))
        got = kh.read_fastq(*(mk(t) for t in texts), **kw)
        assert host(got.seq).tobytes() == want["seq"] and host(got.qual).tobytes() == want["qual"]
        assert host(got.read_starts).tolist() == want["read_starts"] and host(got.read_ends).tolist() == want["read_ends"]
        assert host(got.names[0]).astype(np.int64).tolist() == want["names"][0] and host(got.names[1]).tobytes() == want["names"][1]
        assert got.n_reads == want["n_reads"] and host(got.status).tolist() == want["status"]
        assert got.seq.is_cuda and got.names[0].is_cuda and got.read_starts.dtype == torch.int64 if dev else got.names[0].dtype == np.uint64
    with pytest.raises(ValueError, match="record 0 carries different names"):
        kh.read_fastq(mk(one), mk(two), strip_mate=False)


# ---- kh_pack_rows
_PACK = {}


def pack_model(sep, fill=0xfe):
    if (sep, fill) not in _PACK:
        text, lo, hi, dst, out_len = FC.pack_case()
        _PACK[sep, fill] = bytes(FM.pack_rows(bytes(text), lo.tolist(), hi.tolist(), dst.tolist(), sep, bytearray(bytes([fill]) * out_len)))
    return _PACK[sep, fill]


@pytest.mark.parametrize("dev", [False, True], ids=["numpy", "tensors"])
@pytest.mark.parametrize("sep", [-1, 0, 10, 255])
def test_pack_rows_of_every_length_and_alignment(sep, dev):
    text, lo, hi, dst, out_len = FC.pack_case()
    mk = to_dev if dev else (lambda a: a)
    out = mk(np.full(out_len, 0xfe, dtype=np.uint8))
    got = kh.pack_rows(mk(text), mk(lo), mk(hi), mk(dst), out_len, sep=None if sep < 0 else sep, out=out)
    assert got is out and host(got).tobytes() == pack_model(sep)      # (bytes no row covers keep their pre-fill: the model leaves them)
    fresh = kh.pack_rows(mk(text), mk(lo), mk(hi), mk(dst), out_len, sep=None if sep < 0 else sep)
    assert host(fresh).tobytes() == pack_model(sep, 0)      # out=None: zeroed bytes


@pytest.mark.parametrize("dev", [False, True], ids=["numpy", "tensors"])
def test_pack_rows_out_of_the_text_clamped_stores_and_two_calls_into_one_buffer(dev):
    mk = to_dev if dev else (lambda a: a)
    rng = np.random.RandomState(11)
    text = rng.randint(1, 250, size=3000).astype(np.uint8)
    u32, u64 = (lambda v: np.array(v, dtype=np.uint32)), (lambda v: np.array(v, dtype=np.uint64))
    # hi < lo, hi > n, lo > n, a row that ends at n; destinations at and beyond the end of out, a long row cut by it
    lo, hi, dst = [5, 2990, 3001, 2700, 100, 0, 40, 1200], [2, 3001, 3005, 3000, 100, 600, 50, 2800], [0, 9, 17, 30, 1040, 400, 2000, 1490]
    for out_len in (1500, 1491, 1031):
        for sep in (-1, 10):
            want = bytes(FM.pack_rows(bytes(text), lo, hi, dst, sep, bytearray(b"\xfe" * out_len)))
            got = kh.pack_rows(mk(text), mk(u32(lo)), mk(u32(hi)), mk(u64(dst)), out_len, sep=None if sep < 0 else sep, out=mk(np.full(out_len, 0xfe, dtype=np.uint8)))
            assert host(got).tobytes() == want, (out_len, sep)
    # two texts woven into one buffer: the rows of the first at the even places, of the second at the odd ones
    other = rng.randint(1, 250, size=2000).astype(np.uint8)
    la, lb = rng.randint(0, 40, size=50), rng.randint(0, 40, size=50)
    place = np.concatenate([[0], np.cumsum(np.stack([la, lb], 1).ravel() + 1)])
    a0, b0 = np.arange(50) * 41, np.arange(50) * 39
    out = mk(np.full(int(place[-1]) + 3, 0xfe, dtype=np.uint8))
    kh.pack_rows(mk(text), mk(u32(a0)), mk(u32(a0 + la)), mk(u64(place[:-1][0::2])), len(out), sep=10, out=out)
    kh.pack_rows(mk(other), mk(u32(b0)), mk(u32(b0 + lb)), mk(u64(place[:-1][1::2])), len(out), sep=10, out=out)
    want = b"".join(bytes(text[a:a + x]) + b"\n" + bytes(other[b:b + y]) + b"\n" for a, x, b, y in zip(a0, la, b0, lb)) + b"\xfe" * 3
    assert host(out).tobytes() == want
