"""GPU: the count-scan-emit protocol of the six mapper calls that share it -- kh_chain_cigars, kh_chain_ends, kh_chain_records, kh_cigar_text,
kh_record_diffs, kh_oriented_rows -- through the C ABI, in host and in device memory, on the smallest batch that makes each of them emit
something: two reads of 40 bases against a reference of 200, k = 11, each read one chain of three anchors with one substitution between
the first two and a one-base insertion between the last two, the second read on the reverse strand.  Per call: a count pass with a null
output; an emit pass with the exact capacity; one with the capacity one short, which is refused with the count and the offsets written
and the output untouched; one with room to spare, which leaves the room untouched; and no rows at all.  The expected values are those of
the models the tests of each stage use, fed with each other's results."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kmerhash_amd import _capi as K  # noqa: E402
import cigar_model as CM  # noqa: E402
import diffs_model as DM  # noqa: E402
import edits_model as EDM  # noqa: E402
import ends_model as ENM  # noqa: E402
import orient_model as OM  # noqa: E402
import records_model as RM  # noqa: E402
from ends_cases import revcomp  # noqa: E402
from stream_checks import to_dev  # noqa: E402

KMER, READ, MAX_EDITS, CLIP_COST = 11, 40, 31, 4
SENTINEL = 0xA5
ENTRIES = ["kh_chain_cigars", "kh_chain_ends", "kh_chain_records", "kh_cigar_text", "kh_record_diffs", "kh_oriented_rows"]
u8, u32, i32, u64 = np.uint8, np.uint32, np.int32, np.uint64


def arr(x, dt):
    return np.array(x, dtype=dt)


def text(b):
    return np.frombuffer(bytes(b), dtype=u8).copy()


@pytest.fixture(scope="module")
def batch():
    """the inputs and the model's outputs of every stage -> dict"""
    rng = random.Random(2)
    ref = bytes(rng.choice(b"ACGT") for _ in range(200))
    other = lambda b, *more: next(c for c in b"ACGT" if c != b and c not in more)      # noqa: E731
    reads, qpos, rpos, rev = [], [], [], []
    for r0, rv in ((50, 0), (120, 1)):
        s = revcomp(ref[r0:r0 + READ - 1]) if rv else ref[r0:r0 + READ - 1]           # the 39 reference bases the read faces, in read order
        # 2 bases, a seed, X and a base, a seed, an inserted base and a base, a seed, 1 base
        read = s[:13] + bytes([other(s[13])]) + s[14:26] + bytes([other(s[25], s[26])]) + s[26:]
        assert len(read) == READ
        for q, j in ((2, 2), (15, 15), (28, 27)):                                      # seed at read offset q = offset j of s
            assert read[q:q + KMER] == s[j:j + KMER]
            qpos.append(len(reads) * READ + q); rpos.append(r0 + (READ - 1 - KMER - j if rv else j)); rev.append(rv)
        reads.append(read)
    d = {"qtext": text(b"".join(reads)), "rtext": text(ref), "qpos": arr(qpos, u32), "rpos": arr(rpos, u32), "rev": arr(rev, u8),
         "pred": arr([-1, 0, 1, -1, 3, 4], i32), "chain": arr([0, 0, 0, 1, 1, 1], i32), "first": arr([0, 3], u32), "last": arr([2, 5], u32),
         "q_lo": arr([0, READ], u32), "q_hi": arr([READ, 2 * READ], u32), "rev_row": arr([0, 1], u8)}
    anchors = [d[f] for f in ("qtext", "rtext", "qpos", "rpos", "rev")]
    d["link"] = np.asarray(EDM.chain_edits_model(*anchors, d["pred"], d["chain"], 2, KMER, 0, MAX_EDITS)[0], dtype=i32)
    assert d["link"].tolist() == [-1, 1, 1, -1, 1, 1]
    d["lk_offsets"], d["lk_ops"], d["c_ins"], d["c_del"] = CM.chain_cigars_model(*anchors, d["pred"], d["chain"], 2, KMER, d["link"])
    d["e_q"], d["e_r"], d["e_edits"], d["e_clip"], d["en_offsets"], d["en_ops"] = ENM.chain_ends_model(*anchors, d["first"], d["last"], d["q_lo"], d["q_hi"], KMER, 0,
                                                                                                    MAX_EDITS, CLIP_COST)
    rec = RM.records(d["qpos"], d["rpos"], d["rev"], d["chain"], d["lk_offsets"], d["lk_ops"], d["first"], d["last"], d["q_lo"], d["q_hi"], d["e_q"], d["e_r"], d["e_clip"],
                     d["en_offsets"], d["en_ops"], KMER, 1)
    assert rec["valid"] == [1, 1] and rec["nm"] == [2, 2] and rec["qs"] == [0, 0] and rec["qe"] == [READ, READ]
    d["valid"] = arr(rec["valid"], u8)
    for f in "qs qe rs re qlen n_match n_block nm".split():
        d[f] = arr(rec[f], u32)
    d["rc_offsets"], d["rc_ops"] = arr(rec["offsets"], u64), arr(rec["ops"], u32)
    toff, ttext = RM.cigar_text(d["rc_offsets"], d["rc_ops"])
    d["tx_offsets"], d["tx_text"] = arr(toff, u64), text(ttext)
    df = DM.record_diffs(d["qtext"], d["rtext"], 0, d["rc_offsets"], d["rc_ops"], d["valid"], d["rev_row"], d["q_lo"], d["q_hi"], d["rs"], DM.CS)
    assert df["ok"] == [1, 1]
    d["df_ok"], d["df_offsets"], d["df_text"] = arr(df["ok"], u8), arr(df["offsets"], u64), text(df["text"])
    ooff, otext = OM.oriented_rows(d["qtext"], d["q_lo"], d["q_hi"], d["rev_row"], 1)
    d["or_offsets"], d["or_text"] = arr(ooff, u64), text(otext)
    return d


def spec(name, d, empty):
    """the shape of one call -> (arguments before `where`: arrays and integers; the outputs between `where` and the (out, cap, n) triple as
    expected arrays, the offsets last; the expected variable-length output; the outputs behind the triple).  empty: no rows."""
    z = (lambda a: a[:0]) if empty else (lambda a: a)
    e = (lambda a: a[:0]) if empty else (lambda a: a)
    offs = (lambda a: a[:1] * u64(0)) if empty else (lambda a: a)
    qt, rt = d["qtext"], d["rtext"]
    if name == "kh_chain_cigars":
        m = len(z(d["qpos"]))
        pre = [qt, len(qt), rt, len(rt), 0, z(d["qpos"]), z(d["rpos"]), z(d["rev"]), z(d["pred"]), z(d["chain"]), m, 0 if empty else 2, KMER, z(d["link"])]
        return pre, [offs(d["lk_offsets"])], d["lk_ops"], [e(d["c_ins"]), e(d["c_del"])]
    if name == "kh_chain_ends":
        nc = len(z(d["first"]))
        pre = [qt, len(qt), rt, len(rt), 0, d["qpos"], d["rpos"], d["rev"], len(d["qpos"]), z(d["first"]), z(d["last"]), z(d["q_lo"]), z(d["q_hi"]), nc, KMER, MAX_EDITS, CLIP_COST]
        return pre, [e(d["e_q"]), e(d["e_r"]), e(d["e_edits"]), e(d["e_clip"]), offs(d["en_offsets"])], d["en_ops"], []
    if name == "kh_chain_records":
        nc = len(z(d["first"]))
        pre = [d["qpos"], d["rpos"], d["rev"], d["chain"], len(d["qpos"]), d["lk_offsets"], d["lk_ops"], len(d["lk_ops"]), z(d["first"]), z(d["last"]), z(d["q_lo"]), z(d["q_hi"]),
               nc, z(d["e_q"]), z(d["e_r"]), z(d["e_clip"]), d["en_offsets"][:2 * nc + 1], z(d["en_ops"]), len(z(d["en_ops"])), KMER, 1]
        fixed = [e(d[f]) for f in "valid qs qe rs re qlen n_match n_block nm".split()] + [offs(d["rc_offsets"])]
        return pre, fixed, d["rc_ops"], []
    if name == "kh_cigar_text":
        rows = 0 if empty else len(d["rc_offsets"]) - 1
        return [d["rc_offsets"][:rows + 1], rows, d["rc_ops"], len(d["rc_ops"])], [offs(d["tx_offsets"])], d["tx_text"], []
    if name == "kh_record_diffs":
        rows = len(z(d["valid"]))
        pre = [qt, len(qt), rt, len(rt), 0, d["rc_offsets"][:rows + 1], d["rc_ops"], len(d["rc_ops"]), z(d["valid"]), z(d["rev_row"]), z(d["q_lo"]), z(d["q_hi"]), z(d["rs"]), rows, DM.CS]
        return pre, [e(d["df_ok"]), offs(d["df_offsets"])], d["df_text"], []
    assert name == "kh_oriented_rows"
    rows = len(z(d["q_lo"]))
    return [qt, len(qt), z(d["q_lo"]), z(d["q_hi"]), z(d["rev_row"]), rows, 1], [offs(d["or_offsets"])], d["or_text"], []


def sentinels(n, dt):
    return np.frombuffer(bytes([SENTINEL]) * (n * np.dtype(dt).itemsize), dtype=dt).copy()


def call(name, d, dev, cap, with_out=True, room=None, empty=False):
    """one call of the entry point over fresh sentinel-filled outputs -> (status, n, the outputs before the triple, the variable-length
    output of `room` elements (default: cap), the outputs behind the triple), everything on the host"""
    pre, fixed, var, post = spec(name, d, empty)
    mk = to_dev if dev else (lambda x: x)
    ptr = lambda x: (x.data_ptr() if dev else x.ctypes.data) if len(x) else None      # noqa: E731
    keep = [mk(a) if isinstance(a, np.ndarray) else a for a in pre]
    f_out, p_out = [mk(sentinels(len(a), a.dtype)) for a in fixed], [mk(sentinels(len(a), a.dtype)) for a in post]
    v_out = mk(sentinels(max(cap if room is None else room, 1), var.dtype))
    n = C.c_uint64(12345)
    st = getattr(K.lib(), name)(*(ptr(a) if not isinstance(a, int) else a for a in keep), K.KH_MEM_DEVICE if dev else K.KH_MEM_HOST, *(ptr(a) for a in f_out),
                                ptr(v_out) if with_out else None, cap, C.byref(n), *(ptr(a) for a in p_out), 0, None)
    if dev:
        torch.cuda.synchronize()
    host = lambda x, like: (x.cpu().numpy() if dev else x).view(like.dtype)      # noqa: E731
    return st, n.value, [host(x, a) for x, a in zip(f_out, fixed)], host(v_out, var), [host(x, a) for x, a in zip(p_out, post)]


def untouched(a):
    return (a.view(u8) == SENTINEL).all()


def same_fixed(name, d, got_fixed, got_post, empty=False):
    _, fixed, _, post = spec(name, d, empty)
    for i, (g, e) in enumerate(zip(got_fixed + got_post, fixed + post)):
        assert np.array_equal(g, e), (name, "output %d" % i, g, e)


def test_the_batch_is_what_it_claims(batch):
    d = batch
    for c in (0, 1):
        row = lambda off, ops, i: [(int(v) & 15, int(v) >> 4) for v in ops[int(off[i]):int(off[i + 1])]]      # noqa: E731
        assert row(d["lk_offsets"], d["lk_ops"], 3 * c) == [] and [o for o, _ in row(d["lk_offsets"], d["lk_ops"], 3 * c + 1)] == [CM.OP_EQ, CM.OP_X, CM.OP_EQ]
        assert CM.OP_I in [o for o, _ in row(d["lk_offsets"], d["lk_ops"], 3 * c + 2)]
        assert row(d["en_offsets"], d["en_ops"], 2 * c) == [(CM.OP_EQ, 2)] and row(d["en_offsets"], d["en_ops"], 2 * c + 1) == [(CM.OP_EQ, 1)]
    assert d["c_ins"].tolist() == [1, 1] and d["c_del"].tolist() == [0, 0]
    assert 8 <= len(d["lk_ops"]) + len(d["en_ops"]) <= 24 and len(d["rc_ops"]) == 10 and 20 <= len(d["tx_text"]) <= 60 and 10 <= len(d["df_text"]) <= 60
    assert len(d["or_text"]) == 2 * READ and d["or_text"][:READ].tobytes() == d["qtext"][:READ].tobytes() and d["or_text"][READ:].tobytes() != d["qtext"][READ:].tobytes()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ENTRIES)
def test_count_emit_short_roomy_and_empty(batch, name, dev):
    d = batch
    exp = spec(name, d, False)[2]
    total = len(exp)
    assert total >= 2
    # a. the count pass: a null output
    st, n, fixed, out, post = call(name, d, dev, 0, with_out=False)
    assert (st, n) == (K.KH_OK, total)
    same_fixed(name, d, fixed, post)
    # b. the exact capacity
    st, n, fixed, out, post = call(name, d, dev, total)
    assert (st, n) == (K.KH_OK, total)
    same_fixed(name, d, fixed, post)
    assert np.array_equal(out, exp), (name, out, exp)
    # c. one short: refused, the count and the offsets written, the output untouched
    st, n, fixed, out, post = call(name, d, dev, total - 1, room=total)
    assert (st, n) == (K.KH_ERR_INVALID, total)
    same_fixed(name, d, fixed, post)
    assert untouched(out), (name, out)
    # d. room to spare: the rows, then the sentinel
    st, n, fixed, out, post = call(name, d, dev, total + 5)
    assert (st, n) == (K.KH_OK, total)
    same_fixed(name, d, fixed, post)
    assert np.array_equal(out[:total], exp) and untouched(out[total:]), (name, out)
    # e. no rows
    st, n, fixed, out, post = call(name, d, dev, 4, empty=True)
    assert (st, n) == (K.KH_OK, 0)
    same_fixed(name, d, fixed, post, empty=True)
    assert fixed[-1].tolist() == [0] and untouched(out)
