"""GPU: the mapper's text stages on query and reference texts that start at odd byte offsets of their allocations.  ked_load_up and
ked_load_down (kh_kernels_edits.h) issue 8-byte loads at arbitrary text + pos for kh_chain_edits, kh_chain_cigars and kh_chain_ends;
kh_record_diffs and the source side of kh_oriented_rows read the same texts.  They are written for any alignment; the other tests give
them aligned bases only.

The batch is that of tests/test_gpu_emit_tail.py -- reads of 40 bases against a reference of 200, k = 11, each read one chain of three
anchors with a substitution between the first two and an inserted base between the last two -- plus a read whose first seed starts at
its first byte (the first read of the query text), one whose last seed ends at its last byte (the last read), one that faces reference
position 0 and one that ends at the last reference byte: the short paths of both loaders at both ends of both texts.  The bytes in front
of and behind each view are bases that would lengthen a match if they were read.  Expected: the stage models fed with each other's
results, as tests/test_gpu_emit_tail.py composes them."""
import os
import random
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kmerhash_amd import kmers as KM  # noqa: E402
from kmerhash_amd import sam as SAM  # noqa: E402
import cigar_model as CM  # noqa: E402
import diffs_model as DM  # noqa: E402
import edits_model as EDM  # noqa: E402
import ends_model as ENM  # noqa: E402
import orient_model as OM  # noqa: E402
import records_model as RM  # noqa: E402
from ends_cases import revcomp  # noqa: E402
from stream_checks import to_dev  # noqa: E402

KMER, READ, NREF, MAX_EDITS, CLIP_COST = 11, 40, 200, 31, 4
OFFSET_PAIRS = ((1, 0), (0, 1), (3, 5), (7, 7), (8, 9))          # (query text, reference text)
u8, u32, i32, u64 = np.uint8, np.uint32, np.int32, np.uint64
STD = ((2, 2), (15, 15), (28, 27))                                 # seeds of the emit-tail reads: (read offset, offset in the faced stretch)
END = ((2, 2), (15, 15), (29, 28))                                 # the last seed ends at the last byte of the read
# (reference start of the 39 bases the read faces, strand, seeds), in query-text order
READS = ((80, 0, ((0, 0), (15, 15), (28, 27))),                    # first seed at read offset 0, and at byte 0 of the query text
         (50, 0, STD), (120, 1, STD),                              # the two reads of the emit-tail batch
         (0, 1, END),                                              # its last seed lies at reference position 0 (reverse strand)
         (NREF - (READ - 1), 0, END),                              # its last seed ends at the last reference byte
         (20, 1, END))                                             # the last read: its last seed ends at the last byte of the query text


def arr(x, dt):
    return np.array(x, dtype=dt)


def text(b):
    return np.frombuffer(bytes(b), dtype=u8).copy()


@pytest.fixture(scope="module")
def batch():
    """the inputs and the models' outputs of every stage -> dict"""
    rng = random.Random(2)
    ref = bytes(rng.choice(b"ACGT") for _ in range(NREF))
    other = lambda b, *more: next(c for c in b"ACGT" if c != b and c not in more)      # noqa: E731
    reads, qpos, rpos, rev = [], [], [], []
    for r0, rv, seeds in READS:
        s = revcomp(ref[r0:r0 + READ - 1]) if rv else ref[r0:r0 + READ - 1]           # the 39 reference bases the read faces, in read order
        read = s[:13] + bytes([other(s[13])]) + s[14:26] + bytes([other(s[25], s[26])]) + s[26:]
        assert len(read) == READ
        for q, j in seeds:
            assert read[q:q + KMER] == s[j:j + KMER]
            qpos.append(len(reads) * READ + q); rpos.append(r0 + (READ - 1 - KMER - j if rv else j)); rev.append(rv)
        reads.append(read)
    nc = len(READS)
    d = {"ref": ref, "qtext": text(b"".join(reads)), "rtext": text(ref), "qpos": arr(qpos, u32), "rpos": arr(rpos, u32), "rev": arr(rev, u8),
         "pred": arr([-1 if i % 3 == 0 else i - 1 for i in range(3 * nc)], i32), "chain": arr([i // 3 for i in range(3 * nc)], i32),
         "first": arr([3 * c for c in range(nc)], u32), "last": arr([3 * c + 2 for c in range(nc)], u32),
         "q_lo": arr([READ * c for c in range(nc)], u32), "q_hi": arr([READ * (c + 1) for c in range(nc)], u32), "rev_row": arr([r[1] for r in READS], u8)}
    # the ends the issue asks for are really there
    assert d["qpos"][0] == 0 and d["qpos"][-1] + KMER == len(d["qtext"]) and d["rpos"].min() == 0 and (d["rpos"] + KMER).max() == NREF
    anchors = [d[f] for f in ("qtext", "rtext", "qpos", "rpos", "rev")]
    link, edits, over = EDM.chain_edits_model(*anchors, d["pred"], d["chain"], nc, KMER, 0, MAX_EDITS)
    d["link"], d["edits"], d["over"] = np.asarray(link, dtype=i32), np.asarray(edits, dtype=u32), np.asarray(over, dtype=u32)
    assert d["link"].tolist() == [-1, 1, 1] * nc
    d["lk_offsets"], d["lk_ops"], d["c_ins"], d["c_del"] = CM.chain_cigars_model(*anchors, d["pred"], d["chain"], nc, KMER, d["link"])
    d["e_q"], d["e_r"], d["e_edits"], d["e_clip"], d["en_offsets"], d["en_ops"] = ENM.chain_ends_model(*anchors, d["first"], d["last"], d["q_lo"], d["q_hi"], KMER, 0,
                                                                                                    MAX_EDITS, CLIP_COST)
    rec = RM.records(d["qpos"], d["rpos"], d["rev"], d["chain"], d["lk_offsets"], d["lk_ops"], d["first"], d["last"], d["q_lo"], d["q_hi"], d["e_q"], d["e_r"], d["e_clip"],
                     d["en_offsets"], d["en_ops"], KMER, 1)
    assert rec["valid"] == [1] * nc
    d["valid"] = arr(rec["valid"], u8)
    for f in "qs qe rs re qlen n_match n_block nm".split():
        d[f] = arr(rec[f], u32)
    d["rc_offsets"], d["rc_ops"] = arr(rec["offsets"], u64), arr(rec["ops"], u32)
    for kind, name in ((DM.CS, "cs"), (DM.MD, "md")):
        df = DM.record_diffs(d["qtext"], d["rtext"], 0, d["rc_offsets"], d["rc_ops"], d["valid"], d["rev_row"], d["q_lo"], d["q_hi"], d["rs"], kind)
        assert df["ok"] == [1] * nc
        d[name] = (arr(df["ok"], u8), arr(df["offsets"], u64), text(df["text"]))
    return d


def view_of(t, o, front, back):
    """the bytes of t as a device view o bytes past a 16-byte boundary, `front` ending right in front of it and `back` right behind"""
    buf = to_dev(np.concatenate([text(front[len(front) - o:]), t, text(back)]))
    v = buf[o:o + len(t)]
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == o and v.numel() == len(t)
    return v


def views(d, oq, orf):
    """the two texts at their offsets, wrapped in the bases that would continue a match across each end"""
    ref = d["ref"]
    r0_first, r0_last = READS[0][0], READS[-1][0]
    assert READS[0][1] == 0 and READS[-1][1] == 1 and r0_first >= 16 and r0_last >= 16
    q_front = ref[r0_first - 16:r0_first]                              # read 0 is forward: what the reference holds in front of it
    q_back = revcomp(ref[r0_last - 16:r0_last])                        # the last read is reverse: the reference goes on downwards
    qt = d["qtext"]
    c_end, d_end = READ * 4, READ * 5                                   # the reads at reference position 0 (reverse) and at its end (forward)
    assert READS[3][:2] == (0, 1) and READS[4][:2] == (NREF - (READ - 1), 0)
    r_front = b"ACGTACGTACGTACG" + revcomp(bytes(qt[c_end:c_end + 1]))  # below position 0: the complement of the query byte behind that read
    r_back = bytes(qt[d_end:d_end + 1]) + b"ACGTACGTACGTACG"           # past the end: the query byte behind that read
    return view_of(qt, oq, q_front, q_back), view_of(d["rtext"], orf, r_front, r_back)


def host(x, dt):
    return x.cpu().numpy().view(dt)


@pytest.mark.parametrize("oq,orf", OFFSET_PAIRS)
def test_text_stages_on_misaligned_texts(batch, oq, orf):
    d = batch
    nc = len(READS)
    qt, rt = views(d, oq, orf)
    dv = {f: to_dev(d[f]) for f in "qpos rpos rev pred chain first last q_lo q_hi rev_row link".split()}
    anchors = (dv["qpos"], dv["rpos"], dv["rev"])
    # chain_edits
    e = KM.chain_edits(qt, rt, *anchors, dv["pred"], dv["chain"], nc, KMER, 0, MAX_EDITS)
    assert np.array_equal(host(e.link, i32), d["link"]) and np.array_equal(host(e.edits, u32), d["edits"]) and np.array_equal(host(e.over, u32), d["over"])
    # chain_cigars over the model's link array
    c = KM.chain_cigars(qt, rt, *anchors, dv["pred"], dv["chain"], nc, KMER, dv["link"], 0)
    assert np.array_equal(host(c.offsets, u64), d["lk_offsets"]) and np.array_equal(host(c.ops, u32), d["lk_ops"])
    assert np.array_equal(host(c.ins, u32), d["c_ins"]) and np.array_equal(host(c.dels, u32), d["c_del"])
    # chain_ends
    n = KM.chain_ends(qt, rt, *anchors, dv["first"], dv["last"], dv["q_lo"], dv["q_hi"], KMER, 0, MAX_EDITS, CLIP_COST)
    for got, f, dt in ((n.q, "e_q", u32), (n.r, "e_r", u32), (n.edits, "e_edits", None), (n.clip, "e_clip", None), (n.offsets, "en_offsets", u64), (n.ops, "en_ops", u32)):
        exp = np.asarray(d[f])
        assert np.array_equal(host(got, dt or exp.dtype), exp), f
    # record_diffs, cs and MD, over the model's records
    rec = KM.ChainRecords(*(to_dev(d[f]) for f in "valid qs qe rs re qlen n_match n_block nm rc_offsets rc_ops".split()))
    for kind in ("cs", "md"):
        ok, offs, txt = d[kind]
        g = SAM.record_diffs(qt, rt, rec, dv["rev_row"], dv["q_lo"], dv["q_hi"], kind, 0)
        assert np.array_equal(host(g.ok, u8), ok) and np.array_equal(host(g.offsets, u64), offs) and host(g.text, u8).tobytes() == txt.tobytes(), kind
    # oriented_rows: both strands, with and without complement
    for rv in (d["rev_row"], 1 - d["rev_row"]):
        for comp in (1, 0):
            eoff, etext = OM.oriented_rows(d["qtext"], d["q_lo"], d["q_hi"], rv, comp)
            goff, gtext = SAM.oriented_rows(qt, dv["q_lo"], dv["q_hi"], to_dev(rv.astype(u8)), bool(comp))
            assert np.array_equal(host(goff, u64), arr(eoff, u64)) and host(gtext, u8).tobytes() == bytes(etext)
