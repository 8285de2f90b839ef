"""TEST HELPER (not collected): inputs of kh_sam_lines made to order.  lines(n, seed, ...): n lines over seven byte CSRs whose rows have
the lengths around the 8-byte word and the 64-lane step (0, 1, 7, 8, 9, 63, 64, 65, 300) in every text field, so that line starts and
piece starts fall on every residue mod 8; the numeric columns drawn from the extremes of their types; all kinds of RNEXT, RNAME -1,
every tag mask, and row indexes outside their CSR.  Everything is numpy in the dtypes the call takes."""
import numpy as np

LENS = [0, 1, 7, 8, 9, 63, 64, 65, 300]
UNSIGNED = [0, 9, 10, 99, 100, 2 ** 31 - 1, 2 ** 32 - 1]
SIGNED = [0, 9, 10, 99, 100, 2 ** 31 - 1, -1, -2 ** 31]
BYTES = [0, 9, 10, 99, 100, 255]
OUTSIDE = [-1, -7, -2 ** 31, 2 ** 31 - 1]      # and the CSR's own row count, added per CSR
CSRS = ("names", "tnames", "cigar", "seq", "qual", "md", "cs")
COLUMNS = ("name", "flag", "rname", "pos", "mapq", "cigar", "rnext", "pnext", "tlen", "seq", "qual", "tags", "nm", "tp", "cm", "s1", "s2", "md", "cs")
DTYPES = (np.int32, np.uint32, np.int32, np.uint32, np.uint8, np.int32, np.int32, np.uint32, np.int32, np.int32, np.int32, np.uint8, np.uint32, np.uint8, np.uint32,
          np.int32, np.int32, np.int32, np.int32)
ROW_OF = dict(name="names", rname="tnames", cigar="cigar", rnext="tnames", seq="seq", qual="qual", md="md", cs="cs")


def csr(rng, n_rows, phase, alphabet):
    lens = [LENS[(r + phase) % len(LENS)] for r in range(n_rows)]
    text = np.frombuffer(alphabet, dtype=np.uint8)[rng.randint(0, len(alphabet), size=sum(lens))].copy()
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), text


def lines(n, seed=1, absent=(), n_rows=23):
    """-> (csrs: {name: (offsets, text) or None}, cols: {column: array})"""
    rng = np.random.RandomState(seed)
    alphabets = dict(names=b"readRD_/.0123456789", tnames=b"chrXY_12", cigar=b"0123456789MIDS=X", seq=b"ACGTNacgt", qual=bytes(range(33, 127)), md=b"0123456789ACGT^",
                     cs=b":*+-acgt0123456789")
    csrs = {x: None if x in absent else csr(rng, n_rows + k, k, alphabets[x]) for k, x in enumerate(CSRS)}
    cols = {}
    for c, dt in zip(COLUMNS, DTYPES):
        if c in ROW_OF:
            rows = n_rows + CSRS.index(ROW_OF[c])
            pool = list(range(rows)) * 3 + OUTSIDE + [rows] + ([-2] * 4 if c == "rnext" else [])
        elif c == "tags":
            pool = list(range(16)) + [0xF0 | 5]
        elif c == "tp":
            pool = [ord("P"), ord("S"), ord("R")]
        else:
            pool = BYTES if dt == np.uint8 else SIGNED if dt == np.int32 else UNSIGNED
        cols[c] = np.array([pool[j] for j in rng.randint(0, len(pool), size=n)], dtype=np.int64).astype(dt)
    for i in range(min(n, 16)):      # every mask is there whatever the draw
        cols["tags"][i] = i
    return csrs, cols
