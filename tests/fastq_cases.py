"""TEST HELPER (not collected): FASTQ texts for kh_fastq_records / read_fastq and row sets for kh_pack_rows: the smallest shapes at
which the kernels can go wrong.  The line kernels work on tiles of KH_CMP_TILE = 2048 bytes, a lane on 8 of them; the pack kernel
moves 8-byte words aligned to the destination, 64 per wave step (512 bytes).

CASES[name] = Case(text, good, recs): good = every record is well-formed, there are no tail lines and no '\\r' (then the k-mers of the
packed reads must be those of kh_kmers_from_fastq); recs = the (name line, sequence, plus line, quality) tuples the text was written from."""
import collections

import numpy as np

TILE = 2048
Case = collections.namedtuple("Case", "text good recs")


def bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))


def quals(rng, n):
    return bytes(rng.randint(35, 74, size=n).astype(np.uint8))      # '#' .. 'I': neither '@' nor '+' nor a blank


def rec(rng, name, n, plus=b"+"):
    return (b"@" + name, bases(rng, n), plus, quals(rng, n))


def write(recs, eol=b"\n", last_eol=True):
    t = eol.join(l for r in recs for l in r)
    return t + eol if last_eol and recs else t


def _cases():
    rng = np.random.RandomState(5)
    C = {}

    def add(name, recs, good=True, **kw):
        C[name] = Case(write(recs, **kw), good, recs)

    three = lambda: [rec(rng, b"r%d" % i, 20 + 7 * i) for i in range(3)]      # noqa: E731
    add("single", [rec(rng, b"only", 33)])
    # the newline that ends the first header is the last byte of tile 0 / the first byte of tile 1
    add("newline_last_of_tile", [rec(rng, b"a " + b"x" * (TILE - 1 - 3), 40)] + three())
    add("newline_first_of_tile", [rec(rng, b"a " + b"x" * (TILE - 3), 40)] + three())
    assert C["newline_last_of_tile"].text[TILE - 1] == 10 and C["newline_first_of_tile"].text[TILE] == 10
    # a record over three tiles and more (5000 bases and 5000 qualities), one over two
    add("straddle", [rec(rng, b"s0", 100), rec(rng, b"long", 5000), rec(rng, b"mid", 1200), rec(rng, b"s1", 9)])
    # ~3000 short records: the line numbers of a tile come from the scanned sums of many tiles
    add("many", [rec(rng, b"m%d/%d" % (i // 2, 1 + i % 2), 1 + (i * 7) % 23) for i in range(3000)])
    add("no_trailing_newline", three(), last_eol=False)
    add("crlf", three(), good=False, eol=b"\r\n")
    add("crlf_no_trailing_newline", three(), good=False, eol=b"\r\n", last_eol=False)
    for k in (1, 2, 3):      # a record cut short behind whole ones
        base = three()
        C["tail%d" % k] = Case(write(base) + b"\n".join(rec(rng, b"cut", 12)[:k]) + b"\n", False, base)
    base = three()
    C["blank_trailing_line"] = Case(write(base) + b"\n", True, base)
    C["blank_trailing_crlf"] = Case(write(base, eol=b"\r\n") + b"\r\n", False, base)
    add("empty_sequence", [rec(rng, b"e0", 10), (b"@none", b"", b"+", b""), rec(rng, b"e2", 10)])
    q = quals(rng, 30)
    add("quality_starts_with_at", [rec(rng, b"q0", 12), (b"@q1", bases(rng, 30), b"+", b"@" + q[1:]), rec(rng, b"q2", 12)])
    add("quality_starts_with_plus", [rec(rng, b"q0", 12), (b"@q1", bases(rng, 30), b"+", b"+" + q[1:]), rec(rng, b"q2", 12)])
    add("quality_of_acgt", [(b"@q%d" % i, bases(rng, 40), b"+", bases(rng, 40)) for i in range(3)])
    add("plus_line_repeats_name", [rec(rng, b"p0", 15, plus=b"+p0"), rec(rng, b"p1", 15)])
    add("names", [rec(rng, b"with a comment", 11), rec(rng, b"tab\tBC:Z:ACGT", 11), rec(rng, b"x", 11), rec(rng, b"frag7/1", 11), rec(rng, b"frag7/2", 11),
                  rec(rng, b"/1", 11), rec(rng, b"a/3", 11), rec(rng, b"/2 c", 11)])
    add("empty_name", [rec(rng, b"n0", 14), rec(rng, b"", 14), rec(rng, b" only a comment", 14), rec(rng, b"n3", 14)], good=False)
    r = rec(rng, b"bad", 16)
    add("missing_at", [rec(rng, b"g0", 16), (r[0][1:],) + r[1:], rec(rng, b"g2", 16)], good=False)
    add("missing_plus", [rec(rng, b"g0", 16), (r[0], r[1], b"-", r[3]), (r[0], r[1], b"", r[3]), rec(rng, b"g2", 16)], good=False)
    add("length_mismatch", [rec(rng, b"g0", 16), (r[0], r[1], r[2], r[3][:-1]), (r[0], r[1][:-2], r[2], r[3]), rec(rng, b"g2", 16)], good=False)
    add("empty_header_line", [rec(rng, b"g0", 16), (b"",) + r[1:], rec(rng, b"g2", 16)], good=False)
    C["empty"] = Case(b"", True, [])
    C["only_newlines"] = Case(b"\n" * 9, False, [])
    C["one_newline"] = Case(b"\n", True, [])
    C["no_newline_at_all"] = Case(b"@abc", False, [])
    return C


CASES = _cases()
ALIGN_CASES = ("many", "straddle", "crlf_no_trailing_newline")      # viewed at byte offsets 1..7 of their buffer


def pair_texts(n=60, seed=9, slash=True):
    """two texts of n mates each, names frag<p>/1 and frag<p>/2 (or the same name twice), lengths that differ between the mates"""
    rng = np.random.RandomState(seed)
    one = [rec(rng, b"frag%d%s c" % (p, b"/1" if slash else b""), 30 + p % 11) for p in range(n)]
    two = [rec(rng, b"frag%d%s" % (p, b"/2" if slash else b""), 25 + p % 7) for p in range(n)]
    return write(one), write(two), one, two


# ---- kh_pack_rows
ROW_LENGTHS = (0, 1, 7, 8, 9, 511, 512, 513, 1500)


def pack_case(seed=3):
    """rows of every length of ROW_LENGTHS, each at every source / destination alignment pair mod 8 -> (text, lo, hi, dst, out_len):
    destinations disjoint with room for a separator, gaps between them that no row covers"""
    rng = np.random.RandomState(seed)
    text = rng.randint(1, 255, size=4096 + 8).astype(np.uint8)
    lo, hi, dst, at = [], [], [], 3
    for length in ROW_LENGTHS:
        for sa in range(8):
            for da in range(8):
                a = 8 * int(rng.randint(0, (len(text) - length - 8) // 8)) + sa
                at += (da - at) % 8
                lo.append(a); hi.append(a + length); dst.append(at)      # noqa: E702
                at += length + 1 + int(rng.randint(0, 3))
    return text, np.array(lo, dtype=np.uint32), np.array(hi, dtype=np.uint32), np.array(dst, dtype=np.uint64), at + 5
