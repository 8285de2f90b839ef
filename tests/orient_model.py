"""TEST HELPER (not collected): kh_oriented_rows on Python integers -- the definition of include/kmerhash_amd.h as loops."""
COMP = {ord(a): ord(b) for a, b in zip("ATCGatcg", "TAGCtagc")}


def oriented_rows(text, lo, hi, rev, complement):
    """-> (offsets as a list, text as bytes)"""
    n, offs, parts = len(text), [0], []
    for c in range(len(lo)):
        a, b = min(int(lo[c]), n), min(int(hi[c]), n)
        row = bytes(text[a:b]) if b > a else b""
        if int(rev[c]) & 1:
            row = bytes((COMP.get(x, x) if complement else x) for x in row[::-1])
        parts.append(row)
        offs.append(offs[-1] + len(row))
    return offs, b"".join(parts)
