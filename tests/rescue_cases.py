"""TEST HELPER (not collected): named requests of kh_mate_rescue with outputs written by hand from the definition in
include/kmerhash_amd.h.  A case: (name, qtext, rtext, ref_base, max_edits, (q_lo, q_hi, w_lo, w_hi, rev), (edits, rs, re, span, CIGAR)).
The CIGAR is in reference order; rs / re / the window are global coordinates."""

REF = b"GGGGACGTTGCACCCC"                    # ACGTTGCA at [4, 12)
DEL = b"TTTTACGTACGGTCATTTT"                 # ACGTACGGTCA at [4, 15)

CASES = [
    # the mate as it stands, exact: one end column attains 0
    ("exact forward", b"ACGTTGCA", REF, 0, 31, (0, 8, 0, 16, 0), (0, 4, 12, 0, "8=")),
    # the reverse complement of the same fragment, expected on the reverse strand: R is ACGTTGCA again
    ("exact reverse", b"TGCAACGT", REF, 0, 31, (0, 8, 0, 16, 1), (0, 4, 12, 0, "8=")),
    # the mate lies behind other bytes of the query text, the window is cut to the fragment
    ("offsets and a tight window", b"NNNACGTTGCAN", REF, 0, 31, (3, 11, 4, 12, 0), (0, 4, 12, 0, "8=")),
    # global coordinates: the text covers [100, 116)
    ("ref_base", b"ACGTTGCA", REF, 100, 31, (0, 8, 100, 116, 0), (0, 104, 112, 0, "8=")),
    # one substitution: ending a column earlier or later costs 2
    ("substitution", b"ACGTAGCA", REF, 0, 31, (0, 8, 0, 16, 0), (1, 4, 12, 0, "4=1X3=")),
    ("substitution, max_edits 0", b"ACGTAGCA", REF, 0, 0, (0, 8, 0, 16, 0), (-2, 0, 0, 0, "")),
    # the mate lacks one G of the reference's GG: found from the end, the gap takes the first G in reference order
    ("deletion", b"ACGTACGTCA", DEL, 0, 31, (0, 10, 0, 19, 0), (1, 4, 15, 0, "6=1D4=")),
    # an N matches nothing, not even an N
    ("N facing N", b"ACNT", b"GGACNTGG", 0, 31, (0, 4, 0, 8, 0), (1, 2, 6, 0, "2=1X1=")),
    # the tie rule: every column from m on attains 0; e is the first, span reaches the last
    ("homopolymer", b"AAAA", b"AAAAAAAAAA", 0, 31, (0, 4, 0, 10, 0), (0, 0, 4, 6, "4=")),
    # an empty window: column 0 holds D[m][0] = m, the row is m insertions and the interval is empty
    ("empty window", b"AC", REF, 0, 31, (0, 2, 5, 5, 0), (2, 5, 5, 0, "2I")),
    ("empty window, max_edits 1", b"AC", REF, 0, 1, (0, 2, 5, 5, 0), (-2, 0, 0, 0, "")),
    # not looked at
    ("no bases", b"ACGT", REF, 0, 31, (2, 2, 0, 16, 0), (-1, 0, 0, 0, "")),
    ("mate beyond the query text", b"ACGT", REF, 0, 31, (0, 5, 0, 16, 0), (-1, 0, 0, 0, "")),
    ("window beyond the reference text", b"ACGT", REF, 0, 31, (0, 4, 0, 17, 0), (-1, 0, 0, 0, "")),
    ("window before ref_base", b"ACGT", REF, 100, 31, (0, 4, 99, 110, 0), (-1, 0, 0, 0, "")),
    ("window back to front", b"ACGT", REF, 0, 31, (0, 4, 9, 8, 0), (-1, 0, 0, 0, "")),
]
