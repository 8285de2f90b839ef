#!/usr/bin/env python3
"""FASTA and FASTQ in, SAM out: the read mapper as one command.

  python benchmark/read_mapper.py ref.fa reads_1.fq [reads_2.fq] -o out.sam [-k 15] [-w 10] [--device 0]

Steps: kmerhash_amd.Targets.from_fasta over the reference; a stranded (w,k)-minimizer position index built from its text; the FASTQ
text uploaded as it is and read on the device (ix.map_fastq: read_fastq, then map; with a second file ix.map_fastq_pairs, the two files
interleaved and a closing /1 or /2 dropped from the names); write_sam_bytes, which assembles the lines on the device.  No read, quality
string or name passes through a Python loop.  Paired input is written without mate rescue: write_sam_bytes takes no MateRescue.
Prints the triple write_sam_bytes returns.  Informational driver; the contract benchmark is ../bench.py."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse(argv):
    ap = argparse.ArgumentParser(description="map FASTQ reads to a FASTA reference on the GPU and write SAM")
    ap.add_argument("ref")
    ap.add_argument("reads", nargs="+", help="one FASTQ file, or the two files of a paired run")
    ap.add_argument("-o", "--out", required=True)
    ap.add_argument("-k", type=int, default=15)
    ap.add_argument("-w", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if len(a.reads) > 2:
        ap.error("at most two FASTQ files")
    return a


def main(argv=None):
    a = parse(argv)
    import torch

    import kmerhash_amd as kh
    dev = torch.device("cuda", a.device)
    up = lambda path: torch.from_numpy(np.fromfile(path, dtype=np.uint8)).to(dev)      # noqa: E731
    T = kh.Targets.from_fasta(np.fromfile(a.ref, dtype=np.uint8))
    ref = torch.from_numpy(T.text).to(dev)
    ix = kh.KmerPositionIndex(k=a.k, w=a.w, stranded=True, device=a.device)
    try:
        with torch.cuda.device(dev):
            ix.build_sequences(ref)
            texts = [up(p) for p in a.reads]
            if len(texts) == 2:
                mp, pairs, reads = ix.map_fastq_pairs(texts[0], ref, texts[1], targets=T)
            else:
                (mp, reads), pairs = ix.map_fastq(texts[0], ref, targets=T), None
            with open(a.out, "wb") as fh:
                done = kh.write_sam_bytes(fh, mp, reads.seq, ref, reads.names, reads.read_starts, reads.read_ends, qual=reads.qual, targets=T, pairs=pairs, device=a.device)
    finally:
        ix.close()
    print("%d alignment lines, %d rows skipped, %d unmapped reads -> %s" % (tuple(done) + (a.out,)))
    return done


if __name__ == "__main__":
    main(sys.argv[1:])
