"""Host time per call of the Python binding: three small calls with their input already on the device, where the kernels take
microseconds and what is left is the wrapper -- argument buffers, output allocation, stream lookup, the ctypes call.

    table.count           a 1-key tensor on a hashmap_robinhood_doubling
    kmers_from_sequence   a 64-byte text tensor
    index.find            a 1-key tensor on a KmerPositionIndex (two library calls: the offsets pass, then the positions)

Each figure is the median wall time of one call over --calls calls (default 1000), the stream synchronised once behind the batch, not
per call.  Prints one JSON line.  --root DIR imports kmerhash_amd from another checkout (built there), so that two trees can be run
in turn on one machine:

    python scripts/py_call_overhead.py                    # this tree
    python scripts/py_call_overhead.py --root ../parent   # the tree to compare with
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    import kmerhash_amd as kh
    from kmerhash_amd import kmers as KM
    from kmerhash_amd import workloads as W
    assert os.path.abspath(kh.__file__).startswith(os.path.abspath(a.root)), kh.__file__

    keys = W.distinct_u64(10_000, seed=3)
    table = kh.hashmap_robinhood_doubling(128, 0.35, 0.8)
    table.insert(keys, np.arange(len(keys), dtype=np.uint32))
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, 20_000)].copy()
    index = kh.KmerPositionIndex(k=21)
    index.build_sequences(text)
    one_key = torch.from_numpy(keys[:1].view(np.int64)).cuda()
    one_kmer = KM.kmers_from_sequence(torch.from_numpy(text[:21]).cuda(), 21)
    text64 = torch.from_numpy(text[:64]).cuda()
    calls = {"table.count": lambda: table.count(one_key),
             "kmers_from_sequence": lambda: KM.kmers_from_sequence(text64, 21),
             "index.find": lambda: index.find(one_kmer)}
    out = {"label": a.label or a.root, "calls": a.calls}
    for name, f in calls.items():
        for _ in range(100):
            f()
        torch.cuda.synchronize()
        t = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            f()
            t.append(time.perf_counter() - t0)
        torch.cuda.current_stream().synchronize()
        out[name + "_us"] = round(statistics.median(t) * 1e6, 2)
    table.close()
    index.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
