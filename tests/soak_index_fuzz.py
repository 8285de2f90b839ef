"""soak: random operation sequences over the two position indexes against the numpy model of the whole history (lives under tests/
because it uses the test models; not collected by pytest: run it by hand on the GPU box).  The sequences are those of
tests/index_seq_cases.py and the per-call check is that of tests/test_gpu_index_sequences.py, with seeds counting up and the eight
configs in turn.
usage: python tests/soak_index_fuzz.py [seconds] [first_seed] [config id]   -- prints the failing (config, seed, step, op) if anything
differs; seconds = 0 runs first_seed once (the replay of a failing sequence)"""
import sys
import time
import traceback

sys.path.insert(0, ".")
from tests.index_seq_cases import BY_ID, CONFIGS  # noqa: E402
from tests.test_gpu_index_sequences import run_sequence  # noqa: E402

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 3
configs = [BY_ID[sys.argv[3]]] if len(sys.argv) > 3 else list(CONFIGS)
t_end = time.time() + budget
first, runs = seed, 0
while True:
    for config in configs:
        t0 = time.time()
        try:
            run_sequence(config, seed)
        except Exception as e:                                    # (an AssertionError of the check carries config, seed, step and op itself)
            traceback.print_exc()
            print("FAIL config %s seed %d: %s" % (config.id, seed, str(e)[:400]), flush=True)
            sys.exit(1)
        runs += 1
        print("ok config %s seed %d  %.1f s" % (config.id, seed, time.time() - t0), flush=True)
    seed += 1
    if time.time() >= t_end:
        break
print("soak ok: %d sequences of 30 calls, seeds %d..%d, configs %s" % (runs, first, seed - 1, " ".join(c.id for c in configs)))
