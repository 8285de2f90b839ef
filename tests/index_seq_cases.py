"""TEST HELPER (not collected): random operation sequences over the two position indexes as plain data.  draw_sequence(config, seed)
yields the 30 calls of one sequence -- op name, numpy arguments, host or device input, the query batch to look up afterwards --, drawn
from a PairBag of its own and never from an index, so the same sequence replays on the CPU alone (tests/test_index_seq_cases.py), on
the GPU (tests/test_gpu_index_sequences.py) and in the hand-run soak (tests/soak_index_fuzz.py).  FIXED puts every operation at least
once on a loaded index; the other steps are drawn.  model_apply() is the one statement of what a call does to the bag."""
import collections

import numpy as np

from tests.index_seq_model import PairBag, isin_rows, key_rows, text_pairs
from tests.minimizer_model import HASH_IDS

T = 4096                                        # kmerhash_amd.index.SORT_TILE, restated: this file imports nothing of the library
STEPS = 30
SIZES = (0, 1, 7, 300, 4097, 20000)
UNIVERSE = 2000
HOT = 1500                                      # pairs the hot key gets in each of its six appends
HASHES = ("farm", "murmur3avx64")
SEEDS = (1, 2)

Config = collections.namedtuple("Config", "id wide k stranded w s forms")
CONFIGS = (
    Config("n-pairs", False, 21, False, None, None, ("pairs",)),
    Config("n-text", False, 15, False, None, None, ("sequences", "fastq", "pairs")),
    Config("n-strand", False, 15, True, None, None, ("sequences", "fastq", "pairs")),
    Config("n-min", False, 15, False, 5, None, ("sequences", "pairs")),
    Config("n-sync-strand", False, 15, True, None, 11, ("sequences", "fastq")),
    Config("w-pairs", True, 40, False, None, None, ("pairs",)),
    Config("w-strand", True, 35, True, None, None, ("sequences", "fastq", "pairs")),
    Config("w-sync", True, 35, False, None, 25, ("sequences", "pairs")),
)
BY_ID = {c.id: c for c in CONFIGS}

# step -> what the call is; resolved per config in draw_sequence (a config without pair forms loads and feeds its hot key through text,
# one without FASTQ draws step 11).  Steps that are not listed are drawn.
FIXED = {0: "build_big", 1: "append_big", 2: "hot", 3: "erase", 4: "hot", 5: "counts_one", 6: "hot", 7: "text_run", 8: "hot", 9: "counts_none",
         10: "hot", 11: "append_fastq", 12: "hot", 13: "counts_empty", 14: "counts_hot", 15: "drop_above", 16: "append_big", 17: "erase_all",
         18: "append_some", 19: "clear", 20: "build_a", 22: "clear", 23: "build_b"}
PROTECTED_UNTIL = 14                            # before this step nothing drawn may erase the hot key: its segment grows by appends alone

BUILDS = {"pairs": "build", "sequences": "build_sequences", "fastq": "build_fastq"}
APPENDS = {"pairs": "append", "sequences": "append_sequences", "fastq": "append_fastq"}


def hash_of(config, seed):
    return HASHES[(CONFIGS.index(config) + int(seed)) % 2]


def ops_of(config):
    return {"erase", "erase_counts", "drop_above", "clear"} | {BUILDS[f] for f in config.forms} | {APPENDS[f] for f in config.forms}


def words_of(config):
    return 2 if config.wide else 1


def pairs_of_call(config, call):
    """the (keys, stored positions) a text call adds"""
    return text_pairs(call["text"], config.k, True, call["op"].endswith("fastq"), call.get("pos_base", 0), config.stranded, config.w, config.s,
                      config.wide)


def batch_of_call(config, call):
    """the (keys, positions) of any build / append call, pair form or text form"""
    return (key_rows(call["keys"], words_of(config)), call["pos"]) if call["op"] in ("build", "append") else pairs_of_call(config, call)


def model_apply(bag, config, call):
    """does the call to the bag -> what the index must return"""
    op = call["op"]
    if op in ("build", "append"):
        return bag.append(call["keys"], call["pos"])
    if op in ("build_sequences", "build_fastq", "append_sequences", "append_fastq"):
        bag.append(*pairs_of_call(config, call))
        return bag.total()
    if op == "erase":
        return bag.erase(call["keys"])
    if op == "erase_counts":
        return bag.erase_counts(call["lo"], call["hi"])
    if op == "drop_above":
        return bag.drop_above(call["max_occ"])
    assert op == "clear", op
    return bag.clear()


def home_bits(keys, hash_name):
    """the low 16 bits of the table's hash (seed 43, the indexes' default) of 16-byte keys, by the CPU oracle: equal bits = the same home
    bucket at every capacity up to 65536"""
    from oracle import oracle_py as O
    return O.hash16_batch(HASH_IDS[hash_name], 43, key_rows(keys, 2)) & np.uint64(0xFFFF)


def sibling_keys(rng, hash_name, n=12):
    """n 16-byte keys that share w0 AND the home bucket and differ in w1 only: a probe that compares w0 alone takes one for another"""
    w0 = np.uint64(rng.integers(1, 1 << 62))
    cand = np.stack([np.full(1 << 20, w0, dtype=np.uint64), rng.integers(1, 1 << 62, 1 << 20, dtype=np.uint64)], axis=1)
    h = home_bits(cand, hash_name)
    vals, counts = np.unique(h, return_counts=True)
    rows = np.unique(cand[h == vals[np.argmax(counts >= n)]], axis=0)[:n]
    assert len(rows) == n
    return rows


# ---- the text pool --------------------------------------------------------------------------------------------------------------------
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
NL = np.frombuffer(b"\n", dtype=np.uint8)


def _bases(rng, n):
    return BASES[rng.integers(0, 4, n)].copy()


def make_pool(rng, k):
    """pieces of 500 to 3000 bases with N, lower case and a newline inside, one shorter than k, a run of 6000 A (one k-mer with more than
    SORT_TILE positions from a single call), a run of C for a hot key fed through text, and whole FASTQ records"""
    p0 = _bases(rng, 3000)
    p0[400:430] |= 0x20
    p0[900] = p0[1500] = p0[1501] = ord("N")
    p0[2200] = 10
    p1 = _bases(rng, 1500)
    p1[100:600] = p0[1600:2100]                                   # k-mers shared between pieces
    p2 = _bases(rng, 500)
    p2[250] = ord("n")
    short = _bases(rng, k - 3)
    run = np.concatenate([np.full(6000, ord("A"), dtype=np.uint8), _bases(rng, 1000)])
    hot = np.full(HOT + k - 1, ord("C"), dtype=np.uint8)
    qual = np.frombuffer(b"ACGTIF#5", dtype=np.uint8)
    records = []
    for r in range(16):
        ln = int(rng.integers(k + 5, 150))
        o = int(rng.integers(0, 1400 - ln)) if r % 2 else int(rng.integers(1600, 2100 - ln))
        seq = p0[o:o + ln].copy() if r % 2 == 0 else _bases(rng, ln)
        if r == 5:
            seq[ln // 2] = ord("N")
        records.append(np.concatenate([np.frombuffer(b"@r%d\n" % r, dtype=np.uint8), seq, np.frombuffer(b"\n+\n", dtype=np.uint8),
                                       qual[rng.integers(0, len(qual), ln)], NL]))
    return {"pieces": [p0, p1, p2], "short": short, "run": run, "hot": hot, "records": records}


def _join(parts):
    out = []
    for i, p in enumerate(parts):
        out += [NL, p] if i else [p]
    return np.ascontiguousarray(np.concatenate(out))


# ---- one sequence -----------------------------------------------------------------------------------------------------------------------
def draw_sequence(config, seed):
    """yields STEPS dicts: step, kind (the FIXED entry or "drawn"), op, device, the op's arguments (keys / pos, text / pos_base, lo / hi,
    max_occ), queries (the batch to look up after the call), qtext (every fifth step of a text config: a query text) and homopolymer
    (a text call whose text holds one of the two runs).  The caller does each call to its own PairBag with model_apply()."""
    words = words_of(config)
    rng = np.random.default_rng([CONFIGS.index(config), int(seed)])
    bag = PairBag(words)
    has = lambda f: f in config.forms                                       # noqa: E731
    pool = make_pool(rng, config.k) if has("sequences") else None
    top = 1 << (31 if config.stranded else 32)

    # the key universe: random keys (for wide keys every fourth shares w0 with the one before it) and, where there is text, some of its k-mers
    uni = np.unique(rng.integers(1, 1 << 62, (UNIVERSE + 200, words), dtype=np.uint64), axis=0)
    uni = rng.permutation(uni)[:UNIVERSE]
    siblings = np.zeros((0, words), dtype=np.uint64)
    if words == 2:
        uni[3::4, 0] = uni[2::4, 0]
        # eight keys of one w0 and one home bucket: four come with the first load, four with the second; four more are never inserted
        siblings = sibling_keys(rng, hash_of(config, seed))
        half = (len(uni) - 1) // 2
        uni[1:5], uni[half + 1: half + 5] = siblings[:4], siblings[4:8]
    if pool is not None:
        tk = text_pairs(_join(pool["pieces"]), config.k, wide=config.wide)[0]
        uni[100:400] = tk[rng.integers(0, len(tk), 300)]
        keep = np.sort(np.unique(uni, axis=0, return_index=True)[1])
        uni = uni[keep]
    weights = 0.997 ** np.arange(len(uni) - 1)
    weights /= weights.sum()
    if has("pairs"):
        hot_key = uni[0]                                                    # (the weighted draws take uni[1:])
    else:
        hot_key = text_pairs(pool["hot"], config.k, True, False, 0, config.stranded, config.w, config.s, config.wide)[0][0]
    hot_key = np.array(hot_key, dtype=np.uint64).reshape(1, words)
    graveyard = np.zeros((0, words), dtype=np.uint64)

    def shape(keys):
        return np.ascontiguousarray(keys[:, 0] if words == 1 else keys)

    def pair_batch(n, first=False, second=False):
        if first:                                                           # half the universe, every key of it at least once: the second
            half = (len(uni) - 1) // 2                                      # load brings as many new keys again and the table doubles
            which = 1 + rng.choice(half, n, p=weights[:half] / weights[:half].sum())
            which[:half] = np.arange(1, half + 1)
        else:
            which = 1 + rng.choice(len(uni) - 1, n, p=weights)
            if second:
                rest = np.arange((len(uni) - 1) // 2 + 1, len(uni))
                which[: len(rest)] = rest
        pos = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        if first:
            pos[0], pos[1] = 0, 0xFFFFFFFF
        sh = rng.permutation(n)
        return {"keys": shape(uni[which][sh]), "pos": pos[sh]}

    def hot_batch():
        keys = np.concatenate([np.repeat(hot_key, HOT, axis=0), uni[1 + rng.choice(len(uni) - 1, 20, p=weights)]])
        sh = rng.permutation(len(keys))
        return {"keys": shape(keys[sh]), "pos": rng.integers(0, 1 << 32, len(keys), dtype=np.uint32)[sh]}

    def base_for(text, edge=False):
        choices = (0, 1, 1 << 20, top - len(text))
        return int(choices[3] if edge else choices[int(rng.integers(0, 4))])

    def seq_text():
        picks = [pool["pieces"][i] for i in rng.permutation(3)[: int(rng.integers(1, 4))]]
        if rng.random() < 0.5:
            picks.append(pool["short"])
        return _join(picks)

    def fastq_text():
        n = int(rng.integers(3, len(pool["records"]) + 1))
        return np.ascontiguousarray(np.concatenate([pool["records"][i] for i in rng.permutation(len(pool["records"]))[:n]]))

    def never(n):
        return rng.integers(1 << 63, 1 << 64, (n, words), dtype=np.uint64)

    def erase_batch(n, protected, everything=False):
        live = bag.live()[0]
        if protected:
            live = live[~isin_rows(live, hot_key)]
        if everything:
            keys = live
        else:
            keys = live[rng.integers(0, len(live), n)] if len(live) else live
        parts = [keys, never(5 if everything else n // 4), keys[: len(keys) // 8]]     # live, never inserted, an eighth repeated
        if words == 2 and len(keys):
            near = keys[: max(1, len(keys) // 8)].copy()
            near[:, 1] ^= np.uint64(1 << 63)                                # a live key's w0 under another w1
            parts.append(near)
        return {"keys": shape(rng.permutation(np.concatenate(parts)))}

    def hot_count():
        u, c = bag.live()
        r = isin_rows(u, hot_key)
        return int(c[r][0]) if r.any() else 0

    def drawn_counts(protected):
        c = np.unique(bag.live()[1])
        if len(c) == 0:
            return {"lo": 1, "hi": 5}
        lo, hi = sorted(int(x) for x in c[rng.integers(0, len(c), 2)])
        h = hot_count()
        if protected and lo <= h <= hi:
            hi = h - 1
        return {"lo": lo, "hi": hi}

    def queries():
        live = bag.live()[0]
        hits = live[rng.integers(0, len(live), min(len(live), 200))] if len(live) else live
        parts = [hits, hits[:20], graveyard[:50], never(50), hot_key, siblings]
        if words == 2 and len(hits):
            near = hits[:20].copy()
            near[:, 1] ^= np.uint64(1 << 63)
            parts.append(near)
        return shape(rng.permutation(np.concatenate(parts)))

    for step in range(STEPS):
        kind = FIXED.get(step, "drawn")
        protected = step < PROTECTED_UNTIL
        device = bool(step & 1)
        call = None
        if kind == "text_run" and not has("sequences"):
            kind = "drawn"
        if kind == "append_fastq" and not has("fastq"):
            kind = "drawn"
        if kind == "drawn":
            empty = bag.total() == 0
            names = sorted(ops_of(config) - ({BUILDS[f] for f in config.forms} if not empty else set()) - ({"clear"} if protected else set()))
            p = np.array([0.3 if n == "clear" else 1.0 if n.startswith(("erase", "drop")) else 2.0 for n in names])
            op = names[int(rng.choice(len(names), p=p / p.sum()))]
        else:
            op = None

        if kind in ("build_big", "append_big", "append_some", "build_a", "build_b"):
            verb = BUILDS if kind.startswith("build") else APPENDS
            if kind == "build_a":
                form = "sequences" if has("sequences") else "pairs"
            elif kind == "build_b":
                form = "fastq" if has("fastq") else "pairs"
            else:
                form = "pairs" if has("pairs") else "sequences"
            op = verb[form]
            if kind == "build_a" and not has("pairs"):
                device = True                                               # (a config without pair forms: its build_sequences from a tensor too)
            if form == "pairs":
                n = 20000 if kind.endswith("big") else int(rng.choice([1, 7, 300, 4097])) if kind == "append_some" else SIZES[int(rng.integers(0, len(SIZES)))]
                call = pair_batch(n, first=step == 0, second=step == 1)
            elif form == "sequences":
                # (the second load repeats one piece only: k-mers that occur exactly once stay)
                call = {"text": _join([pool["pieces"][1], pool["short"]]) if kind == "append_big" else pool["pieces"][0] if kind == "build_big"
                        else seq_text()}
            else:
                call = {"text": fastq_text()}
        elif kind == "hot":
            if has("pairs"):
                op, call = "append", hot_batch()
            else:
                op, call = "append_sequences", {"text": pool["hot"], "homopolymer": True}
        elif kind == "text_run":
            op, call = "append_sequences", {"text": _join([pool["run"], pool["short"]]), "homopolymer": True}
            call["pos_base"] = base_for(call["text"], edge=True)            # the upper edge of the coordinate space has to be accepted
        elif kind == "append_fastq":
            op, call = "append_fastq", {"text": fastq_text()}
        elif kind == "erase":
            op, call = "erase", erase_batch(300, protected)
        elif kind == "erase_all":
            op, call, device = "erase", erase_batch(0, False, everything=True), False
        elif kind == "counts_one":
            op, call = "erase_counts", {"lo": 1, "hi": 1}
        elif kind == "counts_none":
            c = bag.live()[1]
            present = np.zeros(int(c.max()) + 2 if len(c) else 2, dtype=bool)
            present[c] = True
            gap = int(rng.choice(np.nonzero(~present[1:])[0] + 1))          # a count no key has
            op, call = "erase_counts", {"lo": gap, "hi": gap}
        elif kind == "counts_empty":
            c = drawn_counts(False)
            op, call = "erase_counts", {"lo": max(c["lo"], c["hi"]) + 1, "hi": min(c["lo"], c["hi"])}
        elif kind == "counts_hot":
            op, call = "erase_counts", {"lo": hot_count(), "hi": hot_count()}
        elif kind == "drop_above":
            c = np.unique(bag.live()[1])
            op, call = "drop_above", {"max_occ": int(c[rng.integers(0, len(c))])}
        elif kind == "clear":
            op, call = "clear", {}
        else:
            assert kind == "drawn", kind
            if op in ("build", "append"):
                call = pair_batch(SIZES[int(rng.integers(0, len(SIZES)))])
            elif op in ("build_sequences", "append_sequences"):
                call = {"text": seq_text()}
            elif op in ("build_fastq", "append_fastq"):
                call = {"text": fastq_text()}
            elif op == "erase":
                call = erase_batch(int(rng.choice([0, 1, 7, 300, 4097])), protected)
            elif op == "erase_counts":
                call = drawn_counts(protected)
            elif op == "drop_above":
                c = np.unique(bag.live()[1])
                call = {"max_occ": int(c[rng.integers(0, len(c))]) if len(c) else 3}
                if protected:
                    call["max_occ"] = max(call["max_occ"], hot_count())
            else:
                call = {}
        if op.startswith("append_") and "pos_base" not in call:
            call["pos_base"] = base_for(call["text"])
        call.update(step=step, kind=kind, op=op, device=device)
        call.setdefault("homopolymer", False)

        before = bag.live()[0]
        model_apply(bag, config, call)
        if op in ("erase", "erase_counts", "drop_above", "clear"):
            gone = before[~isin_rows(before, bag.live()[0])] if len(before) else before
            if len(gone):
                graveyard = rng.permutation(gone)
        call["queries"] = queries()
        if pool is not None and step % 5 == 4:
            o = int(rng.integers(0, 2700))
            call["qtext"] = np.ascontiguousarray(np.concatenate([pool["pieces"][0][o:o + 300], np.full(config.k + 3, ord("A"), dtype=np.uint8)]))
        yield call
