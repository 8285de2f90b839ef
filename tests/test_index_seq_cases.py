"""CPU: the yardstick and the generator of the position-index operation sequences, before anything runs on a GPU.  PairBag and its
per-call models (tests/index_seq_model.py) against a dict of Python lists on tiny inputs, every op and both key widths; then every drawn
sequence of tests/index_seq_cases.py replayed on the model alone, asserting what the sequences claim to cover."""
import numpy as np
import pytest

from tests.index_seq_cases import (BY_ID, CONFIGS, FIXED, SEEDS, STEPS, T, batch_of_call, draw_sequence, hash_of, home_bits, model_apply, ops_of,
                                   words_of)
from tests.index_seq_model import PairBag, isin_rows, key_rows, rank_rows, text_pairs, unique_rows


# ---- PairBag against brute force ------------------------------------------------------------------------------------------------------
class Brute:
    """key (a tuple of words) -> list of positions"""

    def __init__(self, words):
        self.d, self.words = {}, words

    def append(self, keys, pos):
        for k, p in zip(keys.tolist(), pos.tolist()):
            self.d.setdefault(tuple(k), []).append(p)

    def erase(self, keys):
        nk = npos = 0
        for k in keys.tolist():
            got = self.d.pop(tuple(k), None)
            if got is not None:
                nk, npos = nk + 1, npos + len(got)
        return nk, npos

    def erase_counts(self, lo, hi):
        gone = [k for k, v in self.d.items() if lo <= len(v) <= hi]
        return self.erase(np.array(gone, dtype=np.uint64).reshape(len(gone), self.words))

    def sorted_keys(self, words):
        return sorted(self.d, key=lambda k: tuple(reversed(k)))                # (w1 is the major word)


def check_bag(bag, brute, words, rng):
    ks = brute.sorted_keys(words)
    assert (bag.size(), bag.total()) == (len(ks), sum(len(v) for v in brute.d.values()))
    u, c = bag.live()
    assert u.tolist() == [list(k) for k in ks] and c.tolist() == [len(brute.d[k]) for k in ks]
    m = bag.as_model()
    assert (m.size(), m.total()) == (bag.size(), bag.total())
    assert key_rows(m.keys, words).tolist() == [list(k) for k in ks]
    absent = [tuple([7] * words), tuple([0] * (words - 1) + [9])]
    q = [ks[i] for i in rng.integers(0, len(ks), 6)] + absent if ks else absent
    qa = np.array(q, dtype=np.uint64).reshape(len(q), words)
    qa = qa[:, 0] if words == 1 else qa
    want = [sorted(brute.d.get(k, [])) for k in q]
    assert m.count(qa).tolist() == [len(w) for w in want]
    fo, fp = m.find(qa)
    assert fo.dtype == np.uint64 and fp.dtype == np.uint32
    assert fo.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist() and fp.tolist() == [p for w in want for p in w]
    order = [ks[i] for i in rng.permutation(len(ks))]                           # any slot order
    oa = np.array(order, dtype=np.uint64).reshape(len(order), words)
    eo, ep = m.export_in_key_order(oa[:, 0] if words == 1 else oa)
    assert eo.dtype == np.uint32 and eo.tolist() == np.concatenate([[0], np.cumsum([len(brute.d[k]) for k in order])]).tolist()
    assert ep.tolist() == [p for k in order for p in sorted(brute.d[k])]


@pytest.mark.parametrize("words", [1, 2])
def test_pairbag_against_a_dict_of_lists(words):
    rng = np.random.default_rng(words)
    small = np.array([0, 1, 2, (1 << 64) - 1], dtype=np.uint64)                # few values per word: repeats, keys that differ in w1 only
    bag, brute = PairBag(words), Brute(words)
    check_bag(bag, brute, words, rng)
    assert bag.erase(np.zeros((0, words), dtype=np.uint64)) == (0, 0) and bag.erase_counts(0, 2 ** 32 - 1) == (0, 0)
    for rnd in range(60):
        op = ["append", "append", "erase", "erase_counts", "drop_above", "clear"][int(rng.integers(0, 6))] if rnd > 2 else "append"
        if op == "append":
            n = int(rng.integers(0, 12))
            keys, pos = small[rng.integers(0, 4, (n, words))], rng.integers(0, 3, n).astype(np.uint32)      # duplicate pairs occur
            assert bag.append(keys, pos) == n
            brute.append(keys, pos)
        elif op == "erase":
            keys = small[rng.integers(0, 4, (int(rng.integers(0, 5)), words))]
            keys = np.concatenate([keys, keys[:2]])                             # repeats in the batch
            assert bag.erase(keys) == brute.erase(keys)
        elif op == "erase_counts":
            lo, hi = int(rng.integers(0, 6)), int(rng.integers(0, 6))           # lo > hi occurs: the empty range
            got = bag.erase_counts(lo, hi)
            assert got == brute.erase_counts(lo, hi) and (lo <= hi or got == (0, 0))
        elif op == "drop_above":
            mx = int(rng.integers(0, 5))
            assert bag.drop_above(mx) == brute.erase_counts(mx + 1, 2 ** 32 - 1)
            assert bag.drop_above(2 ** 32 - 1) == (0, 0)
        elif rng.random() < 0.3:
            bag.clear()
            brute.d.clear()
        check_bag(bag, brute, words, rng)


def test_rows_helpers():
    rows = np.array([[5, 1], [5, 0], [0, 1], [5, 0], [(1 << 64) - 1, 0]], dtype=np.uint64)
    u, c = unique_rows(rows)
    assert u.tolist() == [[5, 0], [(1 << 64) - 1, 0], [0, 1], [5, 1]] and c.tolist() == [2, 1, 1, 1]
    r, hit = rank_rows(u, np.array([[5, 1], [5, 2], [0, 0], [5, 0]], dtype=np.uint64))
    assert hit.tolist() == [True, False, False, True] and r[hit].tolist() == [3, 0]
    assert isin_rows(rows, np.array([[5, 0], [1, 1]], dtype=np.uint64)).tolist() == [False, True, False, True, False]


def test_text_pairs_states_pos_base_and_the_stamp():
    text = np.frombuffer(b"ACGTTGCAAGGCTNACGTACGTTTGACCA\nGGATCCAAGT", dtype=np.uint8)
    k0, p0 = text_pairs(text, 5)
    k1, p1 = text_pairs(text, 5, pos_base=2 ** 32 - len(text))
    assert np.array_equal(k0, k1) and np.array_equal(p1.astype(np.int64) - p0, np.full(len(p0), 2 ** 32 - len(text)))
    ks, ps = text_pairs(text, 5, pos_base=2 ** 31 - len(text), stranded=True)
    assert np.array_equal(ks, k0) and np.array_equal(ps >> 1, p0.astype(np.int64) + 2 ** 31 - len(text)) and len(set((ps & 1).tolist())) == 2
    kw, pw = text_pairs(text, 5, wide=True)
    assert kw.shape == (len(k0), 2) and np.array_equal(kw[:, 0], k0[:, 0]) and not kw[:, 1].any() and np.array_equal(pw, p0)


# ---- coverage of every drawn sequence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("cid", [c.id for c in CONFIGS])
def test_what_every_sequence_covers(cid, seed):
    config = BY_ID[cid]
    words = words_of(config)
    bag = PairBag(words)
    seen, where = set(), {"append": set(), "erase": set()}
    crossed, small_cross, emptied, refilled = set(), False, False, False
    counts_hit = counts_miss = False
    text_big, strand_bits, sampled, windows = False, set(), 0, 0
    kinds, siblings_live, siblings_absent = {}, 0, 0
    steps = 0
    for call in draw_sequence(config, seed):
        op = call["op"]
        assert call["step"] == steps and call["kind"] in ("drawn", FIXED.get(steps))
        steps += 1
        kinds[call["kind"]] = op
        seen.add(op)
        if op.startswith("build"):
            assert bag.total() == 0, "a build on a loaded index would be refused"
        if op.startswith(("build", "append")):
            keys, pos = batch_of_call(config, call)
            where["append"].add(call["device"])
            u, c = unique_rows(keys)
            before = np.zeros(len(u), dtype=np.int64)
            lu, lc = bag.live()
            r, hit = rank_rows(lu, u)
            before[hit] = lc[r[hit]]
            after = before + c
            for m in (T, 2 * T):                                                # a segment that passes the multiple m in this call
                over = (before <= m) & (after > m)
                if over.any():
                    crossed.add((m, bool((c[over] < T).any())))
            small_cross |= bool(((before // T != after // T) & (c < T) & (before > 0)).any())
            if emptied:
                refilled |= len(pos) > 0
            if op.endswith(("sequences", "fastq")):
                text_big |= bool((c > T).any())
                if config.stranded:
                    strand_bits |= set((pos & 1).tolist())
                if (config.w or config.s) and not call["homopolymer"]:
                    sampled += len(pos)
                    windows += len(text_pairs(call["text"], config.k, fastq=op.endswith("fastq"), wide=config.wide)[1])
            else:
                assert len(pos) in (0, 1, 7, 300, 4097, 20000) or call["kind"] == "hot"
        if op == "erase":
            where["erase"].add(call["device"])
        ret = model_apply(bag, config, call)
        if op in ("erase", "erase_counts", "drop_above"):
            if op == "erase" and ret[0] > 0 and bag.total() == 0:
                emptied = True
            if op == "erase_counts":
                counts_hit |= ret[0] > 0
                counts_miss |= ret == (0, 0)
            if call["kind"] == "counts_one":
                assert ret[0] > 0 and ret[0] == ret[1]
            if call["kind"] in ("counts_none", "counts_empty"):
                assert ret == (0, 0) and (call["kind"] == "counts_none") == (call["lo"] <= call["hi"])
            if call["kind"] == "counts_hot":
                assert ret[0] == 1 and ret[1] > 2 * T, "the range matches the hot key alone"
        assert len(call["queries"]) > 50
        if config.wide:
            # queries that share w0 AND the home bucket with another query: live ones and ones the index does not hold
            q = unique_rows(key_rows(call["queries"], 2))[0]
            w0s, n0 = np.unique(q[:, 0], return_counts=True)
            fam = q[q[:, 0] == w0s[np.argmax(n0)]]
            fam = fam[home_bits(fam, hash_of(config, seed)) == home_bits(fam[:1], hash_of(config, seed))[0]]
            live = isin_rows(fam, bag.live()[0])
            siblings_live, siblings_absent = max(siblings_live, int(live.sum())), max(siblings_absent, int((~live).sum()))
    assert steps == STEPS
    assert seen == ops_of(config), (seen, ops_of(config))
    assert (T, True) in crossed and (2 * T, True) in crossed, "a segment passes 4096 and 8192 by accumulation, less than a tile added per call"
    assert small_cross and emptied and refilled and counts_hit and counts_miss
    assert where == {"append": {False, True}, "erase": {False, True}}
    if config.wide:
        assert siblings_live >= 4 and siblings_absent >= 4, "keys of one w0 and one home bucket, some in the index and some not, are looked up together"
    if "sequences" in config.forms:
        assert text_big, "one text call gives one k-mer more than a tile of positions"
    if config.stranded:
        assert strand_bits == {0, 1}
    if config.w or config.s:
        share, want = sampled / windows, 2.0 / ((config.w + 1) if config.w else (config.k - config.s + 1))
        # the expected density on random text (KmerPositionIndex.__init__); N, lower case and the repeats between pieces move it a little
        assert 0.7 * want < share < 1.3 * want, (share, want)
