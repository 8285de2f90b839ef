"""GPU: random operation sequences over the two position indexes (KmerPositionIndex / WideKmerPositionIndex: build, append, erase,
erase_counts, drop_above and clear, the text forms with pos_base, the strand stamp and the two samplers) against the numpy model of the
whole history, exactly.  tests/index_seq_cases.py draws the 30 calls of a sequence from the model alone; here every call is made on a
real index and on a PairBag, and after EVERY call the return value, size, total, export, count, find (host and device queries) and
the layout of the counting twin are compared.  A failure names config, seed, step, op and the first differing key: replay it with
python tests/soak_index_fuzz.py 0 <seed> <config id>."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kmerhash_amd as kh  # noqa: E402
from kmerhash_amd import wide as W  # noqa: E402
from tests.index_seq_cases import CONFIGS, SEEDS, BY_ID, batch_of_call, draw_sequence, hash_of, model_apply, words_of  # noqa: E402
from tests.index_seq_model import PairBag, isin_rows, key_rows, text_pairs  # noqa: E402


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()


def host(t, dt):
    return t.cpu().numpy().view(dt)


def new_index(config, hash_):
    cls = kh.WideKmerPositionIndex if config.wide else kh.KmerPositionIndex
    return cls(k=config.k, hash=hash_, w=config.w, s=config.s, stranded=config.stranded)


def new_twin(config, hash_):
    make = kh.hashmap_robinhood_doubling_wide if config.wide else kh.hashmap_robinhood_doubling
    return make(128, 0.35, 0.8, hash=hash_, seed=43)


def do_call(ix, call):
    """the call on a real index -> its return value"""
    op, d = call["op"], call["device"]
    if op in ("build", "append"):
        keys, pos = (dev(call["keys"], np.int64), dev(call["pos"], np.int32)) if d else (call["keys"], call["pos"])
        return getattr(ix, op)(keys, pos)
    if op in ("build_sequences", "build_fastq", "append_sequences", "append_fastq"):
        text = torch.from_numpy(call["text"]).cuda() if d else call["text"]
        return getattr(ix, op)(text, pos_base=call["pos_base"]) if op.startswith("append") else getattr(ix, op)(text)
    if op == "erase":
        return ix.erase(dev(call["keys"], np.int64) if d else call["keys"])
    if op == "erase_counts":
        return ix.erase_counts(call["lo"], call["hi"])
    if op == "drop_above":
        return ix.drop_above(call["max_occ"])
    assert op == "clear", op
    return ix.clear()


def key_at(keys, i):
    return [hex(int(w)) for w in np.atleast_1d(keys[i])]


def first_diff(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(a[:n] != b[:n])[0]
    return int(d[0]) if len(d) else n


def check_export(ix, m, words, ctx):
    ek, eo, ep = ix.export()
    assert len(eo) == len(ek) + 1 and eo[0] == 0 and eo[-1] == m.total() == len(ep), "%s: export offsets run 0..%d, model total %d" % (ctx, eo[-1], m.total())
    rows = key_rows(ek, words)
    r, hit = m._rank(ek)
    assert hit.all(), "%s: export holds key %s, which the model does not" % (ctx, key_at(rows, int(np.argmin(hit))))
    assert len(np.unique(r)) == len(r) == m.size(), "%s: export holds %d keys, %d distinct; the model has %d" % (ctx, len(r), len(np.unique(r)), m.size())
    mo, mp = m.export_in_key_order(ek)
    if not np.array_equal(eo, mo):
        i = first_diff(np.diff(eo.astype(np.int64)), np.diff(mo.astype(np.int64)))
        raise AssertionError("%s: segment of key %s has %d positions, the model %d" % (ctx, key_at(rows, i), int(eo[i + 1]) - int(eo[i]), int(mo[i + 1]) - int(mo[i])))
    if not np.array_equal(ep, mp):
        j = first_diff(ep, mp)
        i = int(np.searchsorted(eo, j, side="right")) - 1
        raise AssertionError("%s: position %d of key %s is %d, the model's %d" % (ctx, j - int(eo[i]), key_at(rows, i), int(ep[j]), int(mp[j])))
    if len(ep) > 1:
        falls = np.diff(ep.astype(np.int64)) < 0
        falls[eo[1:-1].astype(np.int64)[(eo[1:-1] > 0) & (eo[1:-1] < len(ep))] - 1] = False          # (between two segments anything goes)
        assert not falls.any(), "%s: a segment does not ascend at export position %d" % (ctx, int(np.argmax(falls)))
    return ek, eo


def check_lookups(ix, m, q, words, ctx):
    """count and find of one query batch, from host arrays and from CUDA tensors: byte-identical to each other and to the model"""
    rows = key_rows(q, words)
    xc = m.count(q)
    xo, xp = m.find(q)
    dq = dev(q, np.int64)
    for where, c, (fo, fp), (lo, none) in (("host", ix.count(q), ix.find(q), ix.find(q, positions=False)),
                                          ("device", host(ix.count(dq), np.uint32), [host(t, d) for t, d in zip(ix.find(dq), (np.uint64, np.uint32))],
                                           ix.find(dq, positions=False))):
        if c.tobytes() != xc.tobytes():
            i = first_diff(c, xc)
            raise AssertionError("%s: count (%s queries) of key %s is %d, the model's %d" % (ctx, where, key_at(rows, i), int(c[i]), int(xc[i])))
        if fo.tobytes() != xo.tobytes():
            i = first_diff(np.diff(fo.astype(np.int64)), np.diff(xo.astype(np.int64)))
            raise AssertionError("%s: find (%s queries) gives key %s %d positions, the model %d" % (ctx, where, key_at(rows, i), int(fo[i + 1] - fo[i]), int(xo[i + 1] - xo[i])))
        if fp.tobytes() != xp.tobytes():
            j = first_diff(fp, xp)
            i = int(np.searchsorted(xo, j, side="right")) - 1
            raise AssertionError("%s: find (%s queries): position %d of key %s is %d, the model's %d" % (ctx, where, j - int(xo[i]), key_at(rows, i), int(fp[j]), int(xp[j])))
        lo = lo if where == "host" else host(lo, np.uint64)
        assert none is None and lo.tobytes() == xo.tobytes(), "%s: find(positions=False) (%s queries) differs from the model's offsets at query %d" % (ctx, where, first_diff(lo, xo))


def check_find_sequences(ix, m, config, call, ctx):
    """find_sequences over a short query text: the index's own sampling of it against the model's windows (or sampled windows)"""
    km, qpos = text_pairs(call["qtext"], config.k, True, False, 0, False, config.w, config.s, config.wide)
    xo, xp = m.find(km[:, 0] if not config.wide else km)
    got = ix.find_sequences(torch.from_numpy(call["qtext"]).cuda() if call["device"] else call["qtext"])
    gq, go, gp = [host(t, d) for t, d in zip(got, (np.uint32, np.uint64, np.uint32))] if call["device"] else got
    assert np.array_equal(gq, qpos), "%s: find_sequences samples %d windows of the query, the model %d (first difference at %d)" % (ctx, len(gq), len(qpos), first_diff(gq, qpos))
    assert np.array_equal(go, xo) and np.array_equal(gp, xp), "%s: find_sequences differs from the model at query window %d (key %s)" % (
        ctx, min(first_diff(np.diff(go.astype(np.int64)), np.diff(xo.astype(np.int64))), len(km) - 1), key_at(km, min(first_diff(np.diff(go.astype(np.int64)), np.diff(xo.astype(np.int64))), len(km) - 1)))


def sorted_inside_home_runs(tk, tv, home, words):
    """check_layout_against_twin's canonical form (tests/test_gpu_index_mutate.py and its wide counterpart) without a loop over the runs:
    (keys, values) in slot order with every run of equal home bucket sorted by key -- (w1, w0) for 16-byte keys --; a run that wraps from
    the last slot to the first one is sorted along the ring"""
    n = len(home)
    if n < 2:
        return tk, tv
    starts = np.nonzero(home[1:] != home[:-1])[0] + 1
    rot = int(starts[0]) if len(starts) and home[0] == home[-1] else 0           # rotate so that a wrapped run becomes one stretch
    idx = np.roll(np.arange(n), -rot)
    h = home[idx]
    run = np.concatenate([[0], np.cumsum(h[1:] != h[:-1])])
    rows = key_rows(tk, words)[idx]
    order = np.lexsort(tuple(rows[:, j] for j in range(words)) + (run,))
    ck, cv = tk.copy(), tv.copy()
    ck[idx], cv[idx] = tk[idx][order], tv[idx][order]
    return ck, cv


def check_twin(ix, twin, config, hash_, ek, eo, ctx, layout=True):
    assert (ix.size(), ix.capacity()) == (twin.size(), twin.capacity()), "%s: size / capacity %r, the counting twin's %r" % (
        ctx, (ix.size(), ix.capacity()), (twin.size(), twin.capacity()))
    if not layout:
        return
    words = words_of(config)
    if config.wide:
        assert np.array_equal(ix.export_info(), twin.export_info()), "%s: the info bytes differ from the twin's" % ctx
    tk, tv = twin.to_vector()
    hashes = (W.hash_batch_wide if config.wide else kh.hash_batch)(tk, hash_, 43) if len(tk) else np.zeros(0, dtype=np.uint64)
    home = (hashes & np.uint64(twin.capacity() - 1)).astype(np.int64)
    ck, cv = sorted_inside_home_runs(tk, tv, home, words)
    if not np.array_equal(ek, ck):
        i = first_diff(key_rows(ek, words).view(np.dtype((np.void, 8 * words))).ravel(), key_rows(ck, words).view(np.dtype((np.void, 8 * words))).ravel())
        raise AssertionError("%s: slot %d of the export holds key %s, the twin's layout %s" % (ctx, i, key_at(key_rows(ek, words), i), key_at(key_rows(ck, words), i)))
    lens = np.diff(eo.astype(np.int64))
    assert np.array_equal(lens, cv.astype(np.int64)), "%s: segment length of key %s differs from the twin's count" % (ctx, key_at(key_rows(ek, words), first_diff(lens, cv.astype(np.int64))))


def run_sequence(config, seed, checks=True):
    """replays draw_sequence(config, seed) on an index, a PairBag and the counting twin, checking after every call -> (the final export,
    the names of the kernels that ran, whether the table doubled)"""
    hash_ = hash_of(config, seed)
    words = words_of(config)
    ix, twin, bag = new_index(config, hash_), new_twin(config, hash_), PairBag(words)
    doubled, kernels = False, set()
    try:
        ix.profile_enable(True)
        for call in draw_sequence(config, seed):
            op = call["op"]
            ctx = "config %s seed %d step %d op %s (%s, hash %s)" % (config.id, seed, call["step"], op, call["kind"], hash_)
            before, cap = bag.live()[0], ix.capacity()
            want = model_apply(bag, config, call)
            if op == "clear":
                kernels |= set(ix.profile())                                    # (clear gives the index a fresh table: its profile starts anew)
            got = do_call(ix, call)
            doubled |= op.startswith("append") and ix.capacity() > cap
            if not checks:
                continue
            assert got == want, "%s: returned %r, the model %r" % (ctx, got, want)
            m = bag.as_model()
            assert (ix.size(), ix.total()) == (m.size(), m.total()), "%s: size / total %r, the model's %r" % (ctx, (ix.size(), ix.total()), (m.size(), m.total()))
            ek, eo = check_export(ix, m, words, ctx)
            check_lookups(ix, m, call["queries"], words, ctx)
            if "qtext" in call and (config.s is not None or not config.wide):
                check_find_sequences(ix, m, config, call, ctx)
            # the twin: fed the key batches of the appends, the same keys erased; after erase_counts / drop_above the keys the model lost;
            # clear gives a fresh table, of which only size and capacity are stated
            if op.startswith(("build", "append")):
                keys = batch_of_call(config, call)[0]
                if len(keys):
                    twin.insert_reduce_plus(np.ascontiguousarray(keys[:, 0] if words == 1 else keys))
            elif op == "erase":
                if len(call["keys"]):
                    twin.erase(call["keys"])
            elif op in ("erase_counts", "drop_above"):
                gone = before[~isin_rows(before, bag.live()[0])] if len(before) else before
                if len(gone):
                    twin.erase(np.ascontiguousarray(gone[:, 0] if words == 1 else gone))
            else:
                twin.close()
                twin = new_twin(config, hash_)
            check_twin(ix, twin, config, hash_, ek, eo, ctx, layout=op != "clear")
        return ix.export(), kernels | set(ix.profile()), doubled
    finally:
        ix.close()
        twin.close()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("cid", [c.id for c in CONFIGS])
def test_random_operation_sequences(cid, seed):
    config = BY_ID[cid]
    export, kernels, doubled = run_sequence(config, seed)
    tag = "config %s seed %d" % (cid, seed)
    # both sort paths of the build / append ran (a segment within a tile, a segment across one), and the table doubled under an append
    assert "k_index_tile_sort" in kernels and "k_index_seg_radix" in kernels, "%s: %r" % (tag, sorted(kernels))
    assert doubled, "%s: no append doubled the table" % tag
    if cid in ("n-pairs", "w-pairs"):
        again, _, _ = run_sequence(config, seed, checks=False)                  # determinism: a second index fed the same calls
        assert all(a.tobytes() == b.tobytes() for a, b in zip(export, again)), "%s: a second index fed the same sequence exports other bytes" % tag
