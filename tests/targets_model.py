"""The definition of kh_anchor_targets (include/kmerhash_amd.h) in Python integers: the search loop word for word, the clamped
segments, the sort and the groups.  The kernels equal it bit for bit (tests/test_gpu_targets.py); tests/test_targets_model.py checks it
against a brute-force version."""
NONE = 0xFFFFFFFF          # KH_TARGET_NONE, and KH_POS_INVALID
LIM = 1 << 31


def target_of(r, t_start, t_end, k):
    """tid of an anchor at reference position r"""
    lo, hi = 0, len(t_start)
    while lo < hi:
        mid = (lo + hi) >> 1
        if t_start[mid] <= r:
            lo = mid + 1
        else:
            hi = mid
    t = lo - 1
    if t >= 0 and r < LIM and r + k <= t_end[t]:
        return t
    return NONE


def segments(m, seg_offsets):
    """the clamped segments [(a, b)], and whether the offsets ascend from 0 to m (None: one segment [0, m))"""
    if seg_offsets is None:
        return [(0, m)], True
    seg = [int(x) for x in seg_offsets]
    out, ok = [], len(seg) >= 2 and seg[0] == 0 and seg[-1] == m
    for s in range(len(seg) - 1):
        a = min(seg[s], m)
        b = max(a, min(seg[s + 1], m))
        out.append((a, b))
        ok = ok and seg[s] <= seg[s + 1] <= m
    return out, ok


def anchor_targets(qpos, rpos, rev, seg_offsets, t_start, t_end, k):
    """-> dict(ok, q, r, v, tid, src, g_off, g_seg, g_tid) as lists of ints; ok == False: KH_ERR_INVALID, the rest is unspecified (None)"""
    m = len(qpos)
    ts, te = [int(x) for x in t_start], [int(x) for x in t_end]
    segs, ok = segments(m, seg_offsets)
    if m == 0:
        return dict(ok=True, q=[], r=[], v=[], tid=[], src=[], g_off=[0], g_seg=[], g_tid=[])
    if not ok:
        return dict(ok=False)
    tid = [target_of(int(r), ts, te, k) for r in rpos]
    src, g_off, g_seg, g_tid = [], [], [], []
    for s, (a, b) in enumerate(segs):
        order = sorted(range(a, b), key=lambda i: (tid[i], i))      # NONE is the largest id: last in its segment
        for j, i in enumerate(order):
            if j == 0 or tid[i] != tid[order[j - 1]]:
                g_off.append(len(src))
                g_seg.append(s)
                g_tid.append(tid[i])
            src.append(i)
    g_off.append(m)
    return dict(ok=True, q=[int(qpos[i]) for i in src], r=[NONE if tid[i] == NONE else int(rpos[i]) for i in src], v=[int(rev[i]) for i in src],
                tid=[tid[i] for i in src], src=src, g_off=g_off, g_seg=g_seg, g_tid=g_tid)
