"""lsdr_ts_stitch's definition (include/lsdr_hip.h) restated in numpy — a test oracle, never imported by the product — and the streams
its tests are run on, cut from ts_common.build_stream(n=3000).

join(t, h, W, M) is the record of one pair, stitch(streams, W, M) what capi.TsStitch.stitch returns: (joins, keep, bytes).
"""
import functools

import numpy as np
import ts_common as tc

W, M, MAX_PACKETS = 256, 8, 1200


def _packets(ts):
    return tc.packets_of(ts) if len(ts) else np.zeros((0, 188), np.uint8)


def join(t, h, window=W, min_run=M):
    """The join of the pair (t, h): dict(joined, run, end, next_start)."""
    t, h = _packets(t), _packets(h)
    T, H = t[len(t) - min(window, len(t)):], h[:min(window, len(h))]
    none = dict(joined=0, run=0, end=len(t), next_start=0)
    if not len(T) or not len(H):
        return none
    ids = {}
    it = np.array([ids.setdefault(p.tobytes(), len(ids)) for p in T])        # equal bytes, equal number
    ih = np.array([ids.setdefault(p.tobytes(), len(ids)) for p in H])
    eq = it[:, None] == ih[None, :]
    not_null = (((T[:, 1].astype(int) & 0x1f) << 8) | T[:, 2]) != tc.NULL_PID
    best = None                                                               # (−L, a, b): the smallest is the join
    for d in range(-(len(T) - 1), len(H)):
        v = np.diagonal(eq, d).astype(np.int8)
        edges = np.flatnonzero(np.diff(np.concatenate(([0], v, [0]))))
        for i0, i1 in zip(edges[0::2], edges[1::2]):                          # a maximal run: the cells [i0, i1) of the diagonal
            b = int(i0) + max(0, -d)
            L = int(i1 - i0)
            if L >= min_run and int(not_null[b:b + L].sum()) >= (min_run + 1) // 2:
                cand = (-L, b + d, b)
                best = cand if best is None or cand < best else best
    if best is None:
        return none
    L, a, b = -best[0], best[1], best[2]
    return dict(joined=1, run=L, end=len(t) - len(T) + b + L, next_start=a + L)


def stitch(streams, window=W, min_run=M):
    """(joins, keep, the stitched TS's bytes) of the streams (uint8 [n][188] arrays or bytes; an empty one is valid)."""
    s = [_packets(x) for x in streams]
    joins = [join(s[k], s[k + 1], window, min_run) for k in range(len(s) - 1)]
    keep, out, off = [], [], 0
    for k, x in enumerate(s):
        start = joins[k - 1]["next_start"] if k else 0
        end = max(start, joins[k]["end"] if k + 1 < len(s) else len(x))
        keep.append(dict(start=start, end=end, out_offset=off))
        out.append(x[start:end].tobytes())
        off += end - start
    return joins, keep, b"".join(out)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base():
    return tc.build_stream(n=3000)[0]


def null_packets(n):
    p = np.full((n, 188), 0xff, np.uint8)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = 0x47, 0x1f, 0xff, 0x10
    return p


def without(x, places):
    return np.delete(x, places, axis=0)


def cases():
    """[(name, [stream 0 … 3], joined flags expected or None)]; every stream at most MAX_PACKETS packets, overlaps inside W."""
    b = base()
    cut = lambda lo, hi: b[lo:hi].copy()
    plain = [cut(0, 900), cut(800, 1700), cut(1600, 2400), cut(2300, len(b))]
    out = [("plain overlaps", plain, [1, 1, 1])]
    # packets deleted inside the overlap [800, 900): the true match spans several diagonals, the longest piece is the join
    left = [without(plain[0], [830, 861, 862]), plain[1], plain[2], plain[3]]
    right = [plain[0], without(plain[1], [20, 45, 46, 47]), plain[2], plain[3]]
    both = [without(plain[0], [815, 870]), without(plain[1], [40, 41, 77]), without(plain[2], [750]), without(plain[3], [12, 60])]
    out += [("deleted on the left", left, [1, 1, 1]), ("deleted on the right", right, [1, 1, 1]), ("deleted on both sides", both, [1, 1, 1])]
    nulls = null_packets(60)
    out.append(("an overlap of null packets only", [np.concatenate([cut(0, 800), nulls]), np.concatenate([nulls, cut(800, 1700)]), plain[2], plain[3]],
                [0, 1, 1]))
    block = cut(2900, 2912)                                                   # twelve packets that stand in both streams at another diagonal
    out.append(("a periodic stretch", [np.concatenate([cut(0, 700), block, cut(700, 900)]), np.concatenate([cut(800, 950), block, cut(950, 1700)]),
                                       plain[2], plain[3]], [1, 1, 1]))
    out.append(("an overlap shorter than M", [cut(0, 805), cut(800, 1700), plain[2], plain[3]], [0, 1, 1]))
    out.append(("an empty stream in the middle", [plain[0], cut(0, 0), plain[1], plain[2]], [0, 0, 1]))
    out.append(("a stream shorter than W", [plain[0], cut(860, 980), cut(940, 1700), plain[2]], [1, 1, 1]))
    out.append(("a stream its joins consume", [plain[0], cut(850, 950), np.concatenate([cut(860, 890), cut(2000, 2500)]), cut(2450, 2990)], [1, 1, 1]))
    changed = plain[1].copy()
    changed[50, 100] ^= 1                                                     # one bit in the middle of the overlap: two runs of 50 and 49
    out.append(("one bit changed inside the overlap", [plain[0], changed, plain[2], plain[3]], [1, 1, 1]))
    return out
