"""The colour layer's definition ("Colour") in plain Python integers, in the manner of attr_ref.py: a dict of slots per
parent whose values are (Y, Co, Cg) triples.  The tree helpers, the pair order and the step are attr_ref's - the layer shares them by
definition; the inverse is its own, because nothing is clamped before the colour transform has been undone."""
import math

import numpy as np

from attr_ref import RATIOS, STAGES, _pairs, _parents, morton, step, symbol

ALPHABET = 1021


def point_color(c):
    """The 8-bit value of one channel of a reader's float32 colour."""
    c = float(np.float32(c))
    if not math.isfinite(c):
        return 0
    return int(min(255.0, max(0.0, math.floor(c + 0.5))))


def rgb_to_ycc(r, g, b):
    co = r - b
    t = b + (co >> 1)
    cg = g - t
    return t + (cg >> 1), co, cg


def ycc_to_rgb(y, co, cg):
    t = y - (cg >> 1)
    g = cg + t
    b = t - (co >> 1)
    return b + co, g, b


def leaf_values(q, rgb8, leaves, D):
    """-> (rgb_mean [U][3], ycc [3][U], cnt [U]); a leaf no point hits has mean (0, 0, 0), cnt = 0."""
    index = {tuple(int(c) for c in lv): i for i, lv in enumerate(leaves)}
    s, n = [[0, 0, 0] for _ in leaves], [0] * len(leaves)
    for p, c in zip(q, rgb8):
        i = index.get(tuple(int(v) for v in p))
        if i is not None and all(0 <= int(v) < (1 << D) for v in p):
            for ch in range(3):
                s[i][ch] += int(c[ch])
            n[i] += 1
    mean = [[((2 * si[ch] + ni) // (2 * ni)) if ni else 0 for ch in range(3)] for si, ni in zip(s, n)]
    ycc = [rgb_to_ycc(*m) for m in mean]
    return mean, [[t[ch] for t in ycc] for ch in range(3)], n


def forward(leaves, ycc, D, Q):
    """ycc [3][U] -> dict(k [3][U - 1], ctx [U - 1] (level - 1), root [3], hist [3 D][1021], level_counts [D + 1])."""
    level = [(morton(lv, D), tuple(int(ycc[ch][i]) for ch in range(3)), 1) for i, lv in enumerate(leaves)]
    assert all(x[0] < y[0] for x, y in zip(level, level[1:])), "leaves are not in strict Morton order"
    counts, blocks = [len(level)], {}
    for j in range(1, D + 1):
        nxt, coefs = [], []
        for pk, slots in _parents(level):
            emitted = {}
            for stage, bit in STAGES:
                emitted[stage] = []
                for lo, hi in _pairs(bit):
                    if hi not in slots:
                        continue
                    if lo in slots:
                        (vl, wl), (vh, wh) = slots[lo], slots[hi]
                        W, s = wl + wh, step(wl, wh, Q)
                        ks, ms = [], []
                        for a, b in zip(vl, vh):
                            d = b - a
                            ms.append(a + (wh * d) // W)
                            k = (abs(d) + (s >> 1)) // s
                            ks.append(k if d > 0 else -k)
                        emitted[stage].append(tuple(ks))
                        slots[lo] = [tuple(ms), W]
                    else:
                        slots[lo] = slots[hi]
                    del slots[hi]
            assert list(slots) == [0]
            coefs += emitted[3] + emitted[2] + emitted[1]
            nxt.append((pk, slots[0][0], slots[0][1]))
        blocks[j] = coefs
        level = nxt
        counts.append(len(level))
    triples, ctx = [], []
    for j in range(D, 0, -1):
        triples += blocks[j]
        ctx += [j - 1] * len(blocks[j])
    k = [[t[ch] for t in triples] for ch in range(3)]
    hist = [[0] * ALPHABET for _ in range(3 * D)]
    for ch in range(3):
        for kk, c in zip(k[ch], ctx):
            hist[ch * D + c][symbol(kk)] += 1
    root = list(level[0][1]) if level else [0, 0, 0]
    return dict(k=k, ctx=ctx, root=root, hist=hist, level_counts=counts)


def inverse(leaves, D, Q, root, k):
    """root [3], k [3][U - 1] -> the leaf colours [U][3] (R, G, B clamped to 0 .. 255 after the inverse colour transform)."""
    if len(leaves) == 0:
        return []
    levels = [[(morton(lv, D), 0, 1) for lv in leaves]]
    for j in range(1, D + 1):
        levels.append([(pk, 0, sum(w for _, w in slots.values())) for pk, slots in _parents(levels[-1])])
    counts = [len(lv) for lv in levels]
    values = {D: [tuple(int(v) for v in root)]}
    pos = 0
    for j in range(D, 0, -1):
        assert pos == counts[j] - 1
        out = []
        for (pk, slots), v in zip(_parents(levels[j - 1]), values[j]):
            w = {s: e[1] for s, e in slots.items()}
            ops = []
            for stage, bit in STAGES:
                for lo, hi in _pairs(bit):
                    if hi not in w:
                        continue
                    if lo in w:
                        ops.append((stage, lo, hi, w[lo], w[hi]))
                        w[lo] += w[hi]
                    else:
                        ops.append((stage, lo, hi, 0, w[hi]))
                        w[lo] = w[hi]
                    del w[hi]
            coef = {}
            for stage in (3, 2, 1):
                for op in ops:
                    if op[0] == stage and op[3]:
                        coef[op[:3]] = tuple(k[ch][pos] for ch in range(3))
                        pos += 1
            val = {0: v}
            for stage, lo, hi, wl, wh in reversed(ops):
                if wl:
                    s = step(wl, wh, Q)
                    lo_v, hi_v = [], []
                    for m, kk in zip(val[lo], coef[(stage, lo, hi)]):
                        dh = kk * s
                        a = m - (wh * dh) // (wl + wh)
                        lo_v.append(a)
                        hi_v.append(a + dh)
                    val[lo], val[hi] = tuple(lo_v), tuple(hi_v)
                else:
                    val[hi] = val.pop(lo)
            out += [val[s] for s in sorted(slots)]
        values[j - 1] = out
    assert pos == len(k[0])
    return [[min(255, max(0, c)) for c in ycc_to_rgb(*v)] for v in values[0]]


def tables():
    """uint16 [16][1022]: the cdf rows over 1021 symbols, the last entry (65536) wrapped to 0."""
    out = np.zeros((len(RATIOS), ALPHABET + 1), np.uint16)
    for g, R in enumerate(RATIOS):
        b = [1 << 24]
        while len(b) < 511:                                       # b_0 .. b_510
            b.append((b[-1] * R) >> 8)
        u = [b[(z + 1) >> 1] for z in range(ALPHABET)]
        c = [1 + ((65536 - ALPHABET) * v) // sum(u) for v in u]
        c[0] += 65536 - sum(c)
        cdf = [0]
        for v in c:
            cdf.append(cdf[-1] + v)
        out[g] = [v & 0xFFFF for v in cdf]
    return out


def pairs(k, ctx, rows, D):
    """k [3][n], ctx [n], rows uint16 [3 D][1022] -> c_low | c_high << 16 in payload order: the Y block, then Co, then Cg."""
    return [int(rows[ch * D + c][symbol(kk)]) | (int(rows[ch * D + c][symbol(kk) + 1]) << 16) for ch in range(3) for kk, c in zip(k[ch], ctx)]


def payload_contexts(ctx, D):
    """The context channel * D + (level - 1) of every symbol of a payload."""
    return [ch * D + c for ch in range(3) for c in ctx]
