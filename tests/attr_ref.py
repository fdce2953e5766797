"""The reflectance layer's definition ("Reflectance") in plain Python integers: a dict of slots per parent, as the prose
reads.  Nothing here looks like the kernels (no scans, no coding-order offsets, no register plans): the coding order is obtained by
collecting every level's coefficients parent by parent and listing the levels D .. 1."""
import math

import numpy as np

ALPHABET = 511
RATIOS = [32, 64, 96, 128, 152, 176, 192, 208, 216, 224, 232, 238, 243, 247, 250, 253]
STAGES = ((1, 1), (2, 2), (3, 4))            # (stage, bit): axis 2, then axis 1, then axis 0


def morton(p, D):
    """D-digit key of an integer position, digit = 4 bx + 2 by + bz, the top bit first."""
    x, y, z = (int(c) for c in p)
    k = 0
    for b in range(D - 1, -1, -1):
        k = (k << 3) | (((x >> b) & 1) << 2) | (((y >> b) & 1) << 1) | ((z >> b) & 1)
    return k


def point_value(r, scale):
    r = float(np.float32(r))
    if not math.isfinite(r):
        return 0
    return int(min(255.0, max(0.0, math.floor(r * float(scale) + 0.5))))


def leaf_values(q, r, leaves, D, scale):
    """-> (a [U], cnt [U]) as Python lists; a leaf no point hits has a = 0, cnt = 0."""
    index = {tuple(int(c) for c in lv): i for i, lv in enumerate(leaves)}
    s, n = [0] * len(leaves), [0] * len(leaves)
    for p, rp in zip(q, r):
        i = index.get(tuple(int(c) for c in p))
        if i is not None:
            s[i] += point_value(rp, scale)
            n[i] += 1
    return [((2 * si + ni) // (2 * ni)) if ni else 0 for si, ni in zip(s, n)], n


def step(w1, w2, Q):
    return max(1, math.isqrt((Q * Q * (w1 + w2)) // (w1 * w2)))


def _pairs(bit):
    return [(lo, lo | bit) for lo in range(8) if lo & bit == 0 and lo & (bit - 1) == 0]


def _parents(level):
    """[(key, value, weight)] in order -> [(parent key, {slot: [value, weight]})] in order."""
    out = []
    for key, v, w in level:
        if not out or out[-1][0] != key >> 3:
            out.append((key >> 3, {}))
        out[-1][1][key & 7] = [v, w]
    return out


def forward(leaves, a, D, Q):
    """-> dict(k, ctx (level - 1), root, hist [D][511], level_counts [D + 1]); k and ctx in coding order."""
    level = [(morton(lv, D), int(v), 1) for lv, v in zip(leaves, a)]
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
                        d, W = vh - vl, wl + wh
                        m = vl + (wh * d) // W
                        s = step(wl, wh, Q)
                        k = (abs(d) + (s >> 1)) // s
                        emitted[stage].append(k if d > 0 else -k)
                        slots[lo] = [m, W]
                    else:
                        slots[lo] = slots[hi]
                    del slots[hi]
            assert list(slots) == [0]
            coefs += emitted[3] + emitted[2] + emitted[1]
            nxt.append((pk, slots[0][0], slots[0][1]))
        blocks[j] = coefs
        level = nxt
        counts.append(len(level))
    k, ctx = [], []
    for j in range(D, 0, -1):
        k += blocks[j]
        ctx += [j - 1] * len(blocks[j])
    hist = [[0] * ALPHABET for _ in range(D)]
    for kk, c in zip(k, ctx):
        hist[c][symbol(kk)] += 1
    root = level[0][1] if level else 0
    return dict(k=k, ctx=ctx, root=root, hist=hist, level_counts=counts)


def symbol(k):
    return 2 * abs(k) - (1 if k > 0 else 0)


def inverse(leaves, D, Q, root, k):
    """-> the leaf values [U], clamped to 0 .. 255."""
    if len(leaves) == 0:
        return []
    levels = [[(morton(lv, D), 0, 1) for lv in leaves]]
    for j in range(1, D + 1):                                       # the tree from the weights alone
        nxt = []
        for pk, slots in _parents(levels[-1]):
            nxt.append((pk, 0, sum(w for _, w in slots.values())))
        levels.append(nxt)
    counts = [len(lv) for lv in levels]
    values = {D: [root]}
    pos = 0
    for j in range(D, 0, -1):
        assert pos == counts[j] - 1
        out = []
        for (pk, slots), v in zip(_parents(levels[j - 1]), values[j]):
            w = {s: e[1] for s, e in slots.items()}
            ops = []                                                # the forward plan
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
            for stage in (3, 2, 1):                                 # the coding order inside a parent
                for op in ops:
                    if op[0] == stage and op[3]:
                        coef[op[:3]] = k[pos]
                        pos += 1
            val = {0: v}
            for stage, lo, hi, wl, wh in reversed(ops):
                if wl:
                    dh = coef[(stage, lo, hi)] * step(wl, wh, Q)
                    val[lo] = val[lo] - (wh * dh) // (wl + wh)
                    val[hi] = val[lo] + dh
                else:
                    val[hi] = val.pop(lo)
            out += [val[s] for s in sorted(slots)]
        values[j - 1] = out
    assert pos == len(k)
    return [min(255, max(0, v)) for v in values[0]]


def tables():
    """uint16 [16][512]: the cdf rows, the last entry (65536) wrapped to 0."""
    out = np.zeros((len(RATIOS), ALPHABET + 1), np.uint16)
    for g, R in enumerate(RATIOS):
        b = [1 << 24]
        while len(b) < 257:
            b.append((b[-1] * R) >> 8)
        u = [b[(z + 1) >> 1] for z in range(ALPHABET)]
        c = [1 + ((65536 - ALPHABET) * v) // sum(u) for v in u]
        c[0] += 65536 - sum(c)
        cdf = [0]
        for v in c:
            cdf.append(cdf[-1] + v)
        out[g] = [v & 0xFFFF for v in cdf]
    return out


def pairs(k, ctx, rows):
    """rows uint16 [D][512] -> c_low | c_high << 16 per coefficient (c_high = 65536 stored as 0)."""
    return [int(rows[c][symbol(kk)]) | (int(rows[c][symbol(kk) + 1]) << 16) for kk, c in zip(k, ctx)]
