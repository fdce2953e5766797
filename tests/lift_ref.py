"""The lifting of both attribute layers once more, as whole-array NumPy over C value planes: what attr_ref.py and color_ref.py
state parent by parent in Python integers, stated level by level on dense [parents, 8] slot tables, so that it can be evaluated on trees of
10^5 .. 10^6 leaves.  tests/test_lift_ref.py ties it to the two plain definitions field for field; the GPU tests at scale take their
expected values from here.  Nothing looks like the kernels: a level's parents come from a head mask and its cumsum, children are scattered
to their slots, the three stages run over the 7 fixed pairs as array operations, and the coding order falls out of a row-major boolean
selection over [parents, 7] - no tile scans, no offsets derived from first[], no clamped counts.  Everything is int64."""
import numpy as np

STAGES = ((1, 1), (2, 2), (3, 4))                       # (stage, bit): axis 2, then axis 1, then axis 0
PAIRS = {bit: [(lo, lo | bit) for lo in range(8) if lo & bit == 0 and lo & (bit - 1) == 0] for _, bit in STAGES}
FORWARD = [(stage, lo, hi) for stage, bit in STAGES for lo, hi in PAIRS[bit]]          # the order in which pairs merge
CODING = [(stage, lo, hi) for stage in (3, 2, 1) for s, lo, hi in FORWARD if s == stage]  # the order of a parent's coefficients
ALPHABETS = {1: 511, 3: 1021}
_SQUARES = np.arange(362, dtype=np.int64) ** 2          # isqrt(x) for x <= 2 * 255^2 = 130 050 < 361^2


def morton(p, D):
    """int [n,3] -> int64 [n]: the D-digit keys, digit = 4 bx + 2 by + bz, the top bit first (below 2^63 for D <= 21)."""
    p = np.asarray(p, np.int64).reshape(-1, 3)
    k = np.zeros(len(p), np.int64)
    for b in range(D - 1, -1, -1):
        k = (k << 3) | (((p[:, 0] >> b) & 1) << 2) | (((p[:, 1] >> b) & 1) << 1) | ((p[:, 2] >> b) & 1)
    return k


def symbol(k):
    k = np.asarray(k, np.int64)
    return 2 * np.abs(k) - (k > 0)


def step(w1, w2, Q):
    """max(1, isqrt((Q Q (w1 + w2)) // (w1 w2))) on arrays; 1 where a weight is 0 (no pair there)."""
    w1, w2 = np.asarray(w1, np.int64), np.asarray(w2, np.int64)
    x = (int(Q) * int(Q) * (w1 + w2)) // np.maximum(w1 * w2, 1)
    return np.maximum(1, np.searchsorted(_SQUARES, x, side="right") - 1)


def rgb_to_ycc(rgb):
    """int [..., 3] -> int64 [3, ...]: YCoCg-R."""
    rgb = np.asarray(rgb, np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    co = r - b
    t = b + (co >> 1)
    cg = g - t
    return np.stack([t + (cg >> 1), co, cg])


def ycc_to_rgb(ycc):
    """int [3, n] -> int64 [n, 3], not clamped."""
    y, co, cg = (np.asarray(p, np.int64) for p in ycc)
    t = y - (cg >> 1)
    b = t - (co >> 1)
    return np.stack([b + co, cg + t, b], axis=-1)


def tree(leaves, D):
    """The levels of a Morton-ordered leaf list: a list over j = 1 .. D of dict(par int64 [n_(j-1)] - every child's parent -, slot int64
    [n_(j-1)], n - parents -, first int64 [n] - every parent's first child) and the level counts n_0 .. n_D."""
    key = morton(leaves, D)
    assert (key[1:] > key[:-1]).all(), "leaves are not in strict Morton order"
    levels, counts = [], [len(key)]
    for _ in range(D):
        pk = key >> 3
        head = np.ones(len(key), bool)
        head[1:] = pk[1:] != pk[:-1]
        levels.append(dict(par=np.cumsum(head) - 1, slot=key & 7, n=int(head.sum()), first=np.flatnonzero(head)))
        key = pk[head]
        counts.append(len(key))
    return levels, counts


def _slots(level, x):
    """x [..., children] -> [..., parents, 8], 0 in the empty slots."""
    out = np.zeros(x.shape[:-1] + (level["n"], 8), np.int64)
    out[..., level["par"], level["slot"]] = x
    return out


def _planes(x):
    """[n] or [C][n] -> int64 [C, n]."""
    x = np.asarray(x, np.int64)
    return x[None] if x.ndim == 1 else x


def forward(leaves, vals, D, Q, alphabet=None):
    """vals int [C][U] -> dict(k int64 [C, U - 1] and ctx int64 [U - 1] (level - 1) in coding order, root int64 [C], hist int64 [C D,
    alphabet] (row channel * D + level - 1), level_counts [D + 1]); alphabet: 511 for one plane, 1021 for three unless given."""
    v = _planes(vals)
    C, U = v.shape
    alphabet = alphabet or ALPHABETS[C]
    if U == 0:
        return dict(k=np.zeros((C, 0), np.int64), ctx=np.zeros(0, np.int64), root=np.zeros(C, np.int64),
                    hist=np.zeros((C * D, alphabet), np.int64), level_counts=[0] * (D + 1))
    levels, counts = tree(leaves, D)
    w = np.ones(U, np.int64)
    blocks = {}
    for j, lv in enumerate(levels, 1):
        W, V = _slots(lv, w), _slots(lv, v)
        coef, both = {}, {}
        for stage, lo, hi in FORWARD:
            wl, wh = W[:, lo], W[:, hi]
            pair = (wl > 0) & (wh > 0)
            d = V[:, :, hi] - V[:, :, lo]
            s = step(wl, wh, Q)
            mag = (np.abs(d) + (s >> 1)) // s
            coef[stage, lo], both[stage, lo] = np.where(d > 0, mag, -mag), pair
            mean = V[:, :, lo] + (wh * d) // np.maximum(wl + wh, 1)
            V[:, :, lo] = np.where(pair, mean, np.where(wh > 0, V[:, :, hi], V[:, :, lo]))
            W[:, lo] = wl + wh
            W[:, hi] = 0
        sel = np.stack([both[stage, lo] for stage, lo, _ in CODING], axis=-1)             # [parents, 7]
        blocks[j] = np.stack([coef[stage, lo] for stage, lo, _ in CODING], axis=-1)[:, sel]   # parent-major, then the coding order
        v, w = V[:, :, 0], W[:, 0]
    k = np.concatenate([blocks[j] for j in range(D, 0, -1)], axis=1)
    ctx = np.concatenate([np.full(blocks[j].shape[1], j - 1, np.int64) for j in range(D, 0, -1)])
    hist = np.stack([np.bincount(symbol(blocks[j][ch]), minlength=alphabet) for ch in range(C) for j in range(1, D + 1)])
    assert hist.shape == (C * D, alphabet) and k.shape == (C, U - 1)
    return dict(k=k, ctx=ctx, root=v[:, 0].copy(), hist=hist, level_counts=counts)


def inverse(leaves, D, Q, root, k):
    """root int [C], k int [C, U - 1] in coding order -> int64 [C, U]: the leaf values before the layer's clamp.  The plan of every
    parent is rebuilt from the weights alone and undone level by level, D .. 1."""
    k = _planes(k)
    C = k.shape[0]
    if len(leaves) == 0:
        return np.zeros((C, 0), np.int64)
    levels, counts = tree(leaves, D)
    assert k.shape[1] == counts[0] - 1
    w, plans = np.ones(counts[0], np.int64), []
    for lv in levels:                                           # upwards: the weights every pair had when it merged
        W, plan = _slots(lv, w), {}
        for stage, lo, hi in FORWARD:
            plan[stage, lo] = (W[:, lo].copy(), W[:, hi].copy())
            W[:, lo] += W[:, hi]
            W[:, hi] = 0
        plans.append(plan)
        w = W[:, 0]
    v = np.asarray(root, np.int64).reshape(C, 1)
    pos = 0
    for j in range(D, 0, -1):
        lv, plan = levels[j - 1], plans[j - 1]
        assert pos == counts[j] - 1
        sel = np.stack([(plan[stage, lo][0] > 0) & (plan[stage, lo][1] > 0) for stage, lo, _ in CODING], axis=-1)
        n = int(sel.sum())
        K = np.zeros((C, lv["n"], 7), np.int64)
        K[:, sel] = k[:, pos:pos + n]
        pos += n
        V = np.zeros((C, lv["n"], 8), np.int64)
        V[:, :, 0] = v
        for stage, lo, hi in reversed(FORWARD):
            wl, wh = plan[stage, lo]
            dh = K[:, :, CODING.index((stage, lo, hi))] * step(wl, wh, Q)
            low = V[:, :, lo] - (wh * dh) // np.maximum(wl + wh, 1)
            pair, moved = (wl > 0) & (wh > 0), (wl == 0) & (wh > 0)
            V[:, :, hi] = np.where(pair, low + dh, np.where(moved, V[:, :, lo], V[:, :, hi]))
            V[:, :, lo] = np.where(pair, low, V[:, :, lo])
        v = V[:, lv["par"], lv["slot"]]
    assert pos == k.shape[1]
    return v


def inverse_reflectance(leaves, D, Q, root, k):
    """-> int64 [U], clamped to 0 .. 255."""
    return np.clip(inverse(leaves, D, Q, [root], [k])[0], 0, 255)


def inverse_rgb(leaves, D, Q, root, k):
    """root [3] (Y, Co, Cg), k [3, U - 1] -> int64 [U, 3]: R, G, B clamped to 0 .. 255 after the inverse colour transform."""
    return np.clip(ycc_to_rgb(inverse(leaves, D, Q, root, k)), 0, 255)


def pairs(k, ctx, rows):
    """k int [C, n] (or [n]), ctx int [n], rows uint16 [C D, alphabet + 1] -> uint32 [C n]: c_low | c_high << 16 in payload order."""
    k = _planes(k)
    C = k.shape[0]
    rows = np.asarray(rows).astype(np.int64)
    row = (np.arange(C) * (rows.shape[0] // C))[:, None] + np.asarray(ctx, np.int64)[None, :]
    z = symbol(k)
    return (rows[row, z] | (rows[row, z + 1] << 16)).astype(np.uint32).reshape(-1)


def _leaf_of(q, leaves, D):
    """-> (point indices that fall in a leaf, their leaves)."""
    q = np.asarray(q, np.int64).reshape(-1, 3)
    inside = np.flatnonzero(((q >= 0) & (q < (1 << D))).all(axis=1))
    keys = morton(leaves, D)
    if len(keys) == 0:
        return inside[:0], inside[:0]
    qk = morton(q[inside], D)
    at = np.minimum(np.searchsorted(keys, qk), len(keys) - 1)
    hit = keys[at] == qk
    return inside[hit], at[hit]


def _rounded_mean(total, cnt):
    return np.where(cnt > 0, (2 * total + cnt) // np.maximum(2 * cnt, 1), 0)


def point_values(r, scale):
    """float32 [P] -> int64 [P]: clamp(floor(double(r) * scale + 0.5), 0, 255), 0 for a non-finite r."""
    r = np.asarray(r, np.float32).astype(np.float64)
    fin = np.isfinite(r)
    return np.where(fin, np.clip(np.floor(np.where(fin, r, 0.0) * float(scale) + 0.5), 0.0, 255.0), 0.0).astype(np.int64)


def leaf_values(q, r, leaves, D, scale):
    """The reflectance layer's -> (a int64 [U], cnt int64 [U]); a leaf no point hits has a = 0, cnt = 0."""
    pts, at = _leaf_of(q, leaves, D)
    U = len(leaves)
    total = np.zeros(U, np.int64)
    np.add.at(total, at, point_values(r, scale)[pts])
    cnt = np.bincount(at, minlength=U).astype(np.int64)
    return _rounded_mean(total, cnt), cnt


def leaf_colors(q, rgb8, leaves, D):
    """The colour layer's -> (rgb_mean int64 [U, 3], ycc int64 [3, U], cnt int64 [U])."""
    pts, at = _leaf_of(q, leaves, D)
    U = len(leaves)
    total = np.zeros((U, 3), np.int64)
    np.add.at(total, at, np.asarray(rgb8, np.int64).reshape(-1, 3)[pts])
    cnt = np.bincount(at, minlength=U).astype(np.int64)
    mean = _rounded_mean(total, cnt[:, None])
    return mean, rgb_to_ycc(mean), cnt
