"""The hard trees of the reflectance layer's tests (host only): every case is dict(D, leaves int32 [U,3] in Morton order, a uint8 [U])
and, for the leaf-value cases, q int32 [P,3] / r float32 [P] / scale.  Built once per process and never modified."""
import functools

import numpy as np

import attr_ref


def _sorted(leaves, D):
    leaves = np.asarray(leaves, np.int32).reshape(-1, 3)
    order = sorted(range(len(leaves)), key=lambda i: attr_ref.morton(leaves[i], D))
    return np.ascontiguousarray(leaves[order])


def _case(D, leaves, a):
    leaves = np.asarray(leaves, np.int32).reshape(-1, 3)
    a = np.asarray(a, np.uint8)
    assert len(a) == len(leaves)
    for arr in (leaves, a):
        arr.setflags(write=False)
    return dict(D=D, leaves=leaves, a=a)


def random_points_case(seed=5):
    """2 000 random leaves at D = 12 under 6 000 points: 500 leaves with two points on the half (v, v + 1), 500 with three points (thirds),
    1 000 with one; 1 500 points in no leaf (other cells, negative and too large coordinates); 500 more points on random leaves whose
    reflectance is NaN, infinite, negative or above 1."""
    rng = np.random.default_rng(seed)
    D, U = 12, 2000
    cells = np.unique(rng.integers(0, 1 << D, size=(U + 1600, 3), dtype=np.int64), axis=0)
    cells = cells[rng.permutation(len(cells))]
    leaves, spare = _sorted(cells[:U], D), cells[U:U + 1500].astype(np.int32)
    base = rng.integers(0, 255, size=U)
    q, r = [], []
    for i in range(U):
        vals = [base[i], base[i] + 1] if i < 500 else ([base[i], base[i], base[i] + 1 + (i & 1)] if i < 1000 else [base[i]])
        for v in vals:
            q.append(leaves[i])
            r.append(min(int(v), 255) / 255.0)
    spare[:50, 0] = -1 - spare[:50, 0]                 # negative coordinates
    spare[50:100, 2] += 1 << D                         # beyond the cube
    q += list(spare)
    r += list(rng.uniform(0, 1, size=len(spare)))
    odd = [np.nan, np.inf, -np.inf, -0.25, 1.5, 3e38, -3e38, 1.0 + 1e-3]
    for t in range(6000 - len(q)):
        q.append(leaves[int(rng.integers(0, U))])
        r.append(odd[t % len(odd)])
    q, r = np.asarray(q, np.int32), np.asarray(r, np.float32)
    assert q.shape == (6000, 3)
    p = rng.permutation(len(q))
    q, r = np.ascontiguousarray(q[p]), np.ascontiguousarray(r[p])
    a, cnt = attr_ref.leaf_values(q, r, leaves, D, 255)
    assert min(cnt) >= 1
    c = _case(D, leaves, a)
    q.setflags(write=False)
    r.setflags(write=False)
    c.update(q=q, r=r, scale=255, cnt=np.asarray(cnt, np.int32))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(11)
    out = {}
    out["single"] = _case(4, [[3, 5, 1]], [77])
    for axis in range(3):                                  # two leaves that differ in the top bit of one axis only, D = 3
        hi = [0, 0, 0]
        hi[axis] = 4
        out[f"axis{axis}"] = _case(3, [[1, 2, 3], [1 + hi[0], 2 + hi[1], 3 + hi[2]]], [10, 201])
    cube = _sorted([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], 2)
    out["full_255_first"] = _case(2, cube, [255, 0] * 4)   # d = -255 in every stage-1 pair: z = 510
    out["full_0_first"] = _case(2, cube, [0, 255] * 4)
    # the full parent (weight 8) beside one leaf of value 0: d < 0 with W = 9 one level up
    out["full_plus_one"] = _case(2, np.concatenate([cube, [[0, 0, 2]]]), [255, 0] * 4 + [0])
    x, y, z = (int(v) for v in rng.integers(0, 1 << 21, size=3))
    out["chain21"] = _case(21, _sorted([[x, y, z & ~1], [x, y, z | 1]], 21), [3, 250])
    block = [[x, y, z] for x in range(16) for y in range(16) for z in range(16)]
    singles = [[16 * bx + int(rng.integers(0, 16)), 16 * by + int(rng.integers(0, 16)), 16 * bz + int(rng.integers(0, 16))]
               for bx in (0, 1) for by in (0, 1) for bz in (0, 1) if bx + by + bz]
    heavy = _sorted(block + singles, 5)
    out["heavy"] = _case(5, heavy, rng.integers(0, 256, size=len(heavy)))
    out["random"] = random_points_case()
    return out


QS = (1, 8, 255)
