"""Stream-sized and edge-placed trees for both attribute layers (host only): what tests/attr_cases.py and tests/color_cases.py cannot hold,
because the plain references take seconds per 10^5 leaves.  Every tree is dict(D, leaves int32 [U,3] in Morton order, a uint8 [U] - the
reflectance layer's values -, rgb uint8 [U,3] and ycc int64 [3,U] - the colour layer's); every builder asserts, on the host, the property
its tree exists for, so that an edit that loses the property fails here and not silently on the GPU.  Built once per process and never
modified.  The kernels' constants that the trees aim at: a tile of 1024 entries (256 threads of 4 items) and a scan chunk of 256 tiles."""
import functools

import numpy as np

import attr_ref
import lift_ref
from color_cases import BLUE, GREEN, MAGENTA, RED

ITEMS, TILE, CHUNK = 4, 1024, 256 * 1024
TILE_PREFIXES = (1023, 1024, 1025, 2049)
CHUNK_PREFIXES = (CHUNK - 1, CHUNK, CHUNK + 1)


def _case(D, cells, a, rgb):
    """Cells in any order -> the case, in Morton order."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    order = np.argsort(lift_ref.morton(cells, D), kind="stable")
    leaves = np.ascontiguousarray(cells[order], np.int32)
    a = np.ascontiguousarray(np.asarray(a)[order], np.uint8)
    rgb = np.ascontiguousarray(np.asarray(rgb)[order], np.uint8)
    ycc = lift_ref.rgb_to_ycc(rgb)
    for arr in (leaves, a, rgb, ycc):
        arr.setflags(write=False)
    return dict(D=D, leaves=leaves, a=a, rgb=rgb, ycc=ycc)


def prefix(c, U):
    """The first U leaves of a case: a prefix of a Morton-ordered set is one."""
    return dict(D=c["D"], leaves=c["leaves"][:U], a=c["a"][:U], rgb=c["rgb"][:U], ycc=c["ycc"][:, :U])


def _families(first, n):
    """first [parents] of a level over n entries -> (start, end) of every family, end exclusive."""
    return first, np.append(first[1:], n)


def _straddled(first, n, edge):
    """Does a family of the level hold entries on both sides of `edge` (a child at edge - 1 and one at edge)?"""
    b, e = _families(first, n)
    return bool(((b < edge) & (e > edge)).any())


@functools.lru_cache(maxsize=None)
def sparse():
    """270 000 distinct random cells at D = 10 with random values: levels 0, 1 and 2 count more than 262 144 entries, so the one-block
    scan of the block sums takes a second trip with a carry on three levels, and parents' offsets (n_j - 1) + first[p] - p run to 5 10^5."""
    rng = np.random.default_rng(31)
    cells = np.unique(rng.integers(0, 1 << 10, size=(275000, 3), dtype=np.int64), axis=0)
    assert len(cells) >= 270000
    cells = cells[rng.permutation(len(cells))[:270000]]
    c = _case(10, cells, rng.integers(0, 256, size=270000), rng.integers(0, 256, size=(270000, 3)))
    levels, counts = lift_ref.tree(c["leaves"], 10)
    assert counts[0] == 270000 and min(counts[:3]) > CHUNK and counts[-1] == 1, counts
    c["level_counts"] = counts
    return c


@functools.lru_cache(maxsize=None)
def sparse_level1_prefixes():
    """The two prefixes of `sparse` whose level 1 counts exactly 262 144 and 262 145 entries (the count grows by 0 or 1 per leaf): the
    first leaf list with that many parents each."""
    c = sparse()
    heads = np.cumsum(np.r_[True, np.diff(lift_ref.morton(c["leaves"], 10) >> 3) != 0])     # level-1 count of the prefix of i + 1 leaves
    out = tuple(int(np.searchsorted(heads, n)) + 1 for n in (CHUNK, CHUNK + 1))
    for U, n in zip(out, (CHUNK, CHUNK + 1)):
        assert heads[U - 1] == n and heads[U - 2] == n - 1 and U > CHUNK + 1
    return out


PREFIXES = tuple(f"sparse[:{U}]" for U in TILE_PREFIXES + CHUNK_PREFIXES) + ("sparse[level1=262144]", "sparse[level1=262145]")


def prefix_length(name):
    """The U of a name of PREFIXES; the two level-1 prefixes are found when first asked for."""
    if name.startswith("sparse[:"):
        return int(name[8:-1])
    return sparse_level1_prefixes()[PREFIXES[-2:].index(name)]


@functools.lru_cache(maxsize=None)
def sphere():
    """The voxels within 0.5 of a sphere of radius 150 around (256, 256, 256) at D = 9: an object-shaped shell with 3 to 4 children per
    parent.  Reflectance: a smooth field, noise, and salt and pepper on one leaf in 16.  Colours: a smooth field, and in four of eight
    azimuth sectors the saturated pairs RED / BLUE, BLUE / RED, GREEN / MAGENTA, MAGENTA / GREEN by the parity of z, so that stage-1 pairs
    reach d = -510 and +510 in Co and Cg."""
    rng = np.random.default_rng(41)
    g = np.arange(256 - 151, 256 + 152, dtype=np.int32)
    d2 = ((g - 256) ** 2)[:, None, None] + ((g - 256) ** 2)[None, :, None] + ((g - 256) ** 2)[None, None, :]
    cells = np.argwhere((4 * d2 >= 299 ** 2) & (4 * d2 <= 301 ** 2)).astype(np.int64) + int(g[0])      # 149.5 <= r <= 150.5
    n = len(cells)
    x, y, z = (cells[:, i].astype(np.float64) for i in range(3))
    smooth = 128 + 90 * np.sin(x / 40.0) * np.cos(y / 30.0) + 30 * np.sin(z / 25.0)
    a = np.clip(np.rint(smooth + rng.normal(0, 6, size=n)), 0, 255)
    salt = rng.integers(0, 16, size=n) == 0
    a[salt] = rng.integers(0, 2, size=int(salt.sum())) * 255
    rgb = np.clip(np.rint(np.stack([smooth, 128 + 100 * np.cos(x / 35.0 + z / 50.0), 128 + 100 * np.sin(y / 45.0 - z / 20.0)], axis=1)
                          + rng.normal(0, 4, size=(n, 3))), 0, 255).astype(np.int64)
    sector = (np.floor((np.arctan2(y - 256, x - 256) + np.pi) / (np.pi / 4)).astype(np.int64)) % 8
    odd = (cells[:, 2] & 1).astype(bool)
    for s, (even_c, odd_c) in ((1, (RED, BLUE)), (3, (BLUE, RED)), (5, (GREEN, MAGENTA)), (7, (MAGENTA, GREEN))):
        rgb[(sector == s) & ~odd] = even_c
        rgb[(sector == s) & odd] = odd_c
    c = _case(9, cells, a, rgb)
    levels, counts = lift_ref.tree(c["leaves"], 9)
    assert 250000 < counts[0] < 300000 and 2.5 < counts[0] / counts[1] < 4.5, counts
    f = lift_ref.forward(c["leaves"], c["ycc"], 9, 1)
    for ch in (1, 2):                                       # Co and Cg: both ends of the alphabet
        assert f["hist"][ch * 9:(ch + 1) * 9, 1019].sum() > 0 and f["hist"][ch * 9:(ch + 1) * 9, 1020].sum() > 0, ch
    # Q = 255: the inverse leaves 0 .. 255 on more than 1 000 leaves before the clamp, in both layers
    g1 = lift_ref.forward(c["leaves"], c["a"], 9, 255)
    back = lift_ref.inverse(c["leaves"], 9, 255, g1["root"], g1["k"])[0]
    assert int(((back < 0) | (back > 255)).sum()) > 1000
    f = lift_ref.forward(c["leaves"], c["ycc"], 9, 255)
    back = lift_ref.ycc_to_rgb(lift_ref.inverse(c["leaves"], 9, 255, f["root"], f["k"]))
    assert int(((back < 0) | (back > 255)).any(axis=1).sum()) > 1000
    c["level_counts"] = counts
    return c


@functools.lru_cache(maxsize=None)
def dense_plus():
    """The full 64^3 block at D = 7 plus the leaf (64, 0, 0), value 0: weights double up to 262 144, and the top pair is (262 144, 1) with
    d < 0 - attr_cases' full_plus_one at the size where the step's quotient floors to 0 and W = 2^18 + 1 divides a negative product."""
    rng = np.random.default_rng(43)
    g = np.arange(64, dtype=np.int64)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    cells = np.concatenate([cells, [[64, 0, 0]]])
    a = np.append(rng.integers(1, 256, size=1 << 18), 0)
    rgb = np.concatenate([rng.integers(0, 256, size=(1 << 18, 3)), [BLUE]])
    rgb[: 1 << 17, 0] |= 128                                # mean R - B > 0 in the block, Co = -255 on the lone leaf
    c = _case(7, cells, a, rgb)
    assert (c["leaves"][-1] == (64, 0, 0)).all() and c["a"][-1] == 0
    levels, counts = lift_ref.tree(c["leaves"], 7)
    assert counts == [262145, 32769, 4097, 513, 65, 9, 2, 1], counts
    for Q in (1, 8, 255):
        assert attr_ref.step(1 << 18, 1, Q) == Q == int(lift_ref.step(1 << 18, 1, Q))
        for w in (1 << e for e in range(19)):
            if w > 2 * Q * Q:
                assert attr_ref.step(w, w, Q) == 1 == int(lift_ref.step(w, w, Q))
    assert (1 << 17) > 2 * 255 * 255                        # the block's last stage merges (131 072, 131 072): step 1 at every Q
    assert 510 * (1 << 18) < 1 << 31                        # wh * d itself stays below 32 bits here: that takes weights beyond 2^22
    c["level_counts"] = counts
    return c


@functools.lru_cache(maxsize=None)
def shifted():
    """Three lone leaves in three level-3 cells of the first octant, then a dense 16^3 block in octant 4, D = 5: on levels 0 .. 3 every
    family of 8 of the block starts at entry 8 m + 3, across every 4-item group, and three of them across the tile edges 1024, 2048 and 3072."""
    rng = np.random.default_rng(47)
    g = np.arange(16, dtype=np.int64)
    block = np.stack(np.meshgrid(g + 16, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    cells = np.concatenate([[[0, 0, 0], [0, 0, 8], [0, 8, 0]], block])
    c = _case(5, cells, rng.integers(0, 256, size=len(cells)), rng.integers(0, 256, size=(len(cells), 3)))
    levels, counts = lift_ref.tree(c["leaves"], 5)
    assert counts == [4099, 515, 67, 11, 2, 1], counts
    assert levels[3]["first"].tolist() == [0, 3]               # level 3: the three lone cells are one family, the block's 8 start at 3
    for j in range(3):
        first = levels[j]["first"]
        assert first[:3].tolist() == [0, 1, 2] and (first[3:] % 8 == 3).all() and (np.diff(first[3:]) == 8).all()
        assert (first[3:] % ITEMS != 0).all() and ((first[3:] + 7) // ITEMS - first[3:] // ITEMS == 2).all()        # three thread groups each
    for edge in (1024, 2048, 3072):
        assert _straddled(levels[0]["first"], counts[0], edge)
    c["level_counts"] = counts
    return c


@functools.lru_cache(maxsize=None)
def deep():
    """The first 1 025 leaves, in Morton order, of 1 000 random cells at D = 21 and a sibling of each: 63-bit keys (bit 20 of x is set
    on three cells in four of the draw) through 21 levels, one entry past a tile, coefficients at the bottom and at the top."""
    rng = np.random.default_rng(53)
    base = rng.integers(0, 1 << 20, size=(1000, 3), dtype=np.int64)
    base[:, 0] |= (rng.integers(0, 4, size=1000) > 0).astype(np.int64) << 20
    base[:, 1] |= rng.integers(0, 2, size=1000, dtype=np.int64) << 20
    base[:, 2] |= rng.integers(0, 2, size=1000, dtype=np.int64) << 20
    sib = base.copy()
    sib[np.arange(1000), rng.integers(0, 3, size=1000)] ^= 1
    cells = np.unique(np.concatenate([base, sib]), axis=0)
    assert len(cells) == 2000
    keys = lift_ref.morton(cells, 21)
    cells = cells[np.argsort(keys)[:TILE + 1]]
    c = _case(21, cells, rng.integers(0, 256, size=len(cells)), rng.integers(0, 256, size=(len(cells), 3)))
    keys = lift_ref.morton(c["leaves"], 21)
    assert len(keys) == TILE + 1 and int(keys[-1]) >= 1 << 62 and (c["leaves"] >> 20).any(axis=0).all() and int(keys[0]) < 1 << 60
    assert keys.tolist() == [attr_ref.morton(p, 21) for p in c["leaves"]]
    levels, counts = lift_ref.tree(c["leaves"], 21)
    assert counts[1] < counts[0] and counts[-1] == 1 and counts[20] > 1
    c["level_counts"] = counts
    return c


BUILDERS = dict(sparse=sparse, sphere=sphere, dense_plus=dense_plus, shifted=shifted, deep=deep)
SMALL = ("shifted", "deep")                                 # below 5 000 leaves: every Q of attr_cases.QS; the others Q = 1 and 255


def case(name):
    """A tree by name: a builder's, or a prefix `sparse[:U]`."""
    if name in BUILDERS:
        return BUILDERS[name]()
    assert name in PREFIXES, name
    return prefix(sparse(), prefix_length(name))


NAMES = tuple(BUILDERS) + PREFIXES


@functools.lru_cache(maxsize=None)
def sphere_points():
    """One million points over the leaves of `sphere` for the leaf values of both layers: 300 000 on one leaf whose values alternate
    v, v + 1 (the mean an exact half, which rounds up; per colour channel the phase differs), 100 000 on a second leaf, all 255, 50 000 in
    no leaf (empty cells three voxels from a leaf, negative coordinates, coordinates >= 2^D), the rest one to three per leaf until they run
    out, so that the last leaves hold none.  -> dict(q int32 [P,3], r float32 [P], scale, rgb8 uint8 [P,3], half, full - the two leaves)."""
    rng = np.random.default_rng(59)
    c = sphere()
    leaves, D, U = c["leaves"].astype(np.int64), c["D"], len(c["leaves"])
    half, full, v = U // 3, (2 * U) // 3, 100
    away = leaves[rng.integers(0, U, size=60000)] + (3, 0, 0)
    keys = lift_ref.morton(leaves, D)
    at = np.minimum(np.searchsorted(keys, lift_ref.morton(away, D)), U - 1)
    away = away[(keys[at] != lift_ref.morton(away, D)) & (away < 1 << D).all(axis=1)][:30000]
    assert len(away) == 30000
    below = leaves[rng.integers(0, U, size=10000)] * (1, 1, -1) - (0, 0, 1)
    above = leaves[rng.integers(0, U, size=10000)] + (0, 1 << D, 0)
    rest = np.setdiff1d(np.arange(U), [half, full])
    per_leaf = np.arange(len(rest)) % 3 + 1
    spread = np.repeat(rest, per_leaf)[:550000]
    assert len(spread) == 550000 and spread[-1] < rest[-1]
    q = np.concatenate([np.repeat(leaves[[half]], 300000, axis=0), np.repeat(leaves[[full]], 100000, axis=0), away, below, above, leaves[spread]])
    val = np.concatenate([v + (np.arange(300000) & 1), np.full(100000, 255), rng.integers(0, 256, size=50000 + 550000)])
    rgb8 = np.concatenate([v + ((np.arange(300000)[:, None] + np.arange(3)) & 1), np.full((100000, 3), 255), rng.integers(0, 256, size=(600000, 3))])
    assert len(q) == len(val) == len(rgb8) == 1000000
    p = rng.permutation(len(q))
    out = dict(q=np.ascontiguousarray(q[p], np.int32), r=np.ascontiguousarray(val[p] / 255.0, np.float32), scale=255,
               rgb8=np.ascontiguousarray(rgb8[p], np.uint8), half=half, full=full)
    assert lift_ref.point_values(out["r"], 255).tolist() == val[p].tolist()          # v / 255 in float32 comes back as v
    for arr in (out["q"], out["r"], out["rgb8"]):
        arr.setflags(write=False)
    return out
