"""Integer clouds of the context-table tests (tests/test_ctx_cases.py checks on the CPU, through the oracle alone, that every case still
has the edge it is named for; tests/test_gpu_context.py runs the device on them).  Pure numpy: each case is the smallest tree that
still has its edge.

A case is one Geom.build call: a list of segments (integer cloud, rho-shell path or None, drop_last), the position mode of the EHEM
tables and the lidar_level of the level clip (encode_dataset_ehem.py:86)."""
import collections
import functools

import numpy as np

MINMAX, MUL, POW2 = "minmax", "mul", "pow2"             # native.POS_MINMAX / POS_MINMAX_MUL / POS_POW2
PATHS = {"00": [0, 0], "01": [0, 1], "1": [1]}
CONTEXT_SIZES = (2, 3, 5, 256, 8192)
GRID_ROWS = 2048 * 256                                   # rows one trip of ctx_ehem_all_kernel's grid-stride loop covers

Seg = collections.namedtuple("Seg", "pts path drop")
Case = collections.namedtuple("Case", "name segs mode lidar_level tags")


def _pts(rows):
    a = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1, 3))
    a.setflags(write=False)
    return a


def _case(name, segs, mode, lidar_level, *tags):
    return Case(name, tuple(Seg(_pts(p), None if path is None else list(path), bool(drop)) for p, path, drop in segs), mode, lidar_level,
                frozenset(tags))


def shell_point(depth, tag, diagonal):
    """A cloud of which the rho shell `tag` keeps ONE point, in a tree of `depth` levels: the kept point and, where that point alone would
    give a shallower tree, a point at x = 2^depth - 1 that fixes the depth and that the path filters out.  diagonal: x == y == z."""
    lo = {"00": 1 << (depth - 3), "01": 1 << (depth - 2), "1": 1 << (depth - 1)}[tag]
    x = lo + 5
    p = [x, x, x] if diagonal else [x, (x * 5 + 3) % (1 << (depth - 1)), 2]
    return [p] if tag == "1" else [p, [(1 << depth) - 1, 0, 0]]


def line2(n, axis_mix=True):
    """n points two apart: the deepest level of the tree has n nodes, the one above about n / 2, ..."""
    i = np.arange(n, dtype=np.int64)
    return np.stack([2 * i, (2 * i[::-1]) % 7 if axis_mix else 0 * i, (i * i) % 5 if axis_mix else 0 * i], 1)


@functools.lru_cache(maxsize=None)
def octree_recipe():
    """The clouds of tests/test_gpu_geom.py::test_octree_random_vs_oracle, by point count (the same generator, drawn in the same order)."""
    rng = np.random.default_rng(7)
    out = {}
    for n, hi in ((1, 5), (17, 3), (1000, 40), (30000, 5000), (200000, 9000)):
        pts = np.stack([rng.integers(0, hi, n), rng.integers(0, hi // 2 + 2, n), rng.integers(0, hi // 3 + 2, n)], 1)
        if pts.max() == 0:
            pts[0, 0] = 1
        out[n] = _pts(pts)
    return out


def skewed(n, hi, seed):
    """That recipe at another size (x up to hi, y up to hi / 2, z up to hi / 3)."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, hi, n), rng.integers(0, hi // 2 + 2, n), rng.integers(0, hi // 3 + 2, n)], 1)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    add = lambda *a: out.append(_case(*a))

    # ---- chains: one point, same-level mode (no path, nothing dropped): every level is a single node
    for tag, p in (("off", [37, 9, 2]), ("diag", [45, 45, 45])):
        for mode in (MINMAX, POW2):
            add(f"chain-{tag}-{mode}", [(p, None, False)], mode, 12, "chain", "single-node-levels", *(["diagonal"] if tag == "diag" else []))

    # ---- one-leaf shells (multi-level, drop_last): the last level holds the dropped node alone, the records end at depth - 1
    D = 6
    for tag in PATHS:
        for var, L in (("ge", D), ("ge1", D + 1), ("eq", D - 1), ("clip", 3)):
            add(f"oneleaf-{tag}-{var}", [(shell_point(D, tag, False), PATHS[tag], True)], MUL, L, "one-leaf", *(["clip"] if var == "clip" else []))
        add(f"oneleaf-{tag}-diag", [(shell_point(D, tag, True), PATHS[tag], True)], MUL, 3, "one-leaf", "clip", "nan")
    # the frame of the finding: two close points at depth 14, lidar_level 8
    add("oneleaf-close-pair-d14", [([[9000, 17, 5000], [9001, 17, 5000]], [1], True)], MUL, 8, "one-leaf", "clip")
    # a duplicated point is one leaf as well
    add("oneleaf-dup", [([[40, 3, 9]] * 3, [1], True)], MUL, 3, "one-leaf", "clip")

    # ---- the dropped node alone holds the last level's maximum / minimum
    add("dropped-owns-max", [([[8, 0, 0], [9, 1, 0], [15, 15, 15]], [1], True)], MUL, 12, "dropped-extreme", "last-two")
    add("dropped-owns-min", [([[8, 4, 4], [12, 0, 0]], [1], True)], MUL, 12, "dropped-extreme", "last-two")

    # ---- the last level has two nodes: one coded row behind the drop, with mx != mn and with mx == mn (0 / 0 without the epsilon)
    add("last-two-differ", [([[8, 2, 6], [14, 1, 1]], [1], True)], MUL, 3, "last-two")
    add("last-two-equal", [([[8, 8, 8], [15, 15, 15]], [1], True)], MUL, 12, "last-two", "nan")

    # ---- small, deep and duplicated clouds
    for mode in (MINMAX, POW2):
        add(f"depth1-{mode}", [([[0, 0, 1], [1, 0, 0], [1, 1, 1]], None, False)], mode, 12, "depth1")
    full = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    for mode in (MINMAX, POW2):
        add(f"full2-{mode}", [(full, None, False)], mode, 1, "full2")
    add("full2-mul-1", [(full, [1], True)], MUL, 2, "full2")
    add("full2-mul-none", [(full, None, True)], MUL, 1, "full2")
    # 19 levels is the deepest tree whose sort key keeps 6 segment bits; 20 and 21 (SCP_MAX_DEPTH) move the segment field of the key
    for d in (19, 20, 21):
        top = (1 << d) - 1
        two = [[top, top, top], [1 << (d - 1), 5, 123456]]
        for mode in (MINMAX, POW2):
            add(f"deep{d}-{mode}", [(two, None, False)], mode, 12, f"deep{d}")
        add(f"deep{d}-mul-1", [(two, [1], True)], MUL, 12, f"deep{d}")
    t20 = (1 << 20) - 1
    add("deep20-three", [([[5, t20, 9], [70000, 3, t20]], [0, 0], True), ([[300000, 8, 1], [400000, t20, 77], [t20, 0, 0]], [0, 1], True),
                         ([[t20, 1, 2], [600000, 600000, 600001], [5, 5, 5]], [1], True)], MUL, 12, "deep20", "deep-three")
    rng = np.random.default_rng(31)
    base = skewed(500, 300, 32)
    dup = np.concatenate([base, base[rng.integers(0, 500, 700)]])[rng.permutation(1200)]
    add("dup-shuffled-minmax", [(dup, None, False)], MINMAX, 12, "dup")
    add("dup-shuffled-mul-1", [(dup, [1], True)], MUL, 7, "dup")

    # ---- lidar_level below, equal to and above the depth, same-level mode
    small = skewed(200, 60, 33)                                              # depth 6
    for L in (3, 6, 9):
        add(f"lidar{L}-depth6", [(small, None, False)], MINMAX, L, "lidar-same-level")

    # ---- levels at the edges of the 256-thread tiles
    for n in (255, 256, 257):
        add(f"tile-{n}-minmax", [(line2(n), None, False)], MINMAX, 12, f"last-level-{n}")
        add(f"tile-{n}-pow2", [(line2(n), None, False)], POW2, 4, f"last-level-{n}")
        add(f"tile-{n}-mul", [(line2(n + 1), None, True)], MUL, 4, f"last-level-{n}")      # n coded rows behind the drop
    # a stem: levels 2 .. 5 stay a single node, level 6 has eight (same-level mode: encode.py:122 codes such levels out of place)
    stem = np.array([[32 + 2 * a, 2 * b, 2 * c] for a in range(2) for b in range(2) for c in range(2)])
    for mode in (MINMAX, POW2):
        add(f"stem-{mode}", [(stem, None, False)], mode, 4, "single-node-levels", "stem")

    # ---- random skewed clouds, three sizes, every path and none
    for n, hi, seed in ((300, 40, 41), (3000, 700, 42), (30000, 5000, 43)):
        pts = skewed(n, hi, seed)
        add(f"skew{n}-minmax", [(pts, None, False)], MINMAX, 12, "random")
        add(f"skew{n}-pow2", [(pts, None, False)], POW2, 5, "random")
        add(f"skew{n}-mul-none", [(pts, None, True)], MUL, 5, "random")
        for tag in PATHS:
            add(f"skew{n}-mul-{tag}", [(pts, PATHS[tag], True)], MUL, 8, "random")

    # ---- three shells in one build (the production layout); row_base / mm_base of a later segment follow a one-leaf one
    big, mid = skewed(3000, 5000, 44), skewed(2000, 9000, 45)
    leaf = shell_point(14, "00", False)
    add("three-leaf-first", [(leaf, [0, 0], True), (big, [0, 1], True), (mid, [1], True)], MUL, 8, "three", "one-leaf", "clip")
    add("three-leaf-middle", [(big, [0, 0], True), (shell_point(14, "01", False), [0, 1], True), (mid, [1], True)], MUL, 8, "three", "one-leaf", "clip")
    add("three-leaf-all", [(shell_point(D, t, False), PATHS[t], True) for t in PATHS], MUL, 3, "three", "one-leaf", "clip", "all-leaf")
    add("three-leaf-all-eq", [(shell_point(D, t, False), PATHS[t], True) for t in PATHS], MUL, D - 1, "three", "one-leaf", "all-leaf")
    add("three-leaf-all-ge", [(shell_point(D, t, False), PATHS[t], True) for t in PATHS], MUL, D, "three", "one-leaf", "all-leaf")
    add("three-leaf-all-diag", [(shell_point(D, t, True), PATHS[t], True) for t in PATHS], MUL, 3, "three", "one-leaf", "clip", "nan", "all-leaf")
    add("three-leaf-last-clip", [(mid, [0, 0], True), (big, [0, 1], True), (shell_point(14, "1", False), [1], True)], MUL, 8, "three", "one-leaf",
        "clip")

    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def large_case():
    """One same-level segment of 1 223 551 rows: ctx_ehem_all_kernel's grid (2048 workgroups of 256) takes three trips over it."""
    return _case("large-200k", [(octree_recipe()[200000], None, False)], MINMAX, 12, "large")


def by_name(name):
    if name == "large-200k":
        return large_case()
    return {c.name: c for c in cases()}[name]


def names(*tags, without=()):
    """Names of the cases that carry every tag of `tags` and none of `without`."""
    return [c.name for c in cases() if set(tags) <= c.tags and not (set(without) & c.tags)]


# --------------------------------------------------------------------------------------------------------- the oracle's side
OracleSeg = collections.namedtuple("OracleSeg", "tree records depth level_nodes sizes ids pos pos_mm data sym")


def oracle_segment(orc, seg, mode, lidar_level):
    """What the reference computes for one segment: the tree, its K-records and the EHEM chunk lists.  level_nodes: nodes per tree
    level (depth entries); sizes: coded rows per level (depth entries, the last one 0 for a one-leaf shell)."""
    tree = orc.octree_build(seg.pts, seg.path)
    rec = tree.krecords(seg.drop)
    with np.errstate(invalid="ignore", divide="ignore"):                     # 0 / 0 where the reference's own arithmetic gives NaN
        ids, pos, pos_mm, data, oct_seq = orc.ehem_level_split(rec, lidar_level, polar=mode != POW2, mul=mode == MUL)
    level_nodes = np.diff(tree.level_off).tolist()
    sizes = list(level_nodes)
    sizes[-1] -= int(seg.drop)
    assert [len(i) for i in ids] == [s for s in sizes if s], (sizes, [len(i) for i in ids])
    return OracleSeg(tree, rec, tree.depth, level_nodes, sizes, ids, pos, pos_mm, data, oct_seq[:, -1, 0].astype(np.uint8))


@functools.lru_cache(maxsize=None)
def _oracle_case_cached(name):
    from oracle import scp_oracle as orc
    c = by_name(name)
    return tuple(oracle_segment(orc, s, c.mode, c.lidar_level) for s in c.segs)


def oracle_case(name):
    """Per segment OracleSeg of a case, computed once per process and shared (read-only) by the tests."""
    return _oracle_case_cached(name)
