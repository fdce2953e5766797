"""The cases of tests/ctx_cases.py, checked on the CPU through the oracle alone: each one still has the edge it is named for, so a later
edit of the generator cannot quietly remove an edge from tests/test_gpu_context.py.  No case is skipped or tolerated away."""
import numpy as np
import pytest

import ctx_cases as CC

ALL = [c.name for c in CC.cases()]


def coded_levels(o):
    """Tree levels (1-based) that have coded rows, in chunk order."""
    return [l + 1 for l, n in enumerate(o.sizes) if n]


def test_the_list_covers_what_it_promises():
    tags = set().union(*(c.tags for c in CC.cases()))
    for t in ("chain", "one-leaf", "clip", "nan", "dropped-extreme", "last-two", "depth1", "full2", "deep19", "deep20", "deep21", "deep-three", "dup", "lidar-same-level",
              "last-level-255", "last-level-256", "last-level-257", "single-node-levels", "stem", "random", "three"):
        assert t in tags, t
    for tag in CC.PATHS:                                   # every path keeps a one-leaf shell of every kind
        assert {f"oneleaf-{tag}-{v}" for v in ("ge", "eq", "clip", "diag")} <= set(ALL)
    modes = {c.name: c.mode for c in CC.cases()}
    assert {modes[n] for n in CC.names("chain")} == {CC.MINMAX, CC.POW2}
    assert all(c.mode == CC.MUL for c in CC.cases() if any(s.drop for s in c.segs))


@pytest.mark.parametrize("name", ALL)
def test_every_case_builds_and_its_chunks_are_its_levels(orc, name):
    """The oracle builds every segment (a path that keeps no point is not in the list) and the reference's chunk list is the tree's
    level list without the levels the drop emptied."""
    c = CC.by_name(name)
    for s, o in zip(c.segs, CC.oracle_case(name)):
        assert o.tree.n == sum(o.level_nodes) and len(o.records) == o.tree.n - int(s.drop) > 0
        assert np.array_equal(o.records[:, 3, 1], np.repeat(np.arange(1, o.depth + 1), o.sizes))
        assert [d.shape for d in o.data] == [(n, 4, 3) for n in o.sizes if n]
        if c.mode != CC.POW2:
            assert len(o.pos_mm) == len(coded_levels(o))
        assert np.array_equal(np.sort(o.tree.krecords(False)[:, 3, 1]), o.tree.level.astype(np.int64))


@pytest.mark.parametrize("name", CC.names("chain"))
def test_chains(orc, name):
    c = CC.by_name(name)
    (o,) = CC.oracle_case(name)
    assert len(c.segs[0].pts) == 1 and o.level_nodes == [1] * o.depth and o.depth >= 3
    x, y, z = c.segs[0].pts[0]
    assert (x == y == z) == ("diagonal" in c.tags)


@pytest.mark.parametrize("name", CC.names("one-leaf"))
def test_one_leaf_shells_end_one_level_above_the_depth(orc, name):
    c = CC.by_name(name)
    hit = 0
    for s, o in zip(c.segs, CC.oracle_case(name)):
        if o.level_nodes != [1] * o.depth:
            continue
        hit += 1
        assert s.drop and c.mode == CC.MUL
        assert int(o.records[:, 3, 1].max()) == o.depth - 1 and o.sizes[-1] == 0           # records end one level above the tree's depth
        assert len(o.data) == o.depth - 1
    assert hit == (3 if "all-leaf" in c.tags else 1)


@pytest.mark.parametrize("name", CC.names("one-leaf", without=("three",)))
def test_one_leaf_lidar_levels(orc, name):
    c = CC.by_name(name)
    (o,) = CC.oracle_case(name)
    D, L = o.depth, c.lidar_level
    var = name.rsplit("-", 1)[1]
    if var in ("ge", "ge1"):
        assert L >= D
    elif var == "eq":
        assert L == D - 1
    else:
        assert L < D - 1 and "clip" in c.tags
    # the clip shows in the last chunk exactly when lidar_level < depth - 1 ...
    last = o.data[-1]
    assert (last[:, -1, 0] == min(D - 1, L)).all()
    assert ("clip" in c.tags) == bool((last[:, :, 0] != o.records[-len(last):, :, 1]).any())
    # ... and in no other chunk
    a = 0
    for d in o.data[:-1]:
        assert np.array_equal(d[:, :, 0], o.records[a:a + len(d), :, 1])
        a += len(d)


@pytest.mark.parametrize("name", CC.names("clip"))
def test_clip_cases_clip_below_the_last_tree_level(orc, name):
    """lidar_level < depth - 1 on a one-leaf shell: a kernel that clips on `level == depth` writes other level bytes than the reference."""
    c = CC.by_name(name)
    n = 0
    for o in CC.oracle_case(name):
        if o.sizes[-1] == 0:
            assert c.lidar_level < o.depth - 1
            assert (o.data[-1][:, -1, 0] == c.lidar_level).all() and (o.records[-len(o.data[-1]):, -1, 1] == o.depth - 1).all()
            n += 1
    assert n >= 1


@pytest.mark.parametrize("name", ALL)
def test_nan_rows_are_exactly_the_tagged_ones(orc, name):
    """The reference's own arithmetic gives NaN (0 / 0, no epsilon on the last multi-level chunk) exactly where the last chunk's extremes
    coincide: in the cases tagged `nan`, in every row of that chunk, and nowhere else."""
    c = CC.by_name(name)
    any_nan = False
    for o in CC.oracle_case(name):
        for k, p in enumerate(o.pos):
            nan = np.isnan(p)
            want = c.mode == CC.MUL and k == len(o.pos) - 1 and o.pos_mm[k][0] == o.pos_mm[k][1]
            assert nan.all() if want else not nan.any(), (name, k)
            any_nan |= bool(want)
            assert not np.isinf(p).any()
    assert any_nan == ("nan" in c.tags)


@pytest.mark.parametrize("name", CC.names("dropped-extreme"))
def test_dropped_node_owns_the_extreme(orc, name):
    """Level min or max changes when the dropped node is excluded."""
    (o,) = CC.oracle_case(name)
    t = o.tree
    full = t.pos[t.level_off[-2]:t.level_off[-1]]
    coded = full[:-1]
    assert len(coded) >= 1
    changed_max, changed_min = full.max() != coded.max(), full.min() != coded.min()
    assert changed_max if name.endswith("max") else changed_min
    assert o.pos_mm[-1] == (coded.min(), coded.max())


@pytest.mark.parametrize("name", CC.names("last-two"))
def test_last_level_with_one_coded_node(orc, name):
    (o,) = CC.oracle_case(name)
    assert o.level_nodes[-1] == 2 and o.sizes[-1] == 1
    mn, mx = o.pos_mm[-1]
    assert (mn == mx) == name.endswith("equal")


def test_last_two_covers_both():
    eq = {CC.oracle_case(n)[0].pos_mm[-1][0] == CC.oracle_case(n)[0].pos_mm[-1][1] for n in CC.names("last-two")}
    assert eq == {True, False}


def test_small_deep_and_duplicated(orc):
    for n in CC.names("depth1"):
        (o,) = CC.oracle_case(n)
        assert o.depth == 1 and o.level_nodes == [1] and CC.by_name(n).segs[0].pts.max() == 1
    for n in CC.names("full2"):
        c = CC.by_name(n)
        (o,) = CC.oracle_case(n)
        assert o.depth == 2 and len(np.unique(c.segs[0].pts, axis=0)) == 64
        assert o.level_nodes == ([1, 8] if c.segs[0].path is None else [1, 4]) and (o.tree.occ[1:] == 255).all()
    for d in (19, 20, 21):
        names = CC.names(f"deep{d}", without=("deep-three",))
        assert {CC.by_name(n).mode for n in names} == {CC.MINMAX, CC.POW2, CC.MUL}
        for n in names:
            (o,) = CC.oracle_case(n)
            assert o.depth == d and len(CC.by_name(n).segs[0].pts) == 2 and CC.by_name(n).segs[0].pts.max() == 2 ** d - 1
            assert o.level_nodes[0] == 1 and o.level_nodes[-1] == 2
    (n,) = CC.names("deep-three")
    assert [o.depth for o in CC.oracle_case(n)] == [20, 20, 20] and all(len(o.records) > 20 for o in CC.oracle_case(n))
    for n in CC.names("dup"):
        pts = CC.by_name(n).segs[0].pts
        assert len(np.unique(pts, axis=0)) < len(pts) and not np.array_equal(pts, pts[np.lexsort(pts.T[::-1])])


def test_lidar_level_in_same_level_mode(orc):
    got = set()
    for n in CC.names("lidar-same-level"):
        c = CC.by_name(n)
        (o,) = CC.oracle_case(n)
        assert not c.segs[0].drop and o.depth == 6
        got.add(np.sign(c.lidar_level - o.depth))
        clipped = (o.data[-1][:, :, 0] != o.records[-len(o.data[-1]):, :, 1]).any()
        assert clipped == (c.lidar_level < o.depth)
    assert got == {-1, 0, 1}


@pytest.mark.parametrize("n", [255, 256, 257])
def test_tile_edge_levels(orc, n):
    names = CC.names(f"last-level-{n}")
    assert {CC.by_name(x).mode for x in names} == {CC.MINMAX, CC.POW2, CC.MUL}
    for x in names:
        (o,) = CC.oracle_case(x)
        assert o.sizes[-1] == n and o.sizes[0] == 1, (x, o.sizes)


@pytest.mark.parametrize("name", CC.names("single-node-levels"))
def test_single_node_levels_in_same_level_mode(orc, name):
    c = CC.by_name(name)
    (o,) = CC.oracle_case(name)
    assert not c.segs[0].drop
    single = [l + 1 for l, n in enumerate(o.sizes) if n == 1]
    assert any(l >= 2 for l in single)                       # level k >= 2 has one node in same-level mode
    if "stem" in c.tags:
        assert o.sizes == [1, 1, 1, 1, 1, 8]


def test_random_clouds(orc):
    names = CC.names("random")
    assert len(names) == 3 * 6
    sizes = sorted({len(CC.by_name(n).segs[0].pts) for n in names})
    assert len(sizes) == 3 and 25000 <= sizes[-1] <= 35000
    for n in names:
        c = CC.by_name(n)
        (o,) = CC.oracle_case(n)
        assert o.tree.n > 50
    paths = {tuple(CC.by_name(n).segs[0].path or ()) for n in names if CC.by_name(n).segs[0].drop}
    assert paths == {(), (0, 0), (0, 1), (1,)}


def test_the_recipe_is_the_octree_test_s(orc):
    r = CC.octree_recipe()
    assert sorted(r) == [1, 17, 1000, 30000, 200000]
    assert orc.octree_build(r[200000]).n == 1_223_551


def test_large_case_needs_more_than_one_grid_trip(orc):
    c = CC.large_case()
    (o,) = CC.oracle_case(c.name)
    assert len(c.segs) == 1 and not c.segs[0].drop
    assert len(o.records) == 1_223_551 > CC.GRID_ROWS                            # rows > 2048 * 256
    assert max(o.sizes) > 8192 and any(n % 8192 for n in o.sizes)


@pytest.mark.parametrize("name", CC.names("three"))
def test_three_segment_cases(orc, name):
    c = CC.by_name(name)
    os_ = CC.oracle_case(name)
    assert [s.path for s in c.segs] == [[0, 0], [0, 1], [1]] and all(s.drop for s in c.segs)
    leaf = [o.sizes[-1] == 0 for o in os_]
    assert any(leaf)
    if "all-leaf" not in c.tags:
        assert max(len(o.records) for o in os_) > 2000 and not all(leaf)
        k = leaf.index(True)
        assert k == {"three-leaf-first": 0, "three-leaf-middle": 1, "three-leaf-last-clip": 2}[name]
        if k < 2:
            assert len(os_[k + 1].records) > 256                     # a later segment's row_base / mm_base follows the degenerate one


def test_coding_plans_differ_only_at_single_node_levels(orc):
    """encode.py:122 leaves `coded_cnt` out for a single-node level (same-level mode), encode_mullevel.py:120 adds it: the two orders differ
    exactly at single-node levels below level 1, where the same-level one names a row already coded (not decodable).  The GPU tests and
    ctx_ehem_all_kernel use the mullevel=True order in both modes."""
    seen_diff = False
    for name in ALL:
        sizes = [n for o in CC.oracle_case(name) for n in o.sizes if n]
        for cs in CC.CONTEXT_SIZES:
            w0, a = orc.ehem_coding_plan(sizes, cs, mullevel=False)
            w1, b = orc.ehem_coding_plan(sizes, cs, mullevel=True)
            assert w0 == w1 and len(a) == len(b) == sum(sizes)
            assert np.array_equal(np.sort(b), np.arange(sum(sizes)))             # the mullevel order is a permutation: decodable
            first = np.cumsum([0] + sizes[:-1])
            want = sorted(int(first[l]) for l, n in enumerate(sizes) if n == 1 and l >= 1)
            assert np.flatnonzero(a != b).tolist() == want, (name, cs)
            assert (a[want] == 0).all()
            seen_diff |= bool(want)
    assert seen_diff
