"""tests/lift_ref.py - the vectorised definition the GPU tests at scale compare with - equals the plain-integer definitions attr_ref.py and
color_ref.py field for field: coefficients, contexts, roots, histograms, level counts, both inverses, the coder's pairs and the leaf values,
on every hard tree of attr_cases / color_cases at every Q and on a 21 000-leaf tree the plain references still manage.  The trees of
tests/lift_cases.py are built here as well, which runs every property assertion of their builders.  No GPU."""
import functools

import numpy as np
import pytest

import attr_cases
import attr_ref
import color_cases
import color_ref
import lift_cases
import lift_ref

QS = attr_cases.QS


@functools.lru_cache(maxsize=None)
def midsize():
    """An 8 % random subset of the 64^3 grid at D = 6, in Morton order, with values for both layers."""
    rng = np.random.default_rng(61)
    g = np.arange(64, dtype=np.int64)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    cells = cells[rng.random(len(cells)) < 0.08]
    cells = np.ascontiguousarray(cells[np.argsort(lift_ref.morton(cells, 6))], np.int32)
    assert 19000 < len(cells) < 23000
    rgb = rng.integers(0, 256, size=(len(cells), 3))
    rgb[::7] = [color_cases.RED, color_cases.BLUE, color_cases.GREEN, color_cases.MAGENTA][len(cells) % 4]
    ycc = [color_ref.rgb_to_ycc(*(int(v) for v in c)) for c in rgb]
    return dict(D=6, leaves=cells, a=rng.integers(0, 256, size=len(cells)).astype(np.uint8), rgb=rgb.astype(np.uint8),
                ycc=[[t[ch] for t in ycc] for ch in range(3)])


def reflectance_case(name):
    return midsize() if name == "midsize" else attr_cases.cases()[name]


def colour_case(name):
    return midsize() if name == "midsize" else color_cases.cases()[name]


def rows_for(D, Q, table, planes):
    rng = np.random.default_rng(D * 1000 + Q)
    return table[rng.integers(0, 16, size=planes * D)]


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("name", sorted(attr_cases.cases()) + ["midsize"])
def test_one_plane_equals_attr_ref(name, Q):
    c = reflectance_case(name)
    leaves, D = c["leaves"], c["D"]
    want = attr_ref.forward(leaves, c["a"], D, Q)
    got = lift_ref.forward(leaves, [c["a"]], D, Q)
    assert got["k"].shape == (1, len(leaves) - 1) and got["k"][0].tolist() == want["k"]
    assert got["ctx"].tolist() == want["ctx"]
    assert got["root"].tolist() == [want["root"]]
    assert got["hist"].shape == (D, 511) and got["hist"].tolist() == want["hist"]
    assert got["level_counts"] == want["level_counts"]
    back = attr_ref.inverse(leaves, D, Q, want["root"], want["k"])
    assert lift_ref.inverse_reflectance(leaves, D, Q, want["root"], want["k"]).tolist() == back
    raw = lift_ref.inverse(leaves, D, Q, [want["root"]], [want["k"]])
    assert raw.shape == (1, len(leaves)) and np.clip(raw[0], 0, 255).tolist() == back
    if Q == 1:
        assert raw[0].tolist() == [int(v) for v in c["a"]]                      # lossless before any clamp
    rows = rows_for(D, Q, attr_ref.tables(), 1)
    assert lift_ref.pairs(want["k"], want["ctx"], rows).tolist() == attr_ref.pairs(want["k"], want["ctx"], rows)


@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("name", sorted(color_cases.cases()) + ["midsize"])
def test_three_planes_equal_color_ref(name, Q):
    c = colour_case(name)
    leaves, D = c["leaves"], c["D"]
    want = color_ref.forward(leaves, c["ycc"], D, Q)
    got = lift_ref.forward(leaves, c["ycc"], D, Q)
    assert got["k"].shape == (3, len(leaves) - 1) and got["k"].tolist() == want["k"]
    assert got["ctx"].tolist() == want["ctx"]
    assert got["root"].tolist() == want["root"]
    assert got["hist"].shape == (3 * D, 1021) and got["hist"].tolist() == want["hist"]
    assert got["level_counts"] == want["level_counts"]
    back = color_ref.inverse(leaves, D, Q, want["root"], want["k"])
    assert lift_ref.inverse_rgb(leaves, D, Q, want["root"], want["k"]).tolist() == back
    if Q == 1:
        assert lift_ref.inverse(leaves, D, Q, want["root"], want["k"]).tolist() == [[int(v) for v in p] for p in c["ycc"]]
    rows = rows_for(D, Q, color_ref.tables(), 3)
    assert lift_ref.pairs(want["k"], want["ctx"], rows).tolist() == color_ref.pairs(want["k"], want["ctx"], rows, D)


def test_colour_transform_keys_and_steps_equal_the_plain_ones():
    rng = np.random.default_rng(3)
    rgb = np.concatenate([rng.integers(0, 256, size=(500, 3)), [color_cases.RED, color_cases.BLUE, color_cases.GREEN, color_cases.MAGENTA, (0, 0, 0), (255, 255, 255)]])
    ycc = lift_ref.rgb_to_ycc(rgb)
    assert ycc.T.tolist() == [list(color_ref.rgb_to_ycc(*(int(v) for v in c))) for c in rgb]
    assert lift_ref.ycc_to_rgb(ycc).tolist() == rgb.tolist()
    wild = rng.integers(-700, 700, size=(3, 300))                                     # what a lossy inverse hands to the transform
    assert lift_ref.ycc_to_rgb(wild).tolist() == [list(color_ref.ycc_to_rgb(*(int(v) for v in t))) for t in wild.T]
    for D in (1, 5, 21):
        p = rng.integers(0, 1 << D, size=(200, 3))
        assert lift_ref.morton(p, D).tolist() == [attr_ref.morton(q, D) for q in p]
    w = np.array([1, 2, 3, 7, 8, 64, 4095, 4096, 4097, 65025, 130050, 130051, 1 << 17, 1 << 18, 1 << 21], np.int64)
    for Q in (1, 2, 8, 64, 255):
        got = lift_ref.step(w[:, None], w[None, :], Q)
        assert got.tolist() == [[attr_ref.step(int(a), int(b), Q) for b in w] for a in w]
    assert lift_ref.symbol([-510, -1, 0, 1, 510]).tolist() == [attr_ref.symbol(k) for k in (-510, -1, 0, 1, 510)] == [1020, 2, 0, 1, 1019]


def test_leaf_values_equal_the_plain_ones():
    c = attr_cases.cases()["random"]
    for scale in (255, 100):
        a, cnt = lift_ref.leaf_values(c["q"], c["r"], c["leaves"], c["D"], scale)
        wa, wc = attr_ref.leaf_values(c["q"], c["r"], c["leaves"], c["D"], scale)
        assert a.tolist() == wa and cnt.tolist() == wc
    assert a.shape == cnt.shape == (2000,)
    lv = c["leaves"][:1000]                                                           # half of the leaves: more points fall in none
    a, cnt = lift_ref.leaf_values(c["q"], c["r"], lv, c["D"], 255)
    wa, wc = attr_ref.leaf_values(c["q"], c["r"], lv, c["D"], 255)
    assert a.tolist() == wa and cnt.tolist() == wc
    a, cnt = lift_ref.leaf_values(c["q"][:0], c["r"][:0], lv, c["D"], 255)
    assert not a.any() and not cnt.any() and a.shape == (1000,)
    k = color_cases.cases()["random"]
    assert not (k["leaves"] == 4095).all(axis=1).any()
    for leaves in (k["leaves"], np.concatenate([k["leaves"][500:1500], [[4095, 4095, 4095]]])):     # the last one a leaf nobody hits
        mean, ycc, cnt = lift_ref.leaf_colors(k["q"], k["rgb8"], leaves, k["D"])
        wm, wy, wc = color_ref.leaf_values(k["q"], k["rgb8"], leaves, k["D"])
        assert mean.tolist() == wm and ycc.tolist() == wy and cnt.tolist() == wc
    assert 0 in wc
    # halves round up, thirds to the nearest, a cell beside the leaf, a negative and a too large coordinate count nowhere
    one = np.array([[1, 1, 1]], np.int32)
    q = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 0], [-1, 1, 1], [1, 5, 1]], np.int32)
    assert [x.tolist() for x in lift_ref.leaf_values(q, np.array([10, 11, 200, 200, 200], np.float32), one, 2, 1)] == [[11], [2]]
    assert lift_ref.leaf_colors(q, [(10, 0, 255), (11, 1, 254)] + [(9, 9, 9)] * 3, one, 2)[0].tolist() == [[11, 1, 255]]
    assert lift_ref.point_values(np.array([np.nan, np.inf, -np.inf, -0.25, 1.5, 0.5, 0.49], np.float32), 1).tolist() == [0, 0, 0, 0, 2, 1, 0]


@pytest.mark.parametrize("name", lift_cases.NAMES)
def test_the_large_trees_build_and_keep_their_properties(name):
    """Every builder asserts what its tree is for; here only what all of them share."""
    c = lift_cases.case(name)
    U, D = len(c["leaves"]), c["D"]
    keys = lift_ref.morton(c["leaves"], D)
    assert (np.diff(keys) > 0).all() and c["a"].shape == (U,) and c["rgb"].shape == (U, 3) and c["ycc"].shape == (3, U)
    assert c["ycc"][0].min() >= 0 and c["ycc"][0].max() <= 255 and np.abs(c["ycc"][1:]).max() <= 255
    assert not c["leaves"].flags.writeable and not c["a"].flags.writeable
    if name in lift_cases.PREFIXES:
        assert U == lift_cases.prefix_length(name) and np.array_equal(c["leaves"], lift_cases.sparse()["leaves"][:U])
    if name.startswith("sparse[level1="):
        assert lift_ref.tree(c["leaves"], D)[1][1] == int(name[14:-1]) and U > lift_cases.CHUNK
