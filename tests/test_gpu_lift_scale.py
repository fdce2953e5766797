"""Both attribute layers on the GPU at the sizes of the streams they exist for: every check tests/test_gpu_attr.py and
tests/test_gpu_color.py make on trees of a few thousand leaves, made on the trees of tests/lift_cases.py - 262 145 to 282 834 leaves, a
second trip of the one-block scan on levels 0, 1 and 2, families across thread groups and tile edges, weights to 2^18, 63-bit keys - and
on prefixes of the sparse tree cut at the tile and scan-chunk edges of levels 0 and 1; a million points on the leaf-value kernels, 400 000
of them on two leaves; the attribute and colour files of two such shells through the host coder.  Expected values come from
tests/lift_ref.py, which tests/test_lift_ref.py ties to the plain definitions.  Every comparison is exact and made on arrays.  A tree's
reference is computed once per process."""
import functools

import numpy as np
import pytest
import torch

import attr_ref
import color_ref
import lift_cases
import lift_ref
from attr_cases import QS
from test_gpu_ringrate import dev

pytestmark = pytest.mark.gpu

LARGE_QS = (1, 255)                                                     # the lossless identity and the clamps


def qs_of(name):
    small = name in lift_cases.SMALL or (name.startswith("sparse[:") and lift_cases.prefix_length(name) < 5000)
    return QS if small else LARGE_QS


TREES = [(name, Q) for name in lift_cases.BUILDERS for Q in qs_of(name)]
CUTS = [(name, Q) for name in lift_cases.PREFIXES for Q in qs_of(name)]


@pytest.fixture(scope="module", autouse=True)
def leave_the_process_as_found():
    """The references are shared by the tests of this module only: afterwards they are dropped and the allocator's cached blocks go back
    to the device, so that the modules that follow start from the memory they always started from."""
    yield
    import gc
    reference.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def up(x, dtype):
    return torch.from_numpy(np.array(x, dtype, order="C")).to(dev())    # a contiguous copy: the shared inputs are read-only


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(layer, name, Q):
    """lift_ref's forward of a tree under one layer ("attr": the plane a, "color": the planes ycc); for the builders' trees also
    `back`, what the layer's decoder returns for the reference's coefficients."""
    c = lift_cases.case(name)
    f = lift_ref.forward(c["leaves"], c["a"] if layer == "attr" else c["ycc"], c["D"], Q)
    if name in lift_cases.BUILDERS:
        inv = lift_ref.inverse_reflectance if layer == "attr" else lift_ref.inverse_rgb
        f["back"] = inv(c["leaves"], c["D"], Q, f["root"][0] if layer == "attr" else f["root"], f["k"][0] if layer == "attr" else f["k"])
    return f


def check_forward(got, want, planes):
    assert np.array_equal(host(got["k"]).reshape(planes, -1), want["k"])
    assert np.array_equal(host(got["ctx"]), want["ctx"])
    assert np.array_equal(host(got["root"]), want["root"])
    assert np.array_equal(host(got["hist"]), want["hist"])
    assert np.array_equal(host(got["level_counts"]), want["level_counts"])


@pytest.mark.parametrize("name,Q", TREES)
def test_reflectance_kernels_equal_the_reference(name, Q):
    from scp_amd import attr, native
    c, want = lift_cases.case(name), reference("attr", name, Q)
    U, D = len(c["leaves"]), c["D"]
    lv = up(c["leaves"], np.int32).reshape(-1, 3)
    got = native.attr_forward(lv, up(c["a"], np.uint8), D, Q)
    assert got["k"].dtype == torch.int16 and got["ctx"].dtype == torch.uint8 and got["k"].shape == (U - 1,)
    check_forward(got, want, 1)
    assert int(want["hist"].sum()) == U - 1
    assert np.array_equal(host(native.attr_level_counts(lv, D)), want["level_counts"])
    assert np.array_equal(attr.level_contexts(want["level_counts"]), want["ctx"])
    rng = np.random.default_rng(D * 1000 + Q)
    rows = attr_ref.tables()[rng.integers(0, 16, size=D)]
    rows[0] = attr_ref.tables()[0 if Q == 1 else 15]
    lohi = native.attr_pairs(got["k"], got["ctx"], up(rows.view(np.int16), np.int16))
    assert np.array_equal(host(lohi).view(np.uint32), lift_ref.pairs(want["k"], want["ctx"], rows))
    back = native.attr_inverse(lv, D, Q, int(want["root"][0]), up(want["k"][0], np.int16))
    assert back.dtype == torch.uint8 and np.array_equal(host(back), want["back"])
    if Q == 1:
        assert np.array_equal(want["back"], c["a"])


@pytest.mark.parametrize("name,Q", TREES)
def test_colour_kernels_equal_the_reference(name, Q):
    from scp_amd import native
    c, want = lift_cases.case(name), reference("color", name, Q)
    U, D = len(c["leaves"]), c["D"]
    lv = up(c["leaves"], np.int32).reshape(-1, 3)
    got = native.color_forward(lv, up(c["ycc"], np.int16), D, Q)
    assert got["k"].dtype == torch.int16 and got["ctx"].dtype == torch.uint8 and got["k"].shape == (3, U - 1) and got["ctx"].shape == (U - 1,)
    assert got["hist"].shape == (3 * D, 1021)
    check_forward(got, want, 3)
    assert np.array_equal(host(native.attr_level_counts(lv, D)), want["level_counts"])
    # the shared launch has the single-channel kernel's bits on the Y plane
    one = native.attr_forward(lv, up(c["ycc"][0], np.uint8), D, Q)
    assert torch.equal(one["k"], got["k"][0]) and torch.equal(one["ctx"], got["ctx"]) and int(one["root"].item()) == int(got["root"][0].item())
    assert torch.equal(one["hist"], got["hist"][:D, :511]) and not got["hist"][:D, 511:].any()
    assert torch.equal(one["level_counts"], got["level_counts"])
    rng = np.random.default_rng(D * 1000 + Q)
    rows = color_ref.tables()[rng.integers(0, 16, size=3 * D)]
    rows[D] = color_ref.tables()[0 if Q == 1 else 15]
    lohi = native.color_pairs(got["k"], got["ctx"], up(rows.view(np.int16), np.int16))
    assert lohi.shape == (3 * (U - 1),) and np.array_equal(host(lohi).view(np.uint32), lift_ref.pairs(want["k"], want["ctx"], rows))
    back = native.color_inverse(lv, D, Q, want["root"].tolist(), up(want["k"], np.int16))
    assert back.dtype == torch.uint8 and back.shape == (U, 3) and np.array_equal(host(back), want["back"])
    if Q == 1:
        assert np.array_equal(want["back"], c["rgb"])


@pytest.mark.parametrize("name,Q", CUTS)
def test_prefixes_cut_at_tile_and_scan_chunk_edges(name, Q):
    """The colour layer's forward and the level counts on the sparse tree cut where level 0 or level 1 ends one entry before, on and one
    entry after a tile of 1024 and the scan's chunk of 262 144 entries."""
    from scp_amd import native
    c, want = lift_cases.case(name), reference("color", name, Q)
    U, D = len(c["leaves"]), c["D"]
    lv = up(c["leaves"], np.int32).reshape(-1, 3)
    got = native.color_forward(lv, up(c["ycc"], np.int16), D, Q)
    assert got["k"].shape == (3, U - 1)
    check_forward(got, want, 3)
    assert np.array_equal(host(native.attr_level_counts(lv, D)), want["level_counts"])


def test_a_million_points_on_the_leaf_value_kernels():
    """tests/lift_cases.sphere_points: 300 000 points on one leaf (an exact half, rounded up) and 100 000 on another contend on their
    64-bit sums; 50 000 points lie in no leaf; the binary search runs over 282 834 keys."""
    from scp_amd import native
    c, p = lift_cases.sphere(), lift_cases.sphere_points()
    lv, q = up(c["leaves"], np.int32), up(p["q"], np.int32)
    wa, wc = lift_ref.leaf_values(p["q"], p["r"], c["leaves"], c["D"], p["scale"])
    assert wc[p["half"]] == 300000 and wa[p["half"]] == 101 and wc[p["full"]] == 100000 and wa[p["full"]] == 255
    assert int(wc.sum()) == 950000 and int((wc == 0).sum()) > 1000 and set(np.unique(wc)) >= {0, 1, 2, 3}
    a, cnt = native.attr_leaf_values(q, up(p["r"], np.float32), lv, c["D"], p["scale"])
    assert a.dtype == torch.uint8 and cnt.dtype == torch.int32
    assert np.array_equal(host(cnt), wc) and np.array_equal(host(a), wa)
    wm, wy, wk = lift_ref.leaf_colors(p["q"], p["rgb8"], c["leaves"], c["D"])
    assert wm[p["half"]].tolist() == [101, 101, 101] and wm[p["full"]].tolist() == [255, 255, 255] and np.array_equal(wk, wc)
    mean, ycc, cnt = native.color_leaf_values(q, up(p["rgb8"], np.uint8), lv, c["D"])
    assert mean.dtype == torch.uint8 and ycc.dtype == torch.int16 and cnt.dtype == torch.int32 and ycc.shape == (3, len(c["leaves"]))
    assert np.array_equal(host(cnt), wc) and np.array_equal(host(mean), wm) and np.array_equal(host(ycc), wy)


def two_shells():
    """`sphere` and the 262 145-leaf prefix of `sparse` as the shells of one file, one point per leaf: the points of a shell lie at -1 for
    the other one, so every leaf's value is its tree's own."""
    s, t = lift_cases.sphere(), lift_cases.case("sparse[:262145]")
    ns, nt = len(s["leaves"]), len(t["leaves"])
    nowhere = lambda n: np.full((n, 3), -1, np.int32)
    qs = [np.concatenate([s["leaves"], nowhere(nt)]), np.concatenate([nowhere(ns), t["leaves"]])]
    return s, t, [up(s["leaves"], np.int32), up(t["leaves"], np.int32)], [s["D"], t["D"]], [up(q, np.int32) for q in qs]


@pytest.mark.parametrize("Q", LARGE_QS)
def test_attribute_file_of_two_large_shells_round_trips(Q):
    """encode_shells -> bytes -> decode_shells: 545 000 symbols through the host coder and back."""
    from scp_amd import attr
    s, t, leaves, depths, qs = two_shells()
    refl = up(np.concatenate([s["a"], t["a"]]) / 255.0, np.float32)
    data, rep = attr.encode_shells(leaves, depths, qs, refl, Q, 255)
    assert np.array_equal(host(rep["values"][0]), s["a"]) and np.array_equal(host(rep["values"][1]), t["a"]) and rep["bits"] == 8 * len(data)
    assert int(rep["counts"][0].min()) == int(rep["counts"][0].max()) == 1
    info = {}
    values = attr.decode_shells(data, leaves, depths, info)
    assert info == dict(Q=Q, scale=255) and [int(v.shape[0]) for v in values] == [len(s["a"]), len(t["a"])]
    for v, d in zip(values, rep["decoded"]):
        assert torch.equal(v, d)
    assert np.array_equal(host(values[0]), reference("attr", "sphere", Q)["back"])
    if Q == 1:
        for v, coded in zip(values, rep["values"]):
            assert torch.equal(v, coded)


@pytest.mark.parametrize("Q", LARGE_QS)
def test_colour_file_of_two_large_shells_round_trips(Q):
    """encode_shells -> bytes -> decode_shells: 1.6 million symbols of the 1021-symbol alphabet through the host coder and back."""
    from scp_amd import color
    s, t, leaves, depths, qs = two_shells()
    rgb8 = up(np.concatenate([s["rgb"], t["rgb"]]), np.uint8)
    data, rep = color.encode_shells(leaves, depths, qs, rgb8, Q)
    assert np.array_equal(host(rep["values"][0]), s["rgb"]) and np.array_equal(host(rep["values"][1]), t["rgb"]) and rep["bits"] == 8 * len(data)
    info = {}
    values = color.decode_shells(data, leaves, depths, info)
    assert info == dict(Q=Q) and [tuple(v.shape) for v in values] == [(len(s["rgb"]), 3), (len(t["rgb"]), 3)]
    for v, d in zip(values, rep["decoded"]):
        assert torch.equal(v, d)
    assert np.array_equal(host(values[0]), reference("color", "sphere", Q)["back"])
    if Q == 1:
        for v, coded in zip(values, rep["values"]):
            assert torch.equal(v, coded)
