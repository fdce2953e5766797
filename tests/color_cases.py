"""The hard trees of the colour layer's tests (host only): the trees of attr_cases.cases() with three-channel values attached.  Every case
is dict(D, leaves int32 [U,3] in Morton order, rgb uint8 [U,3] - the leaf means -, ycc int [3][U] - their YCoCg-R image) and, for the
leaf-value case, q int32 [P,3] / rgb8 uint8 [P,3] / cnt.  Built once per process and never modified."""
import functools

import numpy as np

import attr_cases
import color_ref

RED, BLUE, GREEN, MAGENTA = (255, 0, 0), (0, 0, 255), (0, 255, 0), (255, 0, 255)


def _case(D, leaves, rgb):
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    assert len(rgb) == len(leaves)
    rgb.setflags(write=False)
    ycc = [color_ref.rgb_to_ycc(*(int(v) for v in c)) for c in rgb]
    return dict(D=D, leaves=leaves, rgb=rgb, ycc=[[t[ch] for t in ycc] for ch in range(3)])


def random_points_case(base, seed=17):
    """attr_cases' random case (2 000 leaves at D = 12 under 6 000 points, 1 500 of them in no leaf, negative and too large coordinates
    among them) with colours: the k-th point of a leaf is its base colour + ((k + channel) & 1), so two points per leaf land on halves
    and three on thirds, in either direction depending on the channel."""
    rng = np.random.default_rng(seed)
    D, leaves, q = base["D"], base["leaves"], base["q"]
    index = {tuple(int(c) for c in lv): i for i, lv in enumerate(leaves)}
    tone = rng.integers(0, 255, size=(len(leaves), 3))
    seen = [0] * len(leaves)
    rgb8 = rng.integers(0, 256, size=(len(q), 3))
    for p, pt in enumerate(q):
        i = index.get(tuple(int(c) for c in pt))
        if i is not None:
            rgb8[p] = [min(255, int(tone[i][ch]) + ((seen[i] + ch) & 1)) for ch in range(3)]
            seen[i] += 1
    rgb8 = np.ascontiguousarray(rgb8, np.uint8)
    rgb8.setflags(write=False)
    mean, ycc, cnt = color_ref.leaf_values(q, rgb8, leaves, D)
    assert cnt == base["cnt"].tolist()
    c = _case(D, leaves, mean)
    assert c["ycc"] == ycc
    c.update(q=q, rgb8=rgb8, cnt=np.asarray(cnt, np.int32))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(23)
    a = attr_cases.cases()
    out = {}
    out["single"] = _case(a["single"]["D"], a["single"]["leaves"], [(200, 30, 90)])
    for axis in range(3):
        out[f"axis{axis}"] = _case(3, a[f"axis{axis}"]["leaves"], [(10, 250, 3), (201, 7, 255)])
    cube = a["full_0_first"]["leaves"]
    out["co_red_first"] = _case(2, cube, [RED, BLUE] * 4)              # Co = 255, then -255: d = -510 in every stage-1 pair, z = 1020
    out["co_blue_first"] = _case(2, cube, [BLUE, RED] * 4)             # d = +510: z = 1019
    out["cg_green_first"] = _case(2, cube, [GREEN, MAGENTA] * 4)       # Cg = 255, then -255
    out["cg_magenta_first"] = _case(2, cube, [MAGENTA, GREEN] * 4)
    out["full_plus_one"] = _case(2, a["full_plus_one"]["leaves"], [RED, BLUE] * 4 + [BLUE])
    out["chain21"] = _case(21, a["chain21"]["leaves"], [(3, 250, 128), (250, 3, 127)])
    out["heavy"] = _case(5, a["heavy"]["leaves"], rng.integers(0, 256, size=(len(a["heavy"]["leaves"]), 3)))
    out["random"] = random_points_case(a["random"])
    return out


QS = attr_cases.QS
