"""Step sweep of the attribute layers on the GPU ("Step sweep"): for every step of a grid, scp_attr_sweep / scp_color_sweep
return the histograms of the forward entry at that step and the squared and largest error of what the inverse entry would return, from one
pass over the tree.  The histograms are compared with the forward entries, the errors with the plain-integer references (attr_ref /
color_ref forward + inverse, lift_ref on the lift_cases trees), the chosen step of encode_attr / encode_color(target=...) with a choice
made from the references' own table.  Every comparison is exact.  The references of a case are computed once per process."""
import functools
import math

import numpy as np
import pytest
import torch

import attr_cases
import attr_ref
import color_cases
import color_ref
import lift_cases
import lift_ref
from test_gpu_attr import multilevel_frame
from test_gpu_ringrate import dev, ehem_model

pytestmark = pytest.mark.gpu

DEFAULT = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 255)
GRIDS = ((1,), (1, 8, 255), DEFAULT)
LIFT_NAMES = lift_cases.SMALL + tuple(f"sparse[:{U}]" for U in lift_cases.TILE_PREFIXES)
ATTR_NAMES = tuple(sorted(attr_cases.cases())) + LIFT_NAMES
COLOR_NAMES = tuple(sorted(color_cases.cases())) + LIFT_NAMES


@pytest.fixture(scope="module", autouse=True)
def leave_the_process_as_found():
    yield
    import gc
    for f in (attr_errors, color_errors, frame_reference, object_cloud):
        f.cache_clear()
    multilevel_frame.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def up(x, dtype):
    return torch.from_numpy(np.array(x, dtype)).to(dev())               # a copy: the shared inputs are read-only


def attr_case(name):
    return lift_cases.case(name) if name in LIFT_NAMES else attr_cases.cases()[name]


def color_case(name):
    return lift_cases.case(name) if name in LIFT_NAMES else color_cases.cases()[name]


def errors_of(x, back):
    """int [U, C] coded and returned values -> (sse [C], linf [C]) as Python integers."""
    d = np.abs(np.asarray(x, np.int64).reshape(len(x), -1) - np.asarray(back, np.int64).reshape(len(x), -1))
    return [int(v) for v in (d * d).sum(axis=0)], [int(v) for v in d.max(axis=0, initial=0)]


PLAIN = (1, 8, 255)                 # the steps at which the small trees go through the plain-Python references; the others through lift_ref


@functools.lru_cache(maxsize=None)
def attr_errors(name):
    """Per step of DEFAULT the reference's (sse [1], linf [1], wild: the inverse leaves 0 .. 255 before the clamp on some leaf - known
    where lift_ref ran).  attr_cases' trees: attr_ref at the steps of PLAIN, lift_ref (which test_lift_ref.py ties to it) at the others."""
    c = attr_case(name)
    out = {}
    for Q in DEFAULT:
        if name in LIFT_NAMES or Q not in PLAIN:
            f = lift_ref.forward(c["leaves"], c["a"], c["D"], Q)
            raw = lift_ref.inverse(c["leaves"], c["D"], Q, f["root"], f["k"])[0]
            back, wild = np.clip(raw, 0, 255), bool(((raw < 0) | (raw > 255)).any())
        else:
            f = attr_ref.forward(c["leaves"], c["a"], c["D"], Q)
            back, wild = attr_ref.inverse(c["leaves"], c["D"], Q, f["root"], f["k"]), None
        out[Q] = errors_of(c["a"], back) + (wild,)
    return out


@functools.lru_cache(maxsize=None)
def color_errors(name):
    """As attr_errors, for R, G, B: color_ref at the steps of PLAIN on color_cases' trees, lift_ref elsewhere."""
    c = color_case(name)
    out = {}
    for Q in DEFAULT:
        if name in LIFT_NAMES or Q not in PLAIN:
            f = lift_ref.forward(c["leaves"], c["ycc"], c["D"], Q)
            raw = lift_ref.ycc_to_rgb(lift_ref.inverse(c["leaves"], c["D"], Q, f["root"], f["k"]))
            back, wild = np.clip(raw, 0, 255), bool(((raw < 0) | (raw > 255)).any())
        else:
            f = color_ref.forward(c["leaves"], c["ycc"], c["D"], Q)
            back, wild = color_ref.inverse(c["leaves"], c["D"], Q, f["root"], f["k"]), None
        out[Q] = errors_of(c["rgb"], back) + (wild,)
    return out


def check_sweep(s, grid, forward, want, channels):
    """One sweep's outputs against the forward entry (per step, computed once per test) and the reference's errors."""
    assert s["steps"].tolist() == list(grid)
    assert s["hist"].dtype == torch.int32 and s["sse"].dtype == torch.int64 and s["linf"].dtype == torch.int32
    hist, sse, linf = s["hist"].cpu(), s["sse"].cpu().tolist(), s["linf"].cpu().tolist()
    assert sse == [want[Q][0] for Q in grid] and linf == [want[Q][1] for Q in grid]
    for g, Q in enumerate(grid):
        f = forward(Q)
        assert torch.equal(hist[g], f["hist"].cpu()), (g, Q)
        assert torch.equal(s["root"], f["root"]) and torch.equal(s["level_counts"], f["level_counts"])
    if grid[0] == 1:
        assert sse[0] == [0] * channels and linf[0] == [0] * channels


@pytest.mark.parametrize("name", ATTR_NAMES)
def test_reflectance_sweep_equals_forward_histograms_and_reference_errors(name):
    from scp_amd import native
    c = attr_case(name)
    lv, a = up(c["leaves"], np.int32).reshape(-1, 3), up(c["a"], np.uint8)
    forward = functools.lru_cache(maxsize=None)(lambda Q: native.attr_forward(lv, a, c["D"], Q))
    for grid in GRIDS:
        check_sweep(native.attr_sweep(lv, a, c["D"], grid), grid, forward, attr_errors(name), 1)
    if name == "shifted":                                    # the level-1 clamp is at work at Q = 255: without it the errors would differ
        assert attr_errors(name)[255][2] is True


@pytest.mark.parametrize("name", COLOR_NAMES)
def test_colour_sweep_equals_forward_histograms_and_reference_errors(name):
    from scp_amd import native
    c = color_case(name)
    lv, ycc, rgb = up(c["leaves"], np.int32).reshape(-1, 3), up(c["ycc"], np.int16), up(c["rgb"], np.uint8)
    forward = functools.lru_cache(maxsize=None)(lambda Q: native.color_forward(lv, ycc, c["D"], Q))
    for grid in GRIDS:
        check_sweep(native.color_sweep(lv, ycc, rgb, c["D"], grid), grid, forward, color_errors(name), 3)
    if name == "shifted":                                    # R, G or B leaves 0 .. 255 before the clamp at Q = 255
        assert color_errors(name)[255][2] is True


def test_empty_one_leaf_and_two_leaf_trees():
    from scp_amd import native
    none = torch.zeros((0, 3), dtype=torch.int32, device=dev())
    s = native.attr_sweep(none, torch.zeros(0, dtype=torch.uint8, device=dev()), 7, DEFAULT)
    for k in ("hist", "sse", "linf", "root", "level_counts"):
        assert not s[k].any(), k
    assert s["hist"].shape == (16, 7, 511) and s["sse"].shape == (16, 1) and s["level_counts"].shape == (8,)
    s = native.color_sweep(none, torch.zeros((3, 0), dtype=torch.int16, device=dev()), torch.zeros((0, 3), dtype=torch.uint8, device=dev()), 7, (1, 8, 255))
    for k in ("hist", "sse", "linf", "root", "level_counts"):
        assert not s[k].any(), k
    assert s["hist"].shape == (3, 21, 1021) and s["sse"].shape == (3, 3) and s["linf"].shape == (3, 3)
    c = attr_cases.cases()["single"]
    s = native.attr_sweep(up(c["leaves"], np.int32), up(c["a"], np.uint8), c["D"], DEFAULT)
    assert not s["hist"].any() and not s["sse"].any() and not s["linf"].any()
    assert s["root"].tolist() == [77] and s["level_counts"].tolist() == [1] * (c["D"] + 1)
    c = color_cases.cases()["single"]
    s = native.color_sweep(up(c["leaves"], np.int32), up(c["ycc"], np.int16), up(c["rgb"], np.uint8), c["D"], DEFAULT)
    assert not s["hist"].any() and not s["sse"].any() and not s["linf"].any()
    assert s["root"].tolist() == list(color_ref.rgb_to_ycc(200, 30, 90)) and s["level_counts"].tolist() == [1] * (c["D"] + 1)
    # two leaves, D = 3: one coefficient at the top level, d = 191, root 105; at Q = 255 the step is isqrt(2 * 255^2) = 360, k = 1, and the
    # inverse returns 105 - 180 = -75 -> 0 and -75 + 360 = 285 -> 255: errors 10 and 54 behind the clamp, 85 and 84 without it
    c = attr_cases.cases()["axis0"]
    s = native.attr_sweep(up(c["leaves"], np.int32), up(c["a"], np.uint8), c["D"], (1, 255))
    assert s["sse"].tolist() == [[0], [10 * 10 + 54 * 54]] and s["linf"].tolist() == [[0], [54]]
    assert s["hist"][:, 2].nonzero().tolist() == [[0, 2 * 191 - 1], [1, 1]] and int(s["hist"].sum()) == 2
    assert s["root"].tolist() == [10 + 191 // 2] and s["level_counts"].tolist() == [2, 2, 2, 1]


def table_bits(hist, tables):
    """The bits of histogram rows [contexts, alphabet] under the best of the 16 tables per row, from the tables' definition."""
    t = np.asarray(tables).astype(np.int64)
    hi = t[:, 1:].copy()
    hi[:, -1] = 65536
    cost = np.asarray(hist, np.float64) @ (16.0 - np.log2((hi - t[:, :-1]).astype(np.float64))).T
    return float(cost.min(axis=1).sum())


def psnr(sse, n):
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 * n / sse)


def reference_table(shells, header, tables, points):
    """shells: per shell (forward(Q) -> dict(hist, root, k), inverse(Q, f) -> clamped values [U, C], coded values [U, C], record bytes).
    -> per step of DEFAULT dict(Q, sse, linf, psnr, est_bits) from the references alone, and the number of coded shells."""
    rows = []
    for Q in DEFAULT:
        sse, linf, nbytes, n = 0, 0, header, 0
        for forward, inverse, x, record in shells:
            nbytes += record
            n += np.asarray(x).size
            if len(x) < 2:
                continue
            f = forward(Q)
            e2, em = errors_of(x, inverse(Q, f))
            sse, linf = sse + sum(e2), max([linf] + em)
            nbytes += math.ceil(table_bits(f["hist"], tables) / 8.0)
        rows.append(dict(Q=Q, sse=sse, linf=linf, psnr=psnr(sse, n), est_bits=8 * nbytes))
    return dict(points=points, rows=rows, coded=sum(len(s[2]) >= 2 for s in shells))


@functools.lru_cache(maxsize=None)
def frame_reference():
    """The sweep table of the multi-level frame from attr_ref's leaf values and lift_ref's forward + inverse (test_lift_ref.py ties
    lift_ref to attr_ref)."""
    m = multilevel_frame()
    depths = [int(i.depth) for i in m["enc"].geom.info]
    shells = []
    for s in range(3):
        lv, D = m["kept"][s], depths[s]
        a = np.array(attr_ref.leaf_values(m["qs"][s], m["refl"], lv, D, 255)[0], np.int64)
        shells.append((functools.partial(lift_ref.forward, lv, a, D),
                       lambda Q, f, lv=lv, D=D: lift_ref.inverse_reflectance(lv, D, Q, f["root"][0], f["k"][0]), a, 5 + 1 + D + 4))
    return reference_table(shells, 4 + 7, attr_ref.tables(), len(m["xyz"]))


def pick_targets(ref):
    """Targets whose choice the reference's table decides without a doubt -> [(kind, value, the expected Q, the next grid step or None)]:
    a PSNR halfway between two adjacent rows (the pair nearest Q = 8 / 12 below which every later row stays), the largest error of the
    row of Q = 6, a rate halfway between two adjacent rows (the pair nearest Q = 3 / 4 above which every earlier row stays)."""
    rows, n = ref["rows"], ref["points"]
    near = sorted(range(len(rows) - 1), key=lambda i: abs(i - 5))
    for i in near:
        P = 0.5 * (rows[i]["psnr"] + rows[i + 1]["psnr"])
        if math.isfinite(P) and rows[i]["psnr"] > P and all(r["psnr"] < P for r in rows[i + 1:]):
            break
    else:
        raise AssertionError("no PSNR target between two rows")
    E = rows[4]["linf"]
    q_e = max(r["Q"] for r in rows if r["linf"] <= E)
    after = {q: DEFAULT[DEFAULT.index(q) + 1] if q != DEFAULT[-1] else None for q in DEFAULT}
    for b in sorted(range(1, len(rows)), key=lambda b: abs(b - 3)):
        B = 0.5 * (rows[b]["est_bits"] + rows[b - 1]["est_bits"]) / n
        if rows[b]["est_bits"] < B * n and all(r["est_bits"] > B * n for r in rows[:b]):
            break
    else:
        raise AssertionError("no rate target between two rows")
    return [("psnr", P, rows[i]["Q"], rows[i + 1]["Q"]), ("linf", E, q_e, after[q_e]), ("bpp", B, rows[b]["Q"], None)]


def leaf_errors(rep):
    """(sse, linf, values) of a report's `values` against its `decoded`, over all shells and channels."""
    x = torch.cat([v.reshape(v.shape[0], -1) for v in rep["values"]]).long()
    y = torch.cat([v.reshape(v.shape[0], -1) for v in rep["decoded"]]).long()
    d = (x - y).abs()
    return int((d * d).sum()), int(d.max()), x.numel()


def check_target(encode, decode, ref, kind, value, want_q, next_q, chunk=None):
    """encode(Q=..., target=..., chunk=...) with a target against the reference's choice, the plain call at that step, the decoder and
    the errors recomputed from the report."""
    data, rep = encode(target=(kind, value), chunk=chunk)
    assert (rep["target"], rep["chosen_Q"], rep["met"], rep["Q"]) == ((kind, value), want_q, True, want_q), kind
    plain, prep = encode(Q=want_q, chunk=chunk)
    assert data == plain and rep["bits"] == prep["bits"] == 8 * len(data)
    for got, dec in zip(decode(data), rep["decoded"]):
        assert torch.equal(got, dec)
    table = rep["sweep"]
    assert [r["Q"] for r in table["rows"]] == list(DEFAULT) and table["points"] == ref["points"]
    for r, w in zip(table["rows"], ref["rows"]):                 # the device's table is the reference's
        assert (r["sse"], r["linf"], r["est_bits"]) == (w["sse"], w["linf"], w["est_bits"]) and r["psnr"] == pytest.approx(w["psnr"], rel=1e-12), r["Q"]
    sse, linf, n = leaf_errors(rep)
    row = table["rows"][DEFAULT.index(want_q)]
    assert (sse, linf) == (row["sse"], row["linf"])
    if kind == "psnr":
        assert psnr(sse, n) >= value
    if kind == "linf":
        assert linf <= value
    if kind == "bpp":
        assert row["est_bits"] <= value * ref["points"]
        if chunk is None:                                        # the coder's termination: at most two bytes per coded shell (README)
            print("bpp target: estimated", row["est_bits"], "written", rep["bits"], "coded shells", ref["coded"])
            assert rep["bits"] - row["est_bits"] <= 16 * ref["coded"]
    if next_q is not None:
        sse2, linf2, _ = leaf_errors(encode(Q=next_q, chunk=chunk)[1])
        assert (psnr(sse2, n) < value) if kind == "psnr" else (linf2 > value)
    return rep


def test_multilevel_frame_meets_its_targets():
    from scp_amd import attr, native
    m, ref = multilevel_frame(), frame_reference()
    enc = m["enc"]
    depths = [int(i.depth) for i in enc.geom.info]
    leaves = [up(k, np.int32).reshape(-1, 3) for k in m["kept"]]

    def encode(Q=1, target=None, chunk=None):
        return enc.encode_attr(m["x_dev"], m["r_dev"], Q, chunk=chunk, target=target)

    def decode(data):
        return attr.decode_shells(data, leaves, depths)

    assert ref["coded"] == 3
    sweep = enc.attr_sweep(m["x_dev"], m["r_dev"])
    assert sweep["steps"] == list(DEFAULT) and sweep["leaves"] == sum(len(k) for k in m["kept"])
    targets = pick_targets(ref)
    for kind, value, want_q, next_q in targets:
        rep = check_target(encode, decode, ref, kind, value, want_q, next_q)
        assert rep["sweep"] == sweep
    kind, value, want_q, next_q = targets[0]
    rep = check_target(encode, decode, ref, kind, value, want_q, next_q, chunk=256)       # the same choice into a version-2 file
    assert rep["chunk"] == 256
    short = enc.encode_attr(m["x_dev"], m["r_dev"], target=("psnr", value), steps=(2, want_q, 255))[1]      # the same target on a grid of three
    assert short["chosen_Q"] == want_q and [r["Q"] for r in short["sweep"]["rows"]] == [2, want_q, 255]
    missed = enc.encode_attr(m["x_dev"], m["r_dev"], target=("psnr", 1000.0), steps=(2, 8, 64))[1]
    assert (missed["chosen_Q"], missed["met"], missed["Q"]) == (2, False, 2)
    with pytest.raises(native.ScpError, match="leave Q at 1"):
        enc.encode_attr(m["x_dev"], m["r_dev"], 4, target=("psnr", 40.0))
    with pytest.raises(native.ScpError, match="unknown kind"):
        enc.encode_attr(m["x_dev"], m["r_dev"], target=("mse", 40.0))
    with pytest.raises(native.ScpError, match="strictly ascending"):
        enc.encode_attr(m["x_dev"], m["r_dev"], target=("psnr", 40.0), steps=(8, 2))
    plain = enc.encode_attr(m["x_dev"], m["r_dev"], 4)[1]
    assert not {"target", "chosen_Q", "met", "sweep"} & set(plain)


@functools.lru_cache(maxsize=None)
def object_cloud():
    """synth_object(0, 4096) with synth_colors through the obj front end: the encoder, the integers, the point colours, and the sweep
    table from lift_ref on lift_ref's leaf colours (test_lift_ref.py ties both to color_ref)."""
    from scp_amd import cli, color
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_colors, synth_object
    xyz = synth_object(0, 4096).astype(np.float32)
    rgb = synth_colors(xyz, 0)
    enc = FrameEncoder(ehem_model(), "obj", 12, spher=False, cylin=False, mullevel=False, device=dev())
    q, _ = cli.obj_ints(xyz, "thing_vox10.ply", dev())
    enc.encode_ints([q], 0, 0.0, len(xyz))
    c = color.point_colors(torch.from_numpy(rgb.astype(np.float32)).to(dev()))
    lv, D = enc.attr_leaves()[0].cpu().numpy(), int(enc.geom.info[0].depth)
    mean, ycc, _ = lift_ref.leaf_colors(q.cpu().numpy(), c.cpu().numpy(), lv, D)
    shell = (functools.partial(lift_ref.forward, lv, ycc, D), lambda Q, f: lift_ref.inverse_rgb(lv, D, Q, f["root"], f["k"]), mean, 5 + 5 + 3 * D + 4)
    return dict(enc=enc, q=q, c=c, leaves=[up(lv, np.int32)], depths=[D], ref=reference_table([shell], 4 + 4, color_ref.tables(), len(xyz)))


def test_object_cloud_meets_its_targets():
    from scp_amd import color
    o = object_cloud()
    enc, ref = o["enc"], o["ref"]

    def encode(Q=1, target=None, chunk=None):
        return enc.encode_color(o["q"], o["c"], Q, chunk=chunk, target=target)

    def decode(data):
        return color.decode_shells(data, o["leaves"], o["depths"])

    assert ref["coded"] == 1
    sweep = enc.color_sweep(o["q"], o["c"])
    targets = pick_targets(ref)
    for kind, value, want_q, next_q in targets:
        rep = check_target(encode, decode, ref, kind, value, want_q, next_q)
        assert rep["sweep"] == sweep
    for r in sweep["rows"]:
        assert sum(r["sse_rgb"]) == r["sse"] and max(r["linf_rgb"]) == r["linf"]
        assert r["psnr_rgb"] == pytest.approx([psnr(v, sweep["leaves"]) for v in r["sse_rgb"]], rel=1e-12)
    kind, value, want_q, next_q = targets[0]
    check_target(encode, decode, ref, kind, value, want_q, next_q, chunk=256)
