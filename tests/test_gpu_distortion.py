"""Distortion report on the device (csrc/distreport.hip, scp_amd/native.py, metrics.py, encoder.py, cli.py) against the numpy statement of
its definitions (tests/distortion_ref.py).

Bounds.  idx, d2, bin, axis, rows, axis_rows, max_sq and hist are exact by construction: equality.  A component is a handful of float64
operations on e, each within an ulp: a few 1e-16 |e|, held to 1e-12 sqrt(d2).  A sum of n <= 8192 non-negative terms in any order is
within n 2^-53 = 1e-12 of the correctly rounded one relative to the sum, on top of the squares' 2e-12: held to 1e-9; sum_r, whose terms
change sign, to 1e-9 sum |e_r|."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distortion_ref as ref
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

SUMS2 = ("sum_sq", "sum_r2", "sum_phi2", "sum_theta2")


def dev():
    return torch.device("cuda:0")


def up(x, dtype=np.float64):
    return torch.from_numpy(np.array(x, dtype)).to(dev())               # a copy: the shared inputs are read-only


def run(a, b, edges, group=None, n_groups=1, view=(0.0, 0.0, 0.0)):
    """One direction on the device -> (split tensors, records) on the host."""
    from scp_amd import native
    s = native.nn_error_split(up(a), up(b), edges, None if group is None else up(group, np.int32), n_groups, view)
    seg = native.dist_segments(s["d2"], s["comp"], s["flag"], s["bin"], n_groups * len(edges))
    host = {k: v.cpu().numpy() for k, v in s.items()}
    return host, seg["raw"].cpu().numpy()


def check_records(raw, want, what=""):
    from scp_amd import native
    rec = native.dist_record_views(raw)
    assert raw.shape == (len(want), 72)
    for k, w in enumerate(want):
        assert rec["rows"][k] == w["rows"] and rec["axis_rows"][k] == w["axis_rows"], (what, k)
        assert rec["max_sq"][k] == w["max_sq"], (what, k)
        assert np.array_equal(rec["hist"][k], w["hist"]), (what, k)
        for name in SUMS2:
            assert abs(rec[name][k] - w[name]) <= 1e-9 * w[name], (what, k, name, rec[name][k], w[name])
        assert abs(rec["sum_r"][k] - w["sum_r"]) <= 1e-9 * w["abs_r"], (what, k, rec["sum_r"][k], w["sum_r"])


def check_direction(a, b, edges, group=None, n_groups=1, view=(0.0, 0.0, 0.0), what=""):
    want = ref.direction(a, b, edges, group, n_groups, view)
    got, raw = run(a, b, edges, group, n_groups, view)
    assert got["idx"].dtype == np.int32 and got["bin"].dtype == np.int32 and got["axis"].dtype == bool and got["comp"].shape == (len(a), 3)
    assert np.array_equal(got["idx"], want["idx"]), what
    assert np.array_equal(got["d2"], want["d2"]), what
    assert np.array_equal(got["bin"], want["bin"]), what
    assert np.array_equal(got["axis"], want["axis"]), what
    err = np.abs(got["comp"] - want["comp"]).max(1)
    print(what, "max component error / sqrt(d2):", float((err / np.sqrt(np.maximum(want["d2"], 1e-300))).max()))
    assert (err <= 1e-12 * np.sqrt(want["d2"])).all(), what
    check_records(raw, want["records"], what)
    return got, raw, want


@functools.lru_cache(maxsize=None)
def fixture(name):
    z = golden("d2_" + name)
    a, b = z["a"].astype(np.float64), z["b"].astype(np.float64)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


FIXTURE_EDGES = {"sphere": [0.0, 9.9, 9.9999999, 10.0, 10.1], "lattice": [0.0, 4.0, 8.0, 12.0]}


# ------------------------------------------------------------------------------------------------------------ kernel against reference
@pytest.mark.parametrize("name,reverse", [("sphere", False), ("sphere", True), ("lattice", False), ("lattice", True)])
def test_kernels_equal_the_reference_on_the_fixtures(name, reverse):
    """d2_sphere (2000 x 1902, tie-free) and d2_lattice (120 x 90, up to 8 equal neighbours, 6 axis points), both directions, with three
    groups and with a sensor off the origin."""
    a, b = fixture(name)
    q, p = (b, a) if reverse else (a, b)
    edges = FIXTURE_EDGES[name]
    got, _, want = check_direction(q, p, edges, what=f"{name} reverse={reverse}")
    if name == "lattice" and not reverse:
        assert got["axis"].sum() == 6
        d = ref.sqdist_rows(q, p)
        assert ((d == d.min(1, keepdims=True)).sum(1) > 1).any()           # ties exist, and the lowest index won (idx equals argmin's)
    group = (np.arange(len(q)) * 7 % 3).astype(np.int32)
    check_direction(q, p, edges, group, 3, what=f"{name} reverse={reverse} groups")
    check_direction(q, p, [0.0, 9.0, 11.0], view=(1.0, -2.0, 0.5), what=f"{name} reverse={reverse} view")


# ------------------------------------------------------------------------------------------------------------------ tile and split edges
@pytest.mark.parametrize("na", [1, 255, 256, 257, 1025])
def test_lowest_index_wins_at_every_tile_and_slice_edge(na):
    """A single point, tails of the 256-query block and of the 1024-point tile, more than one slice of B; every coordinate of both clouds
    is a multiple of 0.25, so that equal distances (exact hits and repeated points of B among them) occur."""
    rng = np.random.default_rng(100 + na)
    a = rng.integers(0, 10, (na, 3)) * 0.25
    tied = 0
    for nb in (1, 1023, 1024, 1025, 2049):
        b = rng.integers(0, 10, (nb, 3)) * 0.25
        want_idx, want_d2 = ref.nearest(a, b)
        got, _ = run(a, b, [0.0, 1.0, 2.0])
        assert np.array_equal(got["idx"], want_idx), (na, nb)
        assert np.array_equal(got["d2"], want_d2), (na, nb)
        d = ref.sqdist_rows(a[:256], b)
        tied += int(((d == d.min(1, keepdims=True)).sum(1) > 1).sum())
    assert tied > 0 or na == 1


# --------------------------------------------------------------------------------------------------------------------------- invariance
def test_permuting_the_searched_cloud_changes_nothing_but_the_indices():
    a, b = fixture("sphere")
    edges = FIXTURE_EDGES["sphere"]
    got, raw = run(a, b, edges)
    again, raw2 = run(a, b, edges)
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    assert np.array_equal(raw, raw2)                                       # the same bits in every run
    perm = np.random.default_rng(3).permutation(len(b))
    moved, raw3 = run(a, b[perm], edges)
    assert np.array_equal(perm[moved["idx"]], got["idx"])
    for k in ("d2", "comp", "bin", "axis"):
        assert np.array_equal(moved[k], got[k]), k
    assert np.array_equal(raw3, raw)


def test_a_bin_depends_on_its_own_rows_only():
    """Other bins' rows, the number of groups and the number of bins leave a bin's record bit-identical."""
    from scp_amd import native
    rng = np.random.default_rng(8)
    n = 5000
    d2 = rng.uniform(0, 4, n)
    comp = rng.normal(0, 1, (n, 3))
    flag = (rng.random(n) < 0.01).astype(np.uint8)
    bins = rng.integers(0, 6, n).astype(np.int32)
    base = native.dist_segments(up(d2), up(comp), up(flag, np.uint8), up(bins, np.int32), 6)["raw"].cpu().numpy()
    keep = bins == 2
    d2b, compb, flagb, binsb = d2.copy(), comp.copy(), flag.copy(), bins.copy()
    d2b[~keep] = rng.uniform(0, 9, int((~keep).sum()))
    compb[~keep] *= 3.0
    binsb[~keep] = rng.integers(3, 40, int((~keep).sum()))                 # other bins, more of them - and none below bin 2 any more
    other = native.dist_segments(up(d2b), up(compb), up(flagb, np.uint8), up(binsb, np.int32), 40)["raw"].cpu().numpy()
    assert np.array_equal(other[2], base[2]) and not np.array_equal(other[3], base[3])
    alone = native.dist_segments(up(d2[keep]), up(comp[keep]), up(flag[keep], np.uint8), up(np.zeros(int(keep.sum())), np.int32), 1)["raw"].cpu().numpy()
    assert np.array_equal(alone[0], base[2])
    # through the whole path: group 0's bins with one group and with three
    a, b = fixture("lattice")
    edges = FIXTURE_EDGES["lattice"]
    one = run(a, b, edges)[1]
    group = np.zeros(len(a), np.int32)
    group[::2] = 2
    three = run(a, b, edges, group, 3)[1]
    even = run(a[::2], b, edges)[1]
    assert one.shape == (4, 72) and three.shape == (12, 72)
    assert np.array_equal(three[8:12], even) and (three[4:8] == 0).all()
    rows = lambda raw: native.dist_record_views(raw)["rows"]
    assert np.array_equal(rows(three[0:4]) + rows(three[8:12]), rows(one))


# --------------------------------------------------------------------------------------------------------------------------------- bins
@pytest.mark.parametrize("sizes", [(1,), (1025, 0, 1, 2049), (0, 0, 3000), tuple([37] * 64)], ids=["one-bin-one-row", "stride", "all-in-last", "64-bins"])
def test_bins_of_every_size_in_arbitrary_order(sizes):
    """Bin ids in arbitrary order; empty bins give all zeros; bins of 1, 1025 and 2049 rows cross the 1024-row stride; all rows in one
    bin; 1 bin and 64 bins."""
    from scp_amd import native
    rng = np.random.default_rng(len(sizes) * 1000 + sum(sizes))
    bins = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    n = len(bins)
    d2 = np.exp2(rng.uniform(-45, 25, n)) * (rng.random(n) > 0.05)          # both tails of the histogram, and exact zeros
    comp = rng.normal(0, 1, (n, 3)) * np.sqrt(d2)[:, None]
    axis = rng.random(n) < 0.03
    comp[axis] = 0.0
    seg = native.dist_segments(up(d2), up(comp), up(axis * native.DIST_FLAG_AXIS, np.uint8), up(bins, np.int32), len(sizes))
    raw = seg["raw"].cpu().numpy()
    want = ref.records(d2, comp, axis, bins, len(sizes))
    check_records(raw, want, str(sizes))
    assert [int(r) for r in seg["rows"].cpu()] == list(sizes)
    for k, size in enumerate(sizes):
        if size == 0:
            assert (raw[k] == 0).all()
    assert seg["hist"].shape == (len(sizes), 64) and seg["sum_sq"].dtype == torch.float64 and seg["rows"].dtype == torch.int64
    # the rows already in bin order, as one stable sort leaves them: the same bits
    order = np.argsort(bins, kind="stable")
    again = native.dist_segments(up(d2[order]), up(comp[order]), up(axis[order] * native.DIST_FLAG_AXIS, np.uint8), up(bins[order], np.int32), len(sizes))
    assert np.array_equal(again["raw"].cpu().numpy(), raw)


def test_one_ring_one_group_and_sixty_four_bins_through_the_whole_path():
    a, b = fixture("lattice")
    check_direction(a, b, [0.0], what="1 x 1")
    group = (np.arange(len(a)) % 8).astype(np.int32)
    check_direction(a, b, [0.0, 2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0], group, 8, what="8 x 8")


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused_before_any_launch():
    from scp_amd import native
    a, b = fixture("lattice")
    A, B = up(a), up(b)
    edges = [0.0, 4.0, 8.0]
    for bad in ([0.0, 8.0, 4.0], [-1.0, 4.0], [1.0, 4.0], [0.0, 4.0, 4.0], [], list(range(65))):
        with pytest.raises(native.ScpError, match="ring edges"):
            native.nn_error_split(A, B, bad)
    for qa, qb in ((A[:, :2], B), (A, B[:0]), (A[:0], B), (A.reshape(-1), B)):
        with pytest.raises(native.ScpError, match="clouds of shape"):
            native.nn_error_split(qa, qb, edges)
    with pytest.raises(native.ScpError, match="bins expected"):
        native.nn_error_split(A, B, edges, n_groups=0)
    with pytest.raises(native.ScpError, match="bins expected"):
        native.nn_error_split(A, B, edges, n_groups=1366)
    group = torch.zeros(len(a), dtype=torch.int32, device=dev())
    group[5] = 3
    with pytest.raises(native.ScpError, match="group values 0 .. 3 outside 0 .. 2"):
        native.nn_error_split(A, B, edges, group, 3)
    group[5] = -1
    with pytest.raises(native.ScpError, match="group values -1 .. 0 outside"):
        native.nn_error_split(A, B, edges, group, 3)
    with pytest.raises(native.ScpError, match="group is a device int32 tensor"):
        native.nn_error_split(A, B, edges, group[:-1], 3)
    with pytest.raises(native.ScpError, match="group is a device int32 tensor"):
        native.nn_error_split(A, B, edges, group.long(), 3)
    with pytest.raises(native.ScpError, match="device tensor required"):
        native.nn_error_split(A.cpu(), B, edges)
    with pytest.raises(native.ScpError, match="device tensor required"):
        native.nn_error_split(A, B.cpu(), edges)
    s = native.nn_error_split(A, B, edges)
    with pytest.raises(native.ScpError, match="device tensor of"):
        native.dist_segments(s["d2"].cpu(), s["comp"], s["flag"], s["bin"], 3)
    with pytest.raises(native.ScpError, match="device tensor of"):
        native.dist_segments(s["d2"], s["comp"], s["axis"], s["bin"], 3)
    with pytest.raises(native.ScpError, match="bins expected"):
        native.dist_segments(s["d2"], s["comp"], s["flag"], s["bin"], 0)
    with pytest.raises(native.ScpError, match="bins expected"):
        native.dist_segments(s["d2"], s["comp"], s["flag"], s["bin"], 4097)
    with pytest.raises(native.ScpError, match="with n >= 1 expected"):
        native.dist_segments(s["d2"], s["comp"][:-1], s["flag"], s["bin"], 3)


def test_kernel_clamps_a_group_out_of_range_and_flags_a_row_without_a_neighbour():
    """What include/scp.h promises of the C entry point itself (the Python binding refuses such groups before the launch, so the call
    goes through ctypes): a group of -1 or n_groups is clamped to 0 or n_groups - 1 and the row flagged, never an out-of-range bin; a
    query with a NaN coordinate reproduces no minimum and gets idx -1, d2 0, components 0 and its flag; every other row is the reference's."""
    import ctypes as C
    from scp_amd import native
    a, b = (x.copy() for x in fixture("lattice"))
    a[7, 1] = np.nan
    edges, G = [0.0, 4.0, 8.0, 12.0], 3
    group = (np.arange(len(a)) % G).astype(np.int32)
    group[3], group[4], group[7] = -1, G, 1
    A, B, Gd = up(a), up(b), up(group, np.int32)
    na = len(a)
    idx = torch.empty(na, dtype=torch.int32, device=dev())
    d2 = torch.empty(na, dtype=torch.float64, device=dev())
    comp = torch.empty((na, 3), dtype=torch.float64, device=dev())
    bins = torch.empty(na, dtype=torch.int32, device=dev())
    flag = torch.empty(na, dtype=torch.uint8, device=dev())
    view = (C.c_double * 3)(0.0, 0.0, 0.0)
    esq = (C.c_double * len(edges))(*[e * e for e in edges])
    rc = native.lib().scp_nn_error_split_f64(A.data_ptr(), na, B.data_ptr(), len(b), C.cast(view, C.c_void_p), C.cast(esq, C.c_void_p), len(edges),
                                             Gd.data_ptr(), G, idx.data_ptr(), d2.data_ptr(), comp.data_ptr(), bins.data_ptr(), flag.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    idx, d2h, comph, binh, flagh = idx.cpu().numpy(), d2.cpu().numpy(), comp.cpu().numpy(), bins.cpu().numpy(), flag.cpu().numpy()
    ok = np.ones(na, bool)
    ok[7] = False
    good_group = np.clip(group, 0, G - 1)
    want = ref.direction(a[ok], b, edges, good_group[ok], G)
    assert np.array_equal(idx[ok], want["idx"]) and np.array_equal(d2h[ok], want["d2"]) and np.array_equal(binh[ok], want["bin"])
    assert (np.abs(comph[ok] - want["comp"]).max(1) <= 1e-12 * np.sqrt(want["d2"])).all()
    assert binh.min() >= 0 and binh.max() < G * len(edges)
    assert binh[3] // len(edges) == 0 and binh[4] // len(edges) == G - 1
    clamped = np.zeros(na, bool)
    clamped[[3, 4]] = True
    assert np.array_equal((flagh & native.DIST_FLAG_GROUP_CLAMPED) != 0, clamped)
    assert np.array_equal((flagh & native.DIST_FLAG_NO_NEIGHBOUR) != 0, ~ok)
    assert idx[7] == -1 and d2h[7] == 0.0 and (comph[7] == 0.0).all() and binh[7] == 1 * len(edges) + 0
    assert np.array_equal((flagh & native.DIST_FLAG_AXIS) != 0, np.r_[want["axis"][:7], False, want["axis"][7:]])
    # the records stay finite: the flagged row counts with d2 = 0
    seg = native.dist_segments(d2, comp, flag, bins, G * len(edges))
    assert int(seg["rows"].sum().item()) == na and bool(torch.isfinite(seg["sum_sq"]).all()) and int(seg["hist"][:, 0].sum().item()) == 1
    with pytest.raises(native.ScpError, match="three finite numbers"):
        native.nn_error_split(A, B, edges, view=(0.0, 0.0))


# ----------------------------------------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("mullevel", [False, True], ids=["L12-spher", "L12-multi-level"])
def test_encoder_report_agrees_with_distortion_and_leaves_the_stream_alone(mullevel):
    from cfgs import ehem_cfg
    from scp_amd import metrics, native
    from scp_amd.encoder import FrameEncoder
    from scp_amd.models import EHEM
    from scp_amd.synth import synth_frame
    from scp_amd.weights import fill_weights
    xyz = synth_frame(0)[::16].copy()
    P = len(xyz)
    assert P == 7500 and len(np.unique(xyz, axis=0)) == P and not ((xyz[:, 0] == 0) & (xyz[:, 1] == 0)).any()
    model = fill_weights(EHEM(ehem_cfg()), 0).to(dev())
    enc = FrameEncoder(model, "kitti", 12, spher=True, mullevel=mullevel, device=dev())
    x = torch.from_numpy(xyz).to(dev())
    res = enc.encode(xyz)
    dist = enc.distortion(x)
    rep = enc.distortion_report(x)
    assert enc.distortion(x) == dist                                          # distortion()'s results do not move
    assert enc.distortion_report(x) == rep                                    # nor does the report from run to run
    json.loads(json.dumps(rep))
    assert rep["edges"] == list(metrics.default_edges("kitti"))
    ab, ba = rep["a_to_b"], rep["b_to_a"]
    print(mullevel, "mse_ab", dist["mse_ab"], ab["total"]["sum_sq"] / P, "shares", [ab["total"][k] / ab["total"]["mse"] for k in ("mse_r", "mse_phi", "mse_theta")])
    assert abs(ab["total"]["sum_sq"] / P - dist["mse_ab"]) <= 1e-12 * dist["mse_ab"]
    pts = enc._reconstructed()
    quant = torch.cat(pts)
    assert ab["total"]["max_sq"] == float(native.nn_sqdist(x.double(), quant).max().item())
    assert ba["total"]["max_sq"] == float(native.nn_sqdist(quant, x.double()).max().item())
    assert sum(e["rows"] for e in ab["rings"]) == P == ab["total"]["rows"] and ab["total"]["axis_rows"] == 0
    assert len(ba["groups"]) == len(pts) == (3 if mullevel else 1) and rep["shell_leaves"] == [int(p.shape[0]) for p in pts]
    for g, p in enumerate(pts):
        assert sum(e["rows"] for e in ba["groups"][g]) == p.shape[0]
        h = p.cpu().numpy()
        want = ref.ring((h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]) + h[:, 2] * h[:, 2], rep["edges"])      # the ring of the RECONSTRUCTED point
        assert [e["rows"] for e in ba["groups"][g]] == [int((want == r).sum()) for r in range(len(rep["edges"]))]
    d1 = metrics.chamfer_psnr(x, quant, 59.70, dropdups=False)                # the docstring's statement: no duplicate merging
    assert abs(ab["total"]["sum_sq"] / P - d1["mse_ab"]) <= 1e-12 * d1["mse_ab"]
    assert abs(ba["total"]["sum_sq"] / quant.shape[0] - d1["mse_ba"]) <= 1e-12 * d1["mse_ba"]
    # other edges on request; other data types must give them
    two = enc.distortion_report(x, edges=[0.0, 25.0])
    assert two["edges"] == [0.0, 25.0] and two["a_to_b"]["total"]["sum_sq"] == pytest.approx(ab["total"]["sum_sq"], rel=1e-12)
    assert two["a_to_b"]["total"]["max_sq"] == ab["total"]["max_sq"] and two["a_to_b"]["total"]["hist"] == ab["total"]["hist"]
    # the stream: identical after the report, and identical to an encoder that never made one
    assert enc.encode(xyz)["bytes"] == res["bytes"]
    assert FrameEncoder(model, "kitti", 12, spher=True, mullevel=mullevel, device=dev()).encode(xyz)["bytes"] == res["bytes"]
    if not mullevel:
        other = FrameEncoder(model, "obj", 12, spher=True, device=dev())
        with pytest.raises(native.ScpError, match="give edges"):
            other.distortion_report(x)


# --------------------------------------------------------------------------------------------------------------------------------- CLI
@pytest.mark.parametrize("script", ["encode.py", "encode_mullevel.py"])
def test_cli_distortion_report_writes_the_json_and_leaves_every_other_file_alone(tmp_path, script):
    from scp_amd.synth import synth_frame, write_kitti_bin
    seq = tmp_path / "seq07"
    seq.mkdir()
    for i in range(2):
        write_kitti_bin(str(seq / f"{i:06d}.bin"), synth_frame(i)[::60])
    runs = {"plain": [], "report": ["--distortion_report"], "all": ["--distortion_report", "0,10,30", "--rate_report", "--metrics"]}
    outs = {}
    for tag, flags in runs.items():
        out = tmp_path / ("out_" + tag)
        cmd = [sys.executable, os.path.join(ROOT, script), "--test_files", str(seq / "*.bin"), "--type", "kitti", "--lidar_level", "12",
               "--spher", "--random_weights", "0", "--out_dir", str(out)] + flags
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.count("D1 mse, r/phi/theta, max    :") == (2 if flags else 0)
        assert r.stdout.count("bpp ideal / table / coded   :") == (2 if tag == "all" else 0) and r.stdout.count("PSNR (D1)") == (2 if tag == "all" else 0)
        outs[tag] = out
    reports = (".dist.json", ".rate.json")
    files = {tag: sorted(p.name for p in out.iterdir() if not p.name.endswith(reports)) for tag, out in outs.items()}
    assert len([f for f in files["plain"] if f.endswith(".bin")]) == 2 and any(f.endswith(".dat") for f in files["plain"])
    assert any(f.endswith(".scp.json") for f in files["plain"])
    assert files["report"] == files["plain"] == files["all"]
    for tag in ("report", "all"):
        for f in files["plain"]:
            assert (outs[tag] / f).read_bytes() == (outs["plain"] / f).read_bytes(), (tag, f)
    assert not [p for p in outs["plain"].iterdir() if p.name.endswith(reports)]
    for tag, n_rings in (("report", 9), ("all", 3)):
        docs = sorted(p for p in outs[tag].iterdir() if p.name.endswith(".dist.json"))
        assert [d.name[:-len(".dist.json")] + ".bin" for d in docs] == [f for f in files["plain"] if f.endswith(".bin")]
        assert len([p for p in outs[tag].iterdir() if p.name.endswith(".rate.json")]) == (2 if tag == "all" else 0)
        for d in docs:
            rep = json.load(open(d))
            assert rep["lidar_level"] == 12 and rep["type"] == "kitti" and len(rep["edges"]) == n_rings
            shells = 3 if script == "encode_mullevel.py" else 1
            assert len(rep["shell_leaves"]) == shells == len(rep["b_to_a"]["groups"])
            ab, ba = rep["a_to_b"], rep["b_to_a"]
            assert sum(e["rows"] for e in ab["rings"]) == ab["total"]["rows"] == rep["n_points"]
            assert [sum(e["rows"] for e in g) for g in ba["groups"]] == rep["shell_leaves"] and ba["total"]["rows"] == sum(rep["shell_leaves"])
            for entries, total in ((ab["rings"], ab["total"]), ([e for g in ba["groups"] for e in g], ba["total"])):
                for k in ("sum_sq", "sum_r2", "sum_phi2", "sum_theta2", "sum_r"):
                    assert total[k] == math.fsum(e[k] for e in entries), k
                assert total["max_sq"] == max(e["max_sq"] for e in entries)
