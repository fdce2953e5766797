"""Depth report on the host: the numpy statement of its definitions (tests/depth_ref.py) on the oracle's trees - prefix costs against
ringrate_ref, conservation per truncation depth, the cells of every LOD against the trees' own levels -, metrics.lod_centres and
metrics.depth_dict, the command-line flags and their refusals, tools/rd_depth.py, and the library's argument checks (which come before
any HIP call, so they run without a GPU)."""
import json
import math
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import depth_ref as ref
import rate_ref
import ringrate_ref as rr
from conftest import ROOT
from test_ringrate_ref import names, oracle_trees, raw_of


@pytest.mark.parametrize("name", names("oct_") + names("octmul_"))
def test_prefix_costs_cut_the_chain_short_and_conserve_the_bits_of_the_levels_kept(orc, name):
    rng = np.random.default_rng(zlib.crc32(name.encode()) ^ 0x5EED)
    trees = oracle_trees(orc, name)
    assert trees
    for tag, occ, level, parent, depth, pts in trees:
        n = len(occ)
        bits = rng.uniform(0.0, 12.0, n) * (rng.random(n) > 0.1)              # non-negative, some exact zeros
        bits[-1] = 0.0
        full = rr.leaf_cost(occ, level, parent, depth, bits)
        stack = ref.planes(occ, level, parent, depth, bits, 21)
        assert stack.shape == (22, len(full)) and stack.dtype == np.float64
        for k in sorted({0, 1, 3, depth - 1, depth, depth + 2, 21}):
            cost = ref.prefix_cost(occ, level, parent, depth, bits, k)
            assert cost.shape == full.shape and cost.dtype == np.float64
            assert np.array_equal(stack[k], cost) and not np.signbit(stack[k]).any(), (name, tag, k)      # one climb gives every plane
            if k == 0:
                assert np.array_equal(cost, full), (name, tag)                # cost_0 is the rate per ring's cost, bit for bit
            if k >= depth:
                assert (cost == 0.0).all() and not np.signbit(cost).any(), (name, tag, k)       # +0.0
                continue
            kept = bits[np.asarray(level) <= depth - k]
            total = math.fsum(kept)
            assert abs(math.fsum(cost) - total) <= rate_ref.segment_tolerance(len(kept), total), (name, tag, k, math.fsum(cost), total)
            assert (cost <= full).all()                                       # non-negative shares: a shorter chain never costs more
        assert np.array_equal(ref.planes(occ, level, parent, depth, bits, 0)[0], full)


@pytest.mark.parametrize("name", names("oct_") + names("octmul_"))
def test_cells_of_every_lod_are_the_nodes_of_one_level_and_every_leaf_lies_in_exactly_one(orc, name):
    for tag, occ, level, parent, depth, pts in oracle_trees(orc, name):
        leaves = orc.deoctree(occ).astype(np.int64)                           # the tree's leaves in the tree's own (Morton) order
        assert sorted(map(tuple, leaves)) == sorted(map(tuple, np.asarray(pts).astype(np.int64)))
        level = np.asarray(level)
        per_node = rr.leaves_per_node(occ, level, parent, depth)
        assert len(leaves) == per_node[0]
        for k in range(0, depth):
            cells, cell_of = ref.cell_origins(leaves, k)
            if k == 0:
                assert len(cells) == len(leaves) and np.array_equal(cell_of, np.arange(len(leaves)))
                assert np.array_equal(ref.centres(leaves, 0), leaves.astype(np.float64))
                continue
            nodes = np.flatnonzero(level == depth - k + 1)
            assert len(cells) == len(nodes), (name, tag, k)
            # one cell per leaf, and as many leaves per cell as the tree counts below the node - in node (Morton) order
            assert cell_of.shape == (len(leaves),) and cell_of.min() == 0 and cell_of.max() == len(cells) - 1
            assert np.array_equal(np.bincount(cell_of, minlength=len(cells)), per_node[nodes]), (name, tag, k)
            assert (np.diff(cell_of) >= 0).all()                              # leaves in Morton order: the cells come in node order
            o = cells[cell_of]
            assert ((leaves >= o) & (leaves < o + 2 ** k)).all()
            c = ref.centres(leaves, k)
            assert np.array_equal(c, o + (2 ** k - 1) / 2.0) and np.array_equal(c * 2, np.round(c * 2))      # exact half-integers


def test_lod_centres_equal_the_reference_on_tensors_and_arrays():
    import torch
    from scp_amd import metrics, native
    rng = np.random.default_rng(3)
    x = rng.integers(0, 2 ** 20, (200, 3)).astype(np.int32)
    for k in (0, 1, 2, 5, 19):
        want = ref.centres(x, k)
        got = metrics.lod_centres(x, k)
        assert got.dtype == np.float64 and np.array_equal(got, want)
        t = metrics.lod_centres(torch.from_numpy(x), k)
        assert t.dtype == torch.float64 and np.array_equal(t.numpy(), want)
        origins = ((x.astype(np.int64) >> k) << k)
        assert np.array_equal(metrics.lod_centres(origins, k), want)          # cells or leaves: the same centres
    assert metrics.lod_centres(np.array([[5, 6, 7]]), 2).tolist() == [[5.5, 5.5, 5.5]]
    for bad in (-1, 22):
        with pytest.raises(native.ScpError, match="lod_centres"):
            metrics.lod_centres(x, bad)


def test_depth_dict_is_plain_python_and_holds_ring_rate_dict_per_plane():
    from scp_amd import metrics, native
    rng = np.random.default_rng(12)
    n, edges, G, K = 400, [0.0, 10.0, 20.0], 2, 2
    b = rng.integers(0, G * len(edges), n)
    ci = rng.uniform(0, 9, (K + 1, n))
    ct = rng.uniform(0, 9, (K + 1, n))
    raw = np.stack([raw_of(rr.records(ci[k], ct[k], b, G * len(edges))) for k in range(K + 1)])
    points = [7, 0, 30]
    cells = [[300, 100], [200, 80], [90, 40]]
    dist = [dict(edges=edges, tag=k) for k in range(K + 1)]
    d1 = [dict(chamfer=0.1 * k, psnr=70.0 - k, mse_ab=0.0, mse_ba=0.0) for k in range(K + 1)]
    rep = metrics.depth_dict(edges, raw, points, G, cells, dist, d1, [300, 100], [12, 13])
    assert json.loads(json.dumps(rep)) == rep
    assert sorted(rep) == ["edges", "levels", "shell_depths", "shell_leaves"] and rep["edges"] == edges
    assert rep["shell_leaves"] == [300, 100] and rep["shell_depths"] == [12, 13] and len(rep["levels"]) == K + 1
    for k, lv in enumerate(rep["levels"]):
        assert sorted(lv) == ["cells", "d1", "distortion", "drop", "rate"] and lv["drop"] == k and lv["cells"] == cells[k]
        assert lv["rate"] == metrics.ring_rate_dict(edges, raw[k], points, G) and lv["distortion"] == dist[k] and lv["d1"] == d1[k]
    with pytest.raises(native.ScpError, match="depth report"):
        metrics.depth_dict(edges, raw[:2], points, G, cells, dist, d1, [300, 100], [12, 13])
    with pytest.raises(native.ScpError, match="depth report"):
        metrics.depth_dict(edges, raw, points, G, cells, dist, d1, [300], [12, 13])


def test_cli_accepts_depth_report_and_lod_and_refuses_where_they_cannot_run():
    from scp_amd import native
    from scp_amd.cli import depth_request, get_args, get_decode_args, parse_depth_report, refuse_unsupported, rings_request
    base = ["--test_files", "x.bin", "--type", "kitti", "--lidar_level", "12", "--spher"]
    assert parse_depth_report("3") == (3, None) and parse_depth_report("2:0,10,20") == (2, (0.0, 10.0, 20.0)) and parse_depth_report(":0,5") == (4, (0.0, 5.0))
    for mullevel in (False, True):
        off = get_args(base, mullevel)
        assert not hasattr(off, "depth_report") and depth_request(off) == (False, None, None)
        for name in ("EHEM", "OctAttention"):
            refuse_unsupported(off, name, mullevel)                                   # as today
        on = get_args(base + ["--depth_report"], mullevel)
        assert depth_request(on) == (True, 4, None) and rings_request(on) == (False, None) and not hasattr(on, "rate_report")
        refuse_unsupported(on, "EHEM", mullevel)
        given = get_args(base + ["--depth_report", "2:0,2.5,10", "--rate_rings", "0,2.5,10", "--rate_report", "--metrics", "--distortion_report"], mullevel)
        assert depth_request(given) == (True, 2, (0.0, 2.5, 10.0)) and rings_request(given) == (True, (0.0, 2.5, 10.0))
        refuse_unsupported(given, "EHEM", mullevel)
        with pytest.raises(native.ScpError, match="--depth_report is available for the EHEM encoders only"):
            refuse_unsupported(on, "OctAttention", mullevel)
        with pytest.raises(native.ScpError, match="--depth_report with --preproc_path: no geometry of the frame is built"):
            refuse_unsupported(get_args(base + ["--depth_report", "--preproc_path", "pp/"], mullevel), "EHEM", mullevel)
        with pytest.raises(native.ScpError, match="--depth_report bins the points by their range .* --type obj has none"):
            refuse_unsupported(get_args(["--test_files", "x.ply", "--type", "obj", "--depth_report"], mullevel), "EHEM", False)
        for bad in ("x", "-1", "22", "2:1,2", "2:0,a"):
            with pytest.raises(native.ScpError, match="--depth_report|ring edges"):
                get_args(base + ["--depth_report", bad], mullevel)
    assert get_decode_args([]).lod == 0 and get_decode_args(["--lod", "3"]).lod == 3


def test_lod_outside_the_shells_depths_is_refused_with_the_reason():
    from scp_amd import native
    from scp_amd.decoder import check_lod
    assert check_lod(0, [12]) == 0 and check_lod(11, [12]) == 11 and check_lod(12, [13, 14, 15]) == 12
    for lod, depths in ((12, [12]), (-1, [12]), (13, [13, 14, 15]), (True, [12]), (1.0, [12])):
        with pytest.raises(native.ScpError, match=r"outside 0 \.\. "):
            check_lod(lod, depths)


def test_encoder_without_the_opt_in_says_why():
    from scp_amd import native
    from scp_amd.encoder import FrameEncoder
    enc = FrameEncoder.__new__(FrameEncoder)
    for rate, rows in ((False, False), (True, False), (False, True)):
        enc.rate, enc.rate_rows, enc._rate_rows = rate, rows, None
        with pytest.raises(native.ScpError, match="rate=True and rate_rows=True"):
            enc.depth_report(None)
    enc.rate, enc.rate_rows = True, True
    with pytest.raises(native.ScpError, match="after a synchronous encode"):
        enc.depth_report(None)


# ------------------------------------------------------------------------------------------------------------------- tools/rd_depth.py
def _rate_entry(ideal, points):
    return dict(leaves=points, ideal_bits=ideal, table_bits=ideal * 1.01, points=points, ideal_bits_per_point=ideal / points if points else 0.0)


def _level(k, ideal, sum_sq, points):
    return dict(drop=k, cells=[sum(points) >> k],
                rate=dict(rings=[_rate_entry(i, p) for i, p in zip(ideal, points)], total=_rate_entry(math.fsum(ideal), sum(points))),
                distortion=dict(a_to_b=dict(rings=[dict(rows=p, sum_sq=s) for s, p in zip(sum_sq, points)], total=dict(rows=sum(points), sum_sq=math.fsum(sum_sq)))),
                d1=dict(psnr=70.0 - 6 * k))


def test_rd_depth_prints_bits_error_and_the_marginal_db_per_bit(tmp_path):
    points = [100, 50, 0]
    doc = dict(edges=[0.0, 10.0, 20.0], shell_leaves=[140], shell_depths=[12],
               levels=[_level(0, [400.0, 300.0, 0.0], [1.0, 2.0, 0.0], points), _level(1, [200.0, 100.0, 0.0], [4.0, 8.0, 0.0], points),
                       _level(2, [100.0, 100.0, 0.0], [16.0, 8.0, 0.0], points)])
    f = tmp_path / "f.depth.json"
    f.write_text(json.dumps(doc))
    tool = os.path.join(ROOT, "tools", "rd_depth.py")
    r = subprocess.run([sys.executable, tool, str(f), "--json"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = json.loads(r.stdout)
    assert len(rows) == 4 and [e["ring"] for e in rows] == [0, 1, 2, "total"]
    first = rows[0]["levels"]
    assert [e["drop"] for e in first] == [0, 1, 2] and [e["bits_per_point"] for e in first] == [4.0, 2.0, 1.0]
    assert [e["mse_ab"] for e in first] == [0.01, 0.04, 0.16]
    # level D - k buys 10 log10(mse_{k+1} / mse_k) dB for the bits per point it adds
    assert first[0]["db_per_bit"] == pytest.approx(10 * math.log10(4.0) / 2.0) and first[1]["db_per_bit"] == pytest.approx(10 * math.log10(4.0) / 1.0)
    assert first[2]["db_per_bit"] is None                                     # the coarsest level of the report: nothing to compare with
    second = rows[1]["levels"]
    assert second[1]["db_per_bit"] is None and second[1]["gain_db"] == 0.0    # a level that costs this ring nothing
    assert all(e["bits_per_point"] == 0.0 and e["mse_ab"] == 0.0 and e["db_per_bit"] is None for e in rows[2]["levels"])       # an empty ring
    assert rows[3]["levels"][0]["bits_per_point"] == 700.0 / 150
    table = subprocess.run([sys.executable, tool, str(f)], capture_output=True, text=True, timeout=60)
    assert table.returncode == 0 and "dB/bit" in table.stdout and "20 -" in table.stdout and "total" in table.stdout
    bad = tmp_path / "g.depth.json"
    bad.write_text(json.dumps(dict(edges=[0.0])))
    r = subprocess.run([sys.executable, tool, str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "levels" in r.stderr and r.stdout == ""


# --------------------------------------------------------------------------------------------------------- the library's own refusals
def test_library_rejects_bad_depth_share_arguments_without_a_gpu():
    """The argument checks come before any HIP call: SCP_EINVAL (-1), nothing launched."""
    from scp_amd import native
    L = native.lib()
    z, one = None, 4096                         # NULL and a fake (never dereferenced) non-NULL address
    assert L.scp_rate_depth_share_workspace_bytes(0, 1) == -1 and L.scp_rate_depth_share_workspace_bytes((1 << 30) + 1, 1) == -1
    assert L.scp_rate_depth_share_workspace_bytes(10, 0) == -1 and L.scp_rate_depth_share_workspace_bytes(10, 63) == -1
    need = L.scp_rate_depth_share_workspace_bytes(100, 2)
    assert need >= 3 * 8 * 100 + 2 * 40 + 3 * 8 and need % 256 == 0

    def table(rows):
        return np.ascontiguousarray(rows, np.int64)
    good = table([[0, 60, 5, 0], [60, 40, 7, 30]])
    ok = dict(occ=one, level=one, parent=one, N=100, bi=one, bt=one, segs=good, S=2, leaves_total=50, drop=2, leaves=one, ci=one, ct=one, ws=one, wsb=need)

    def call(**kw):
        k = dict(ok, **kw)
        segs = k["segs"]
        return L.scp_rate_depth_share(k["occ"], k["level"], k["parent"], k["N"], k["bi"], k["bt"], None if segs is None else segs.ctypes.data, k["S"],
                                      k["leaves_total"], k["drop"], k["leaves"], k["ci"], k["ct"], k["ws"], k["wsb"], None)
    for bad in (dict(occ=z), dict(level=z), dict(parent=z), dict(bi=z), dict(bt=z), dict(segs=None), dict(leaves=z), dict(ci=z), dict(ct=z), dict(ws=z),
                dict(N=0), dict(N=(1 << 30) + 1), dict(leaves_total=0), dict(leaves_total=(1 << 30) + 1), dict(S=0), dict(S=63), dict(wsb=need - 1),
                dict(ws=4100),                                                       # misaligned workspace
                dict(drop=-1), dict(drop=native.MAX_DEPTH + 1),                      # max_drop outside 0 .. SCP_MAX_DEPTH
                dict(segs=table([[0, 60, 0, 0], [60, 40, 7, 30]])),                  # depth 0
                dict(segs=table([[0, 60, 22, 0], [60, 40, 7, 30]])),                 # depth above SCP_MAX_DEPTH
                dict(segs=table([[0, 60, 5, 0], [61, 39, 7, 30]])),                  # a gap in the node table
                dict(segs=table([[0, 60, 5, 0], [60, 41, 7, 30]])),                  # past its end
                dict(segs=table([[0, 60, 5, 1], [60, 40, 7, 30]])),                  # leaves not from 0
                dict(segs=table([[0, 60, 5, 0], [60, 40, 7, 50]]))):                 # the last segment without leaves
        assert call(**bad) == -1, bad

    def seg(ci=one, ct=one, n=10, off=one, bins=3, depths=2, stride=10, out=one):
        return L.scp_share_segments_depth_f64(ci, ct, z, n, off, bins, depths, stride, out, None)
    for bad in (dict(ci=z), dict(ct=z), dict(off=z), dict(out=z), dict(n=0), dict(n=(1 << 30) + 1, stride=(1 << 30) + 1), dict(bins=0), dict(bins=4097),
                dict(depths=0), dict(depths=native.MAX_DEPTH + 2), dict(stride=9), dict(stride=(1 << 30) + 1)):
        assert seg(**bad) == -1, bad
