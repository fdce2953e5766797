"""Rate per ring on the host: the numpy statement of the definition (tests/ringrate_ref.py) against a literal reading of it on the
oracle's trees, conservation, the dropped node, the report's layout, the command-line flag and its refusals, tools/rd_rings.py, and the
library's argument checks (which come before any HIP call, so they run without a GPU)."""
import glob
import json
import math
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import rate_ref
import ringrate_ref as ref
from conftest import GOLDEN, ROOT, golden


def names(prefix):
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def oracle_trees(orc, name):
    """[(tag, occ, level, parent 0-based, depth)] of one golden point set: its single tree, or the shells of the multi-level form."""
    z = golden(name)
    out = []
    if name.startswith("octmul_"):
        for tag, path in (("00", [0, 0]), ("01", [0, 1]), ("1", [1])):
            if f"p{tag}_empty" in z:
                continue
            t = orc.octree_build(z["pts"], path)
            out.append((tag, t.occ, t.level, t.parent.astype(np.int64) - 1, t.depth, orc.deoctree(t.codes)))
    else:
        t = orc.octree_build(z["pts"])
        out.append(("", t.occ, t.level, t.parent.astype(np.int64) - 1, t.depth, np.unique(z["pts"], axis=0)))
    return out


@pytest.mark.parametrize("name", names("oct_") + names("octmul_"))
def test_reference_equals_the_brute_force_walk_and_conserves_the_bits(orc, name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    trees = oracle_trees(orc, name)
    assert trees
    for tag, occ, level, parent, depth, pts in trees:
        n = len(occ)
        assert parent[0] == -1 and (parent[1:] >= 0).all() and (parent[1:] < np.arange(1, n)).all()
        leaves = ref.leaves_per_node(occ, level, parent, depth)
        assert (leaves >= 1).all() and leaves[0] == len(pts) == int(ref.POP[occ[level == depth]].sum())
        for drop in (False, True):
            bits = rng.uniform(0.0, 12.0, n) * (rng.random(n) > 0.1)          # non-negative, some exact zeros
            if drop:
                bits[-1] = 0.0
            cost = ref.leaf_cost(occ, level, parent, depth, bits)
            brute = ref.leaf_cost_brute(occ, level, parent, depth, bits)
            assert cost.shape == (len(pts),) and np.array_equal(cost, brute), (name, tag)
            total = math.fsum(bits)
            assert abs(float(np.sum(cost)) - total) <= rate_ref.segment_tolerance(n, total), (name, tag, float(np.sum(cost)), total)
            assert abs(math.fsum(cost) - total) <= rate_ref.segment_tolerance(n, total)


def test_a_last_level_that_holds_only_the_dropped_node_gives_finite_costs():
    """A one-leaf shell: one node per level; drop_last leaves the last level without a coded row, the node's bits are 0."""
    depth = 5
    occ = np.array([1, 2, 4, 8, 128], np.uint8)
    level = np.arange(1, depth + 1).astype(np.uint8)
    parent = np.arange(-1, depth - 1)
    row_bits = np.array([3.0, 0.5, 2.25, 1.0])                               # four coded rows for five nodes
    bits = ref.node_bits([1] * depth, True, 8192, row_bits)
    assert bits.tolist() == [3.0, 0.5, 2.25, 1.0, 0.0]
    cost = ref.leaf_cost(occ, level, parent, depth, bits)
    assert cost.shape == (1,) and np.isfinite(cost).all() and cost[0] == ((3.0 + 0.5) + 2.25) + 1.0 + 0.0
    assert np.array_equal(cost, ref.leaf_cost_brute(occ, level, parent, depth, bits))
    # and a root alone (depth 1) that is dropped: no coded row at all
    one = ref.leaf_cost(np.array([3], np.uint8), np.array([1], np.uint8), np.array([-1]), 1, ref.node_bits([1], True, 8192, np.zeros(0)))
    assert one.tolist() == [0.0, 0.0]


def test_node_bits_follow_the_coding_order_of_the_plan():
    from scp_amd.encoder import EncodePlan
    counts = [1, 3, 9, 14]
    for drop in (False, True):
        sizes = counts[:-1] + [counts[-1] - int(drop)]
        order = EncodePlan(sizes, 4).coding_order()
        row_bits = np.arange(1, len(order) + 1, dtype=np.float64)
        want = np.zeros(sum(counts))
        want[order] = row_bits
        assert np.array_equal(ref.node_bits(counts, drop, 4, row_bits), want)


def test_share_of_a_node_is_split_equally_among_the_leaves_below_it():
    """A hand-made tree: root with two children, the first owning three leaves and the second one."""
    occ = np.array([0b11, 0b111, 0b1], np.uint8)
    level = np.array([1, 2, 2], np.uint8)
    parent = np.array([-1, 0, 0])
    assert ref.leaves_per_node(occ, level, parent, 2).tolist() == [4, 3, 1]
    cost = ref.leaf_cost(occ, level, parent, 2, np.array([8.0, 3.0, 5.0]))
    assert cost.tolist() == [3.0, 3.0, 3.0, 7.0]


def test_bins_put_an_edge_point_into_the_upper_ring():
    edges = [0.0, 5.0, 10.0]
    xyz = np.array([[3.0, 4.0, 0.0], [2.9999999, 4.0, 0.0], [0.0, 0.0, 0.0], [6.0, 8.0, 0.0], [1e3, 0, 0]])
    assert ref.bins(xyz, edges).tolist() == [1, 0, 0, 2, 2]
    assert ref.bins(xyz, edges, np.array([2, 0, 1, 0, 1]), 3).tolist() == [7, 0, 3, 2, 5]
    assert ref.bins(xyz + 1.0, edges, view=(1.0, 1.0, 1.0)).tolist() == [1, 0, 0, 2, 2]


def raw_of(records):
    raw = np.zeros((len(records), 4), np.int64)
    raw[:, 0] = [r["leaves"] for r in records]
    for k, name in enumerate(("ideal_bits", "table_bits", "max_ideal_bits")):
        raw[:, 1 + k] = np.array([r[name] for r in records], np.float64).view(np.int64)
    return raw


def test_report_layout_is_plain_python_and_adds_up():
    from scp_amd import metrics, native
    rng = np.random.default_rng(11)
    n, edges, G = 500, [0.0, 10.0, 20.0, 40.0], 3
    ci, ct = rng.uniform(0, 9, n), rng.uniform(0, 9, n)
    b = rng.integers(0, G * len(edges), n)
    b[b == 5] = 6                                                            # an empty bin
    recs = ref.records(ci, ct, b, G * len(edges))
    points = [7, 0, 30, 11]
    rep = metrics.ring_rate_dict(edges, raw_of(recs), points, G)
    assert json.loads(json.dumps(rep)) == rep
    assert sorted(rep) == ["edges", "groups", "rings", "total"] and rep["edges"] == edges
    keys = sorted(["leaves", "ideal_bits", "table_bits", "max_ideal_bits", "ideal_bits_per_leaf", "table_bits_per_leaf"])
    assert len(rep["groups"]) == G and all(len(g) == len(edges) for g in rep["groups"])
    for g in range(G):
        for r in range(len(edges)):
            e, w = rep["groups"][g][r], recs[g * len(edges) + r]
            assert sorted(e) == keys and all(e[k] == w[k] for k in w)
            assert e["ideal_bits_per_leaf"] == (w["ideal_bits"] / w["leaves"] if w["leaves"] else 0.0)
    assert rep["groups"][1][1] == dict(leaves=0, ideal_bits=0.0, table_bits=0.0, max_ideal_bits=0.0, ideal_bits_per_leaf=0.0, table_bits_per_leaf=0.0)
    for r, e in enumerate(rep["rings"]):
        shells = [rep["groups"][g][r] for g in range(G)]
        assert e["leaves"] == sum(s["leaves"] for s in shells) and e["points"] == points[r]
        assert e["ideal_bits"] == math.fsum(s["ideal_bits"] for s in shells) and e["table_bits"] == math.fsum(s["table_bits"] for s in shells)
        assert e["max_ideal_bits"] == max(s["max_ideal_bits"] for s in shells)
        assert e["ideal_bits_per_point"] == (e["ideal_bits"] / points[r] if points[r] else 0.0)
    assert rep["total"]["leaves"] == n and rep["total"]["points"] == sum(points)
    assert rep["total"]["ideal_bits"] == math.fsum(r["ideal_bits"] for r in recs)
    with pytest.raises(native.ScpError, match="records and"):
        metrics.ring_rate_dict(edges, raw_of(recs)[:5], points, G)
    with pytest.raises(native.ScpError, match="records and"):
        metrics.ring_rate_dict(edges, raw_of(recs), points[:3], G)


def test_cli_accepts_rate_rings_and_refuses_where_it_cannot_run():
    from scp_amd import native
    from scp_amd.cli import distortion_request, get_args, parse_ring_edges, refuse_unsupported, rings_request
    base = ["--test_files", "x.bin", "--type", "kitti", "--lidar_level", "12", "--spher"]
    assert parse_ring_edges("0,10,20,40") == (0.0, 10.0, 20.0, 40.0) and parse_ring_edges("0") == (0.0,)
    for mullevel in (False, True):
        off = get_args(base, mullevel)
        assert not hasattr(off, "rate_rings") and rings_request(off) == (False, None)
        for name in ("EHEM", "OctAttention"):
            refuse_unsupported(off, name, mullevel)                                   # as today
        on = get_args(base + ["--rate_rings"], mullevel)
        assert rings_request(on) == (True, None) and distortion_request(on) == (False, None) and not hasattr(on, "rate_report")
        refuse_unsupported(on, "EHEM", mullevel)
        given = get_args(base + ["--rate_rings", "0,2.5,10", "--rate_report", "--metrics", "--distortion_report", "0,2.5,10"], mullevel)
        assert rings_request(given) == (True, (0.0, 2.5, 10.0)) == distortion_request(given) and given.rate_report is True
        refuse_unsupported(given, "EHEM", mullevel)
        with pytest.raises(native.ScpError, match="--rate_rings is available for the EHEM encoders only"):
            refuse_unsupported(on, "OctAttention", mullevel)
        with pytest.raises(native.ScpError, match="--rate_rings with --preproc_path: no geometry of the frame is built"):
            refuse_unsupported(get_args(base + ["--rate_rings", "--preproc_path", "pp/"], mullevel), "EHEM", mullevel)
        with pytest.raises(native.ScpError, match="--rate_rings bins the points by their range .* --type obj has none"):
            refuse_unsupported(get_args(["--test_files", "x.ply", "--type", "obj", "--rate_rings", "0,1"], mullevel), "EHEM", False)
        for bad in ("1,2", "0,3,3", "0,a", ""):
            with pytest.raises(native.ScpError, match="ring edges"):
                get_args(base + ["--rate_rings", bad], mullevel)
    with pytest.raises(native.ScpError, match="--rate_rings: ring edges are comma-separated"):
        parse_ring_edges("0,x")


def test_encoder_without_the_opt_in_says_why(monkeypatch):
    """ring_rate of an encoder made without rate_rows (or without rate) raises with the reason before anything touches a device."""
    from scp_amd import native
    from scp_amd.encoder import FrameEncoder
    enc = FrameEncoder.__new__(FrameEncoder)
    for rate, rows in ((False, False), (True, False), (False, True)):
        enc.rate, enc.rate_rows, enc._rate_rows = rate, rows, None
        with pytest.raises(native.ScpError, match="rate=True and rate_rows=True"):
            enc.ring_rate(None)
    enc.rate, enc.rate_rows = True, True
    with pytest.raises(native.ScpError, match="after a synchronous encode"):
        enc.ring_rate(None)


# ------------------------------------------------------------------------------------------------------------------- tools/rd_rings.py
def _entry(leaves, ideal, points):
    return dict(leaves=leaves, ideal_bits=ideal, table_bits=ideal * 1.01, max_ideal_bits=ideal / max(leaves, 1) * 2,
                ideal_bits_per_leaf=ideal / leaves if leaves else 0.0, table_bits_per_leaf=0.0, points=points,
                ideal_bits_per_point=ideal / points if points else 0.0, table_bits_per_point=0.0)


def _dist_entry(rows, sum_sq):
    return dict(rows=rows, sum_sq=sum_sq)


def test_rd_rings_joins_two_reports_and_refuses_differing_edges(tmp_path):
    rings = dict(edges=[0.0, 10.0, 20.0], rings=[_entry(100, 250.0, 120), _entry(50, 200.0, 40), _entry(0, 0.0, 0)],
                 groups=[], total=_entry(150, 450.0, 160), shell_leaves=[150])
    dist = dict(edges=[0.0, 10.0, 20.0],
                a_to_b=dict(rings=[_dist_entry(120, 1.2), _dist_entry(40, 1.6), _dist_entry(0, 0.0)], total=_dist_entry(160, 2.8)),
                b_to_a=dict(groups=[[_dist_entry(60, 0.3), _dist_entry(50, 1.0), _dist_entry(0, 0.0)], [_dist_entry(40, 0.2), _dist_entry(0, 0.0), _dist_entry(0, 0.0)]],
                            total=_dist_entry(150, 1.5)))
    rj, dj, other = tmp_path / "f.rings.json", tmp_path / "f.dist.json", tmp_path / "g.dist.json"
    rj.write_text(json.dumps(rings))
    dj.write_text(json.dumps(dist))
    other.write_text(json.dumps(dict(dist, edges=[0.0, 10.0, 25.0])))
    tool = os.path.join(ROOT, "tools", "rd_rings.py")
    r = subprocess.run([sys.executable, tool, str(rj), str(dj), "--json"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = json.loads(r.stdout)
    assert [e["leaves"] for e in rows] == [100, 50, 0] and [e["points"] for e in rows] == [120, 40, 0]
    assert rows[0]["bits_per_leaf"] == 2.5 and rows[0]["bits_per_point"] == 250.0 / 120 and rows[1]["bits_per_leaf"] == 4.0
    assert rows[0]["mse_ab"] == 1.2 / 120 and rows[0]["mse_ba"] == math.fsum([0.3, 0.2]) / 100 and rows[1]["mse_ba"] == 1.0 / 50
    assert rows[2] == dict(rows[2], bits_per_leaf=0.0, bits_per_point=0.0, mse_ab=0.0, mse_ba=0.0, hi=None)
    table = subprocess.run([sys.executable, tool, str(rj), str(dj)], capture_output=True, text=True, timeout=60)
    assert table.returncode == 0 and len(table.stdout.strip().splitlines()) == 4 and "bits/leaf" in table.stdout and "20 -" in table.stdout
    bad = subprocess.run([sys.executable, tool, str(rj), str(other)], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "ring edges differ" in bad.stderr and bad.stdout == ""


# --------------------------------------------------------------------------------------------------------- the library's own refusals
def test_library_rejects_bad_ring_rate_arguments_without_a_gpu():
    """The argument checks come before any HIP call: SCP_EINVAL (-1), nothing launched."""
    import ctypes as C
    from scp_amd import native
    L = native.lib()
    z, one = None, 4096                         # NULL and a fake (never dereferenced) non-NULL address
    assert L.scp_rate_leaf_share_workspace_bytes(0, 1) == -1 and L.scp_rate_leaf_share_workspace_bytes((1 << 30) + 1, 1) == -1
    assert L.scp_rate_leaf_share_workspace_bytes(10, 0) == -1 and L.scp_rate_leaf_share_workspace_bytes(10, 63) == -1
    need = L.scp_rate_leaf_share_workspace_bytes(100, 2)
    assert need >= 3 * 8 * 100 + 2 * 40 + 3 * 8 and need % 256 == 0

    def table(rows):
        return np.ascontiguousarray(rows, np.int64)
    good = table([[0, 60, 5, 0], [60, 40, 7, 30]])
    ok = dict(occ=one, level=one, parent=one, N=100, bi=one, bt=one, segs=good, S=2, leaves_total=50, leaves=one, ci=one, ct=one, ws=one, wsb=need)

    def call(**kw):
        k = dict(ok, **kw)
        segs = k["segs"]
        return L.scp_rate_leaf_share(k["occ"], k["level"], k["parent"], k["N"], k["bi"], k["bt"], None if segs is None else segs.ctypes.data, k["S"],
                                     k["leaves_total"], k["leaves"], k["ci"], k["ct"], k["ws"], k["wsb"], None)
    for bad in (dict(occ=z), dict(level=z), dict(parent=z), dict(bi=z), dict(bt=z), dict(segs=None), dict(leaves=z), dict(ci=z), dict(ct=z), dict(ws=z),
                dict(N=0), dict(N=(1 << 30) + 1), dict(leaves_total=0), dict(leaves_total=(1 << 30) + 1), dict(S=0), dict(S=63), dict(wsb=need - 1),
                dict(ws=4100),                                                       # misaligned workspace
                dict(segs=table([[0, 60, 0, 0], [60, 40, 7, 30]])),                  # depth 0
                dict(segs=table([[0, 60, 22, 0], [60, 40, 7, 30]])),                 # depth above SCP_MAX_DEPTH
                dict(segs=table([[0, 60, 5, 0], [61, 39, 7, 30]])),                  # a gap in the node table
                dict(segs=table([[0, 60, 5, 0], [59, 41, 7, 30]])),                  # an overlap
                dict(segs=table([[0, 60, 5, 0], [60, 39, 7, 30]])),                  # the node table not covered
                dict(segs=table([[0, 60, 5, 0], [60, 41, 7, 30]])),                  # past its end
                dict(segs=table([[1, 59, 5, 0], [60, 40, 7, 30]])),                  # not from node 0
                dict(segs=table([[0, 60, 5, 0], [60, 0, 7, 30]]), N=60),             # an empty segment
                dict(segs=table([[0, 60, 5, 1], [60, 40, 7, 30]])),                  # leaves not from 0
                dict(segs=table([[0, 60, 5, 0], [60, 40, 7, 0]])),                   # a segment without leaves
                dict(segs=table([[0, 60, 5, 0], [60, 40, 7, 50]])),                  # the last segment without leaves
                dict(segs=table([[0, 60, 5, 0], [60, 40, 7, 51]]))):                 # a leaf base past the table
        assert call(**bad) == -1, bad
    view = (C.c_double * 3)(0.0, 0.0, 0.0)
    esq = (C.c_double * 3)(0.0, 25.0, 100.0)
    okb = dict(a=one, n=10, view=C.cast(view, C.c_void_p), esq=C.cast(esq, C.c_void_p), R=3, group=z, G=1, bin=one, flag=z)

    def bins(**kw):
        k = dict(okb, **kw)
        return L.scp_ring_bins_f64(k["a"], k["n"], k["view"], k["esq"], k["R"], k["group"], k["G"], k["bin"], k["flag"], None)
    unsorted = (C.c_double * 3)(0.0, 25.0, 25.0)
    negative = (C.c_double * 3)(-1.0, 25.0, 100.0)
    nanview = (C.c_double * 3)(0.0, float("nan"), 0.0)
    wide = (C.c_double * 65)(*[float(i) for i in range(65)])
    for bad in (dict(a=z), dict(view=z), dict(esq=z), dict(bin=z), dict(n=0), dict(n=-1), dict(n=(1 << 30) + 1), dict(R=0), dict(G=0), dict(G=1366),
                dict(esq=C.cast(unsorted, C.c_void_p)), dict(esq=C.cast(negative, C.c_void_p)), dict(view=C.cast(nanview, C.c_void_p)),
                dict(esq=C.cast(wide, C.c_void_p), R=65)):
        assert bins(**bad) == -1, bad
    assert L.scp_share_segments_f64(z, one, z, 10, one, 3, one, None) == -1
    assert L.scp_share_segments_f64(one, z, z, 10, one, 3, one, None) == -1
    assert L.scp_share_segments_f64(one, one, z, 0, one, 3, one, None) == -1
    assert L.scp_share_segments_f64(one, one, z, (1 << 30) + 1, one, 3, one, None) == -1
    assert L.scp_share_segments_f64(one, one, z, 10, z, 3, one, None) == -1
    assert L.scp_share_segments_f64(one, one, z, 10, one, 0, one, None) == -1
    assert L.scp_share_segments_f64(one, one, z, 10, one, 4097, one, None) == -1
    assert L.scp_share_segments_f64(one, one, z, 10, one, 3, z, None) == -1
