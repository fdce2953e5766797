"""Rate per ring on the device (csrc/ringrate.hip, scp_amd/native.py, metrics.py, encoder.py, cli.py) against the numpy statement of its
definition (tests/ringrate_ref.py).

Bounds.  leaves, both leaf costs (a fixed sequence of IEEE float64 operations), the bins, a bin's leaf count and its maximum are exact:
equality.  A bin's two sums are sums of at most 8192 non-negative terms in a fixed order: within n 2^-53 = 1e-12 of the correctly
rounded one relative to the sum - held to 1e-9, the bound test_gpu_distortion.py derives for such sums.  Over a whole frame the bins'
sums are compared with the rate report's through rate_ref.segment_tolerance (every node's bits are handed out in equal parts, each
division and each of the at most 21 additions per leaf within an ulp).

On the parent commit none of this exists: every test here fails there (no symbols, no method, no flag)."""
import ctypes as C
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rate_ref
import ringrate_ref as ref
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

SHELLS = ([0, 0], [0, 1], [1])


def dev():
    return torch.device("cuda:0")


def up(x, dtype=np.float64):
    return torch.from_numpy(np.array(x, dtype)).to(dev())               # a copy: the shared inputs are read-only


def pts_of(name):
    return np.ascontiguousarray(golden(name)["pts"], np.int32)


# name -> the segments of ONE Geom.build call: [(points, path, drop_last)]
CASES = {
    "single-point": lambda: [(pts_of("oct_single_one"), None, False)],
    "single-point-depth4": lambda: [(pts_of("oct_single"), None, False)],
    "single-leaf-under-a-shell-path": lambda: [(np.array([[5, 1, 2], [15, 3, 3]], np.int32), [0, 1], True)],
    "line": lambda: [(pts_of("oct_line_x"), None, False)],
    "duplicates": lambda: [(pts_of("oct_dups_shuffled"), None, False)],
    "depth-15-coordinates": lambda: [(pts_of("oct_pow2max15"), None, False)],
    "deep": lambda: [(pts_of("oct_deep300"), None, False)],
    "frame5k-single-level": lambda: [(pts_of("oct_frame5k_L12"), None, False)],
    "frame5k-three-shells": lambda: [(pts_of("octmul_frame5k_L14"), p, True) for p in SHELLS],
    "two-frames-three-shells": lambda: [(pts_of(n), p, True) for n in ("octmul_frame5k_L14", "octmul_skew") for p in SHELLS],
    "skew-then-frame5k": lambda: [(pts_of("oct_skew2000"), None, False), (pts_of("oct_frame5k_L12"), None, False)],
}


def build(case):
    from scp_amd import native
    segs = CASES[case]()
    q = torch.from_numpy(np.concatenate([p for p, _, _ in segs])).to(dev())
    g, off, layout = native.Geom(), 0, []
    for p, path, drop in segs:
        layout.append((off, len(p), path, drop))
        off += len(p)
    g.build(q, layout)
    return g


def bits_for(g, seed):
    """Random non-negative bits per node, some exact zeros; 0 for the node a drop_last segment leaves uncoded."""
    rng = np.random.default_rng(seed)
    bi = rng.uniform(0.0, 12.0, g.total_nodes) * (rng.random(g.total_nodes) > 0.1)
    bt = rng.uniform(0.0, 12.0, g.total_nodes)
    for s, i in enumerate(g.info):
        if g.segments[s][3]:
            bi[i.node_base + i.n_nodes - 1] = bt[i.node_base + i.n_nodes - 1] = 0.0
    return bi, bt


def run_share(g, bi, bt):
    from scp_amd import native
    nd = g.nodes(("occ", "level", "parent"))
    out = native.rate_leaf_share(nd["occ"], nd["level"], nd["parent"], up(bi), up(bt), native.share_table(g.info), sum(int(i.n_leaves) for i in g.info))
    return {k: v.cpu().numpy() for k, v in nd.items()}, {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def solved(case):
    """(geometry info, node columns, bits, device results, reference results) of one case - computed once, shared, read-only."""
    g = build(case)
    bi, bt = bits_for(g, 17)
    nd, got = run_share(g, bi, bt)
    want_leaves, want_i, want_t = [], [], []
    for i in g.info:
        sl = slice(int(i.node_base), int(i.node_base + i.n_nodes))
        occ, level = nd["occ"][sl], nd["level"][sl]
        parent = np.where(nd["parent"][sl] < 0, -1, nd["parent"][sl].astype(np.int64) - int(i.node_base))
        want_leaves.append(ref.leaves_per_node(occ, level, parent, i.depth))
        want_i.append(ref.leaf_cost(occ, level, parent, i.depth, bi[sl]))
        want_t.append(ref.leaf_cost(occ, level, parent, i.depth, bt[sl]))
    want = dict(leaves=np.concatenate(want_leaves), cost_ideal=np.concatenate(want_i), cost_table=np.concatenate(want_t))
    for d in (nd, got, want):
        for v in d.values():
            v.setflags(write=False)
    info = [(int(i.node_base), int(i.n_nodes), int(i.depth), int(i.n_leaves)) for i in g.info]
    return info, nd, (bi, bt), got, want


# ------------------------------------------------------------------------------------------------------------ kernels against reference
@pytest.mark.parametrize("case", [c for c in CASES if c != "skew-then-frame5k"])
def test_leaves_and_leaf_costs_equal_the_reference(case):
    info, nd, (bi, bt), got, want = solved(case)
    assert got["leaves"].dtype == np.int64 and got["cost_ideal"].dtype == np.float64 and got["cost_table"].dtype == np.float64
    assert len(want["cost_ideal"]) == sum(n for _, _, _, n in info)
    assert np.array_equal(got["leaves"], want["leaves"]), case
    assert np.array_equal(got["cost_ideal"], want["cost_ideal"]), case
    assert np.array_equal(got["cost_table"], want["cost_table"]), case
    assert (got["leaves"] >= 1).all() and np.isfinite(got["cost_ideal"]).all()
    for base, n, depth, n_leaves in info:
        assert got["leaves"][base] == n_leaves
    total = math.fsum(bi)
    print(case, "nodes", len(bi), "leaves", len(got["cost_ideal"]), "sum of costs - sum of bits:", float(np.sum(got["cost_ideal"])) - total)
    assert abs(float(np.sum(got["cost_ideal"])) - total) <= rate_ref.segment_tolerance(len(bi), total)


def test_the_one_leaf_shell_has_no_row_on_its_last_level_and_still_works():
    info, nd, (bi, bt), got, want = solved("single-leaf-under-a-shell-path")
    assert info == [(0, 4, 4, 1)] and nd["level"].tolist() == [1, 2, 3, 4] and bi[3] == 0.0
    assert got["cost_ideal"].tolist() == [((bi[0] + bi[1]) + bi[2]) + bi[3]]


def test_a_frame_costs_the_same_alone_and_as_the_second_frame_of_a_build():
    alone, both = solved("frame5k-single-level"), solved("skew-then-frame5k")
    (base, n, depth, n_leaves) = both[0][1]
    assert base > 0 and (n, depth, n_leaves) == alone[0][0][1:]
    # the same bits for the frame's nodes in both builds
    bi, bt = alone[2]
    g = build("skew-then-frame5k")
    bi2, bt2 = (np.concatenate([x[:base], y]) for x, y in zip(both[2], (bi, bt)))
    _, got = run_share(g, bi2, bt2)
    first_leaves = both[0][0][3]
    assert np.array_equal(got["cost_ideal"][first_leaves:], alone[3]["cost_ideal"])
    assert np.array_equal(got["cost_table"][first_leaves:], alone[3]["cost_table"])
    assert np.array_equal(got["leaves"][base:], alone[3]["leaves"])
    assert np.array_equal(got["cost_ideal"][:first_leaves], both[3]["cost_ideal"][:first_leaves])      # and the first frame does not care either


# ---------------------------------------------------------------------------------------------------------------------------- bin sums
def check_records(raw, want, what=""):
    from scp_amd import native
    rec = native.share_record_views(raw)
    assert raw.shape == (len(want), 4)
    for k, w in enumerate(want):
        assert rec["leaves"][k] == w["leaves"] and rec["max_ideal_bits"][k] == w["max_ideal_bits"], (what, k)
        for name in ("ideal_bits", "table_bits"):
            assert abs(rec[name][k] - w[name]) <= 1e-9 * w[name], (what, k, name, rec[name][k], w[name])


def test_bins_of_every_size_sum_exactly_as_promised():
    """Bins of 0, 1, 1023, 1024, 1025 and 2049 rows (around the 1024-row stride), bin ids in arbitrary order."""
    from scp_amd import native
    sizes = (1025, 0, 1, 2049, 1023, 1024)
    rng = np.random.default_rng(5)
    bins = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    n = len(bins)
    ci = np.exp2(rng.uniform(-30, 6, n)) * (rng.random(n) > 0.05)
    ct = rng.uniform(0, 20, n)
    seg = native.share_segments(up(ci), up(ct), up(bins, np.int32), len(sizes))
    raw = seg["raw"].cpu().numpy()
    check_records(raw, ref.records(ci, ct, bins, len(sizes)), "sizes")
    assert [int(v) for v in seg["leaves"].cpu()] == list(sizes) and (raw[1] == 0).all()
    assert seg["leaves"].dtype == torch.int64 and seg["ideal_bits"].dtype == torch.float64 and seg["max_ideal_bits"].shape == (len(sizes),)
    again = native.share_segments(up(ci), up(ct), up(bins, np.int32), len(sizes))["raw"].cpu().numpy()
    assert np.array_equal(again, raw)                                       # the same bits in every run
    order = np.argsort(bins, kind="stable")                                 # the rows already in bin order: the same bits
    assert np.array_equal(native.share_segments(up(ci[order]), up(ct[order]), up(bins[order], np.int32), len(sizes))["raw"].cpu().numpy(), raw)


def test_a_bin_depends_on_its_own_rows_only():
    """Other bins' rows, the number of groups and the number of bins leave a bin's record bit-identical."""
    from scp_amd import native
    rng = np.random.default_rng(8)
    n = 5000
    ci, ct = rng.uniform(0, 4, n), rng.uniform(0, 4, n)
    bins = rng.integers(0, 6, n).astype(np.int32)
    base = native.share_segments(up(ci), up(ct), up(bins, np.int32), 6)["raw"].cpu().numpy()
    keep = bins == 2
    cib, ctb, binsb = ci.copy(), ct.copy(), bins.copy()
    cib[~keep] = rng.uniform(0, 9, int((~keep).sum()))
    ctb[~keep] *= 3.0
    binsb[~keep] = rng.integers(3, 40, int((~keep).sum()))                 # other bins, more of them - and none below bin 2 any more
    other = native.share_segments(up(cib), up(ctb), up(binsb, np.int32), 40)["raw"].cpu().numpy()
    assert np.array_equal(other[2], base[2]) and not np.array_equal(other[3], base[3])
    alone = native.share_segments(up(ci[keep]), up(ct[keep]), up(np.zeros(int(keep.sum())), np.int32), 1)["raw"].cpu().numpy()
    assert np.array_equal(alone[0], base[2])
    # n_groups: group 0's bins with one group and with three, through ring_bins
    xyz = rng.uniform(-30, 30, (n, 3))
    edges = [0.0, 10.0, 20.0, 40.0]
    one = native.share_segments(up(ci[::2]), up(ct[::2]), native.ring_bins(up(xyz[::2]), edges), 4)["raw"].cpu().numpy()
    group = np.zeros(n, np.int32)
    group[1::2] = 2
    three = native.share_segments(up(ci), up(ct), native.ring_bins(up(xyz), edges, up(group, np.int32), 3), 12)["raw"].cpu().numpy()
    assert np.array_equal(three[0:4], one) and (three[4:8] == 0).all() and three[8:12, 0].sum() == n // 2


# --------------------------------------------------------------------------------------------------------------------------- ring bins
def test_ring_bins_equal_the_distortion_reports_bins_integer_for_integer():
    from scp_amd import native
    z = golden("d2_sphere")
    a, b = z["a"].astype(np.float64), z["b"].astype(np.float64)
    on_edge = np.array([[6.0, 8.0, 0.0], [0.0, 0.0, 10.0], [-10.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 9.9, 0.0], [0.0, 0.0, -10.1]])
    a = np.concatenate([a, on_edge])
    edges = [0.0, 9.9, 9.9999999, 10.0, 10.1]
    group = (np.arange(len(a)) * 7 % 3).astype(np.int32)
    for view in ((0.0, 0.0, 0.0), (1.0, -2.0, 0.5)):
        want = native.nn_error_split(up(a), up(b), edges, up(group, np.int32), 3, view)["bin"].cpu().numpy()
        got = native.ring_bins(up(a), edges, up(group, np.int32), 3, view)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(got.cpu().numpy(), ref.bins(a, edges, group, 3, view))
        plain = native.ring_bins(up(a), edges, view=view).cpu().numpy()
        assert np.array_equal(plain, native.nn_error_split(up(a), up(b), edges, view=view)["bin"].cpu().numpy())
        assert np.array_equal(plain, want - group * len(edges))
    origin = native.ring_bins(up(a), edges).cpu().numpy()
    assert origin[len(a) - 6:].tolist() == [3, 3, 3, 0, 1, 4]                # exactly on an edge: the upper ring
    assert len(np.unique(origin)) >= 4
    f32 = native.ring_bins(torch.from_numpy(a.astype(np.float32)).to(dev()), edges).cpu().numpy()   # compared in float64
    assert np.array_equal(f32, ref.bins(a.astype(np.float32).astype(np.float64), edges))


# ---------------------------------------------------------------------------------------------------------------------------- refusals
def raw_share(nd, bi, bt, table, total_leaves, n_nodes=None):
    """scp_rate_leaf_share through ctypes with tensors of the test's own making -> (return code, outputs)."""
    from scp_amd import native
    L = native.lib()
    N = int(nd["occ"].shape[0]) if n_nodes is None else n_nodes
    table = np.ascontiguousarray(table, np.int64)
    wsb = int(L.scp_rate_leaf_share_workspace_bytes(int(nd["occ"].shape[0]), len(table)))
    ws = torch.empty(wsb // 8, dtype=torch.int64, device=dev())
    leaves = torch.full((int(nd["occ"].shape[0]),), -7, dtype=torch.int64, device=dev())
    ci = torch.full((max(int(total_leaves), 1),), -7.0, dtype=torch.float64, device=dev())
    ct = torch.full((max(int(total_leaves), 1),), -7.0, dtype=torch.float64, device=dev())
    rc = L.scp_rate_leaf_share(nd["occ"].data_ptr(), nd["level"].data_ptr(), nd["parent"].data_ptr(), N, bi.data_ptr(), bt.data_ptr(), table.ctypes.data,
                               len(table), int(total_leaves), leaves.data_ptr(), ci.data_ptr(), ct.data_ptr(), ws.data_ptr(), wsb,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, leaves, ci, ct


def test_malformed_tables_are_refused_and_nothing_is_written():
    """Host checks refuse without a launch; what only the device can see - a parent outside its segment, a parent behind its child, a
    wrong level, a popcount total that disagrees with the leaf count - is refused by the validation pass before any index is followed:
    SCP_EINVAL, the outputs untouched, and the next well-formed call works."""
    from scp_amd import native
    g = build("skew-then-frame5k")
    nd = g.nodes(("occ", "level", "parent"))
    N, table = g.total_nodes, native.share_table(g.info)
    total = sum(int(i.n_leaves) for i in g.info)
    bi, bt = (up(x) for x in bits_for(g, 3))
    base1 = int(g.info[1].node_base)

    def untouched(out):
        rc, leaves, ci, ct = out
        return rc == -1 and bool((leaves == -7).all()) and bool((ci == -7.0).all()) and bool((ct == -7.0).all())
    good = raw_share(nd, bi, bt, table, total)
    assert good[0] == 0 and int(good[1][0]) == g.info[0].n_leaves and bool((good[2] >= 0).all())
    # the host's checks: tables that do not tile the node table or the leaf table
    for bad in (table[:1], table[::-1], np.array([[0, base1 - 1, 10, 0], list(table[1])]), np.array([list(table[0]), [base1, N - base1, 10, total]])):
        assert untouched(raw_share(nd, bi, bt, bad, total)), bad
    assert untouched(raw_share(nd, bi, bt, table, int(table[1][3])))        # the last segment left without leaves
    assert untouched(raw_share(nd, bi, bt, table, int(table[1][3]) - 1))    # its leaf base past the leaf table
    # the validation pass: one broken entry at a time, in a copy
    def broken(column, index, value):
        cols = {k: v.clone() for k, v in nd.items()}
        cols[column][index] = value
        return cols
    last = N - 1
    occ_last = int(nd["occ"][last].item())
    more = 0xFF if bin(occ_last).count("1") < 8 else 0x7F                  # another popcount on the last level: the leaf total is off by some
    for what, cols in (("a parent past the table", broken("parent", base1 + 5, N + 100)),
                       ("a parent in the segment before", broken("parent", base1 + 5, base1 - 1)),
                       ("a parent behind its child", broken("parent", 5, 900)),
                       ("a negative parent", broken("parent", 7, -1)),
                       ("a root with a parent", broken("parent", base1, 0)),
                       ("a parent on the wrong level", broken("parent", last, base1)),
                       ("a level above the depth", broken("level", 3, 200)),
                       ("a level of 0", broken("level", 3, 0)),
                       ("an occupancy of 0", broken("occ", 3, 0)),
                       ("a leaf total that disagrees with the leaf table", broken("occ", last, more))):
        assert untouched(raw_share(cols, bi, bt, table, total)), what
    with pytest.raises(native.ScpError, match="SCP_EINVAL"):
        native.rate_leaf_share(nd["occ"], nd["level"], broken("parent", base1 + 5, N + 100)["parent"], bi, bt, table, total)
    again = raw_share(nd, bi, bt, table, total)
    assert again[0] == 0 and torch.equal(again[2], good[2]) and torch.equal(again[1], good[1])
    # the Python binding's own refusals
    with pytest.raises(native.ScpError, match="one entry per node"):
        native.rate_leaf_share(nd["occ"], nd["level"], nd["parent"], bi[:-1], bt, table, total)
    with pytest.raises(native.ScpError, match="one entry per node"):
        native.rate_leaf_share(nd["occ"].cpu(), nd["level"], nd["parent"], bi, bt, table, total)
    with pytest.raises(native.ScpError, match=r"int64 \[S,4\]"):
        native.rate_leaf_share(nd["occ"], nd["level"], nd["parent"], bi, bt, table[:, :3], total)
    with pytest.raises(native.ScpError, match="ring edges"):
        native.ring_bins(bi.reshape(-1, 1).expand(-1, 3), [0.0, 8.0, 4.0])
    with pytest.raises(native.ScpError, match="shape"):
        native.ring_bins(bi, [0.0, 8.0])
    with pytest.raises(native.ScpError, match="group values 0 .. 3 outside 0 .. 2"):
        native.ring_bins(torch.zeros((4, 3), device=dev()), [0.0, 8.0], torch.tensor([0, 1, 3, 2], dtype=torch.int32, device=dev()), 3)
    with pytest.raises(native.ScpError, match="bins expected"):
        native.share_segments(bi, bt, torch.zeros(N, dtype=torch.int32, device=dev()), 4097)
    with pytest.raises(native.ScpError, match="device tensor of"):
        native.share_segments(bi.cpu(), bt, torch.zeros(N, dtype=torch.int32, device=dev()), 3)
    with pytest.raises(native.ScpError, match="with n >= 1 expected"):
        native.share_segments(bi, bt[:-1], torch.zeros(N, dtype=torch.int32, device=dev()), 3)


def test_ring_bins_kernel_clamps_a_group_out_of_range():
    """What include/scp.h promises of the C entry point itself (the Python binding refuses such groups before the launch)."""
    from scp_amd import native
    xyz = up([[1.0, 0.0, 0.0], [9.0, 0.0, 0.0], [1.0, 0.0, 0.0], [9.0, 0.0, 0.0]])
    group = up([-1, 3, 1, 0], np.int32)
    bins = torch.empty(4, dtype=torch.int32, device=dev())
    flag = torch.empty(4, dtype=torch.uint8, device=dev())
    view = (C.c_double * 3)(0.0, 0.0, 0.0)
    esq = (C.c_double * 2)(0.0, 25.0)
    rc = native.lib().scp_ring_bins_f64(xyz.data_ptr(), 4, C.cast(view, C.c_void_p), C.cast(esq, C.c_void_p), 2, group.data_ptr(), 3, bins.data_ptr(),
                                        flag.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and bins.cpu().tolist() == [0, 5, 2, 1]
    assert flag.cpu().tolist() == [native.DIST_FLAG_GROUP_CLAMPED, native.DIST_FLAG_GROUP_CLAMPED, 0, 0]


# ----------------------------------------------------------------------------------------------------------------------------- encoder
@functools.lru_cache(maxsize=None)
def ehem_model():
    from cfgs import ehem_cfg
    from scp_amd.models import EHEM
    from scp_amd.weights import fill_weights
    return fill_weights(EHEM(ehem_cfg()), 0).to(dev()).eval()


@pytest.mark.parametrize("level,mullevel", [(12, False), (14, True)], ids=["L12-spher", "L14-multi-level"])
def test_encoder_report_conserves_the_bits_and_leaves_the_stream_alone(level, mullevel):
    from scp_amd import metrics, native
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    xyz = synth_frame(4)[::30].copy()
    P = len(xyz)
    model = ehem_model()
    enc = FrameEncoder(model, "kitti", level, spher=True, mullevel=mullevel, device=dev(), rate=True, rate_rows=True)
    x = torch.from_numpy(xyz).to(dev())
    res = enc.encode(xyz)
    rep = enc.ring_rate(x)
    assert enc.ring_rate(x) == rep                                            # the same from call to call
    assert json.loads(json.dumps(rep)) == rep
    assert sorted(rep) == ["edges", "groups", "rings", "shell_leaves", "total"] and rep["edges"] == list(metrics.default_edges("kitti"))
    shells = 3 if mullevel else 1
    assert len(rep["groups"]) == shells == len(rep["shell_leaves"]) and all(len(g) == len(rep["edges"]) for g in rep["groups"])
    # conservation: the bins hold what the rate report counted
    flat = [e for g in rep["groups"] for e in g]
    rate = res["rate"]
    for name in ("ideal_bits", "table_bits"):
        got = math.fsum(e[name] for e in flat)
        print(level, mullevel, name, got, rate[name], got - rate[name])
        assert abs(got - rate[name]) <= rate_ref.segment_tolerance(res["n_nodes"], rate[name]), name
        assert rep["total"][name] == got
    # the bins are the distortion report's
    drep = enc.distortion_report(x)
    for s in range(shells):
        assert [e["leaves"] for e in rep["groups"][s]] == [e["rows"] for e in drep["b_to_a"]["groups"][s]]
        assert sum(e["leaves"] for e in rep["groups"][s]) == rep["shell_leaves"][s] == drep["shell_leaves"][s]
    assert [e["points"] for e in rep["rings"]] == [e["rows"] for e in drep["a_to_b"]["rings"]] and rep["total"]["points"] == P
    assert enc.ring_rate(x) == rep                                            # the distortion report in between changes nothing
    # every step against the reference: node bits from the rows in coding order, leaf costs, bins, records
    row_ideal, row_table, plan = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in enc._rate_rows)
    nd = {k: v.cpu().numpy() for k, v in enc.geom.nodes(("occ", "level", "parent")).items()}
    ci, ct, row = [], [], 0
    for s, i in enumerate(enc.geom.info):
        sl = slice(int(i.node_base), int(i.node_base + i.n_nodes))
        rows = enc.geom.rows(s)
        parent = np.where(nd["parent"][sl] < 0, -1, nd["parent"][sl].astype(np.int64) - int(i.node_base))
        for out, bits in ((ci, row_ideal), (ct, row_table)):
            node_bits = ref.node_bits(enc.geom.level_counts(s), mullevel, enc.context_size, bits[row:row + rows])
            out.append(ref.leaf_cost(nd["occ"][sl], nd["level"][sl], parent, i.depth, node_bits))
        row += rows
    assert row == len(row_ideal) == res["n_nodes"]
    pts = [p.cpu().numpy() for p in enc._reconstructed()]
    group = np.concatenate([np.full(len(p), s) for s, p in enumerate(pts)])
    want = ref.records(np.concatenate(ci), np.concatenate(ct), ref.bins(np.concatenate(pts), rep["edges"], group, shells), shells * len(rep["edges"]))
    for e, w in zip(flat, want):
        assert e["leaves"] == w["leaves"] and e["max_ideal_bits"] == w["max_ideal_bits"]
        assert abs(e["ideal_bits"] - w["ideal_bits"]) <= 1e-9 * w["ideal_bits"] and abs(e["table_bits"] - w["table_bits"]) <= 1e-9 * w["table_bits"]
    # other edges on request
    two = enc.ring_rate(x, edges=[0.0, 25.0])
    assert two["edges"] == [0.0, 25.0] and two["total"]["leaves"] == rep["total"]["leaves"] and two["total"]["max_ideal_bits"] == rep["total"]["max_ideal_bits"]
    assert two["total"]["ideal_bits"] == pytest.approx(rep["total"]["ideal_bits"], rel=1e-12)
    # the stream: identical after the report, identical to an encoder without the feature, whose rate report is the same too
    assert enc.encode(xyz)["bytes"] == res["bytes"]
    plain = FrameEncoder(model, "kitti", level, spher=True, mullevel=mullevel, device=dev(), rate=True)
    pres = plain.encode(xyz)
    assert pres["bytes"] == res["bytes"] and pres["rate"] == rate
    assert FrameEncoder(model, "kitti", level, spher=True, mullevel=mullevel, device=dev()).encode(xyz)["bytes"] == res["bytes"]
    with pytest.raises(native.ScpError, match="rate=True and rate_rows=True"):
        plain.ring_rate(x)
    # an asynchronous call rebuilds the geometry: no report on a frame whose rows are gone
    enc.finish(enc.encode_async(xyz))
    with pytest.raises(native.ScpError, match="after a synchronous encode"):
        enc.ring_rate(x)


# --------------------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_rate_rings_writes_the_json_and_leaves_every_other_file_alone(tmp_path):
    from scp_amd import native
    from scp_amd.data_preproc import pt as pointCloud
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame, write_kitti_bin
    seq = tmp_path / "seq07"
    seq.mkdir()
    for i in range(2):
        write_kitti_bin(str(seq / f"{i:06d}.bin"), synth_frame(i)[::60])
    runs = {"plain": [], "rings": ["--rate_rings", "0,10,20,40"],
            "all": ["--rate_rings", "0,10,20,40", "--distortion_report", "0,10,20,40", "--rate_report", "--metrics"]}
    outs, lines = {}, {}
    for tag, flags in runs.items():
        out = tmp_path / ("out_" + tag)
        cmd = [sys.executable, os.path.join(ROOT, "encode_mullevel.py"), "--test_files", str(seq / "*.bin"), "--type", "kitti", "--lidar_level", "12",
               "--spher", "--random_weights", "0", "--out_dir", str(out)] + flags
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.count("ideal bits per leaf by ring :") == (2 if "--rate_rings" in flags else 0)
        assert r.stdout.count("bpp ideal / table / coded   :") == (2 if "--rate_report" in flags else 0)
        outs[tag], lines[tag] = out, len(r.stdout.splitlines())
    assert lines["rings"] == lines["plain"] + 2                                                   # one more line per frame
    reports = (".rings.json", ".rate.json", ".dist.json")
    files = {tag: sorted(p.name for p in out.iterdir() if not p.name.endswith(reports)) for tag, out in outs.items()}
    streams = [f for f in files["plain"] if f.endswith(".bin")]
    assert len(streams) == 2 and any(f.endswith(".dat") for f in files["plain"]) and any(f.endswith(".scp.json") for f in files["plain"])
    assert files["rings"] == files["plain"] == files["all"]
    assert not [p for p in outs["rings"].iterdir() if p.name.endswith((".rate.json", ".dist.json"))]    # the flag alone writes no other report
    for tag in ("rings", "all"):
        for f in files["plain"]:
            assert (outs[tag] / f).read_bytes() == (outs["plain"] / f).read_bytes(), (tag, f)
    assert not [p for p in outs["plain"].iterdir() if p.name.endswith(reports)]
    assert len([p for p in outs["all"].iterdir() if p.name.endswith((".rate.json", ".dist.json"))]) == 4
    enc = FrameEncoder(ehem_model(), "kitti", 12, spher=True, mullevel=True, device=dev(), rate=True, rate_rows=True)
    frames = sorted(str(p) for p in seq.iterdir())
    for tag in ("rings", "all"):
        docs = sorted(p for p in outs[tag].iterdir() if p.name.endswith(".rings.json"))
        assert [d.name[:-len(".rings.json")] + ".bin" for d in docs] == streams
        for d, frame in zip(docs, frames):
            doc = json.load(open(d))
            xyz = pointCloud.ptread(frame)
            res = enc.encode(xyz)
            want = enc.ring_rate(torch.from_numpy(np.ascontiguousarray(xyz[:, :3], np.float32)).to(dev()), (0.0, 10.0, 20.0, 40.0))
            assert res["bytes"] == (outs[tag] / (d.name[:-len(".rings.json")] + ".bin")).read_bytes()
            assert {k: doc[k] for k in want} == want
            assert doc["lidar_level"] == 12 and doc["type"] == "kitti" and doc["n_points"] == res["n_points"] and doc["bits"] == res["bits"]
            assert len(doc["groups"]) == 3 and doc["edges"] == [0.0, 10.0, 20.0, 40.0]
