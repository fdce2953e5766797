"""Depth report on the device (csrc/ringrate.hip, scp_amd/native.py, metrics.py, encoder.py, decoder.py, cli.py) against the numpy
statement of its definitions (tests/depth_ref.py), and the decoders' --lod against the encoder's cells.

Bounds.  leaves and every plane of both leaf costs (a fixed sequence of IEEE float64 operations) are exact: equality.  A bin's leaf
count and maximum are exact; its two sums are sums of at most 8192 non-negative terms in a fixed order, held to 1e-9 relative - the
bound test_gpu_distortion.py derives for such sums.  Over a whole frame the bins' sums of plane k are compared with the rate report's
levels <= D - k through rate_ref.segment_tolerance.  Cell origins are integers and the LOD points come from one dequantiser on the same
half-integers: equality.

On the parent commit none of this exists: every test here fails there (no symbols, no method, no flag, no `lod` argument)."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_ref as ref
import rate_ref
import ringrate_ref as rr
from conftest import ROOT
from test_gpu_ringrate import CASES, bits_for, build, check_records, dev, ehem_model, solved, up

pytestmark = pytest.mark.gpu

MAX_DEPTH = 21                                                                # include/scp.h: SCP_MAX_DEPTH
DROPS = (0, 1, 3, MAX_DEPTH)


def run_depth(g, bi, bt, max_drop):
    from scp_amd import native
    nd = g.nodes(("occ", "level", "parent"))
    out = native.rate_depth_share(nd["occ"], nd["level"], nd["parent"], up(bi), up(bt), native.share_table(g.info), sum(int(i.n_leaves) for i in g.info),
                                  max_drop)
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def wanted(case):
    """The reference planes 0 .. SCP_MAX_DEPTH of one case, on the node columns and bits of test_gpu_ringrate.solved - computed once,
    shared, read-only: (ideal [22, leaves], table [22, leaves])."""
    info, nd, (bi, bt), _, _ = solved(case)
    wi, wt = [], []
    for base, n, depth, n_leaves in info:
        sl = slice(base, base + n)
        occ, level = nd["occ"][sl], nd["level"][sl]
        parent = np.where(nd["parent"][sl] < 0, -1, nd["parent"][sl].astype(np.int64) - base)
        wi.append(ref.planes(occ, level, parent, depth, bi[sl], MAX_DEPTH))
        wt.append(ref.planes(occ, level, parent, depth, bt[sl], MAX_DEPTH))
    wi, wt = np.concatenate(wi, axis=1), np.concatenate(wt, axis=1)
    wi.setflags(write=False)
    wt.setflags(write=False)
    return wi, wt


# ------------------------------------------------------------------------------------------------------------ kernels against reference
@pytest.mark.parametrize("case", [c for c in CASES if c != "skew-then-frame5k"])
def test_every_plane_equals_the_reference_and_plane_0_the_rate_per_ring(case):
    info, nd, (bi, bt), share, share_want = solved(case)
    wi, wt = wanted(case)
    total_leaves = sum(n for _, _, _, n in info)
    assert wi.shape == (MAX_DEPTH + 1, total_leaves) and np.array_equal(wi[0], share_want["cost_ideal"])
    g = build(case)
    for max_drop in DROPS:
        got = run_depth(g, bi, bt, max_drop)
        assert got["leaves"].dtype == np.int64 and got["cost_ideal"].dtype == np.float64 and got["cost_table"].dtype == np.float64
        assert got["cost_ideal"].shape == (max_drop + 1, total_leaves) == got["cost_table"].shape
        assert np.array_equal(got["leaves"], share["leaves"]) and np.array_equal(got["leaves"], share_want["leaves"]), (case, max_drop)
        assert np.array_equal(got["cost_ideal"], wi[:max_drop + 1]), (case, max_drop)
        assert np.array_equal(got["cost_table"], wt[:max_drop + 1]), (case, max_drop)
        assert np.array_equal(got["cost_ideal"][0], share["cost_ideal"]) and np.array_equal(got["cost_table"][0], share["cost_table"])
        assert not np.signbit(got["cost_ideal"]).any() and not np.signbit(got["cost_table"]).any()          # +0.0 past the root
    # past a tree's root the planes are 0 for that tree's leaves, and only there (the shares of a root are positive here or the bits 0)
    leaf = 0
    for base, n, depth, n_leaves in info:
        assert (got["cost_ideal"][depth:, leaf:leaf + n_leaves] == 0.0).all() and (got["cost_table"][depth:, leaf:leaf + n_leaves] == 0.0).all()
        assert (got["cost_table"][:depth, leaf:leaf + n_leaves] > 0.0).all()
        kept = bi[base:base + n][nd["level"][base:base + n] <= depth - 1]
        total = math.fsum(kept)
        assert abs(math.fsum(got["cost_ideal"][1, leaf:leaf + n_leaves]) - total) <= rate_ref.segment_tolerance(len(kept), total)
        leaf += n_leaves


def test_a_frame_gives_the_same_planes_alone_and_as_the_second_frame_of_a_build():
    alone, both = solved("frame5k-single-level"), solved("skew-then-frame5k")
    (base, n, depth, n_leaves) = both[0][1]
    assert base > 0 and (n, depth, n_leaves) == alone[0][0][1:]
    bi, bt = alone[2]
    bi2, bt2 = (np.concatenate([x[:base], y]) for x, y in zip(both[2], (bi, bt)))
    first_leaves = both[0][0][3]
    one = run_depth(build("frame5k-single-level"), bi, bt, 3)
    two = run_depth(build("skew-then-frame5k"), bi2, bt2, 3)
    assert two["cost_ideal"].shape == (4, first_leaves + n_leaves)
    assert np.array_equal(two["cost_ideal"][:, first_leaves:], one["cost_ideal"]) and np.array_equal(two["cost_table"][:, first_leaves:], one["cost_table"])
    assert np.array_equal(two["leaves"][base:], one["leaves"])
    assert np.array_equal(two["cost_ideal"][0, :first_leaves], both[3]["cost_ideal"][:first_leaves])    # and the first frame does not care either
    assert np.array_equal(one["cost_ideal"], wanted("frame5k-single-level")[0][:4])


# ---------------------------------------------------------------------------------------------------------------------------- bin sums
def test_bins_of_every_size_sum_per_plane_as_promised_and_plane_0_as_share_segments():
    """Bins of 0, 1, 1023, 1024, 1025 and 2049 rows (around the 1024-row stride), bin ids in arbitrary order, three planes."""
    from scp_amd import native
    sizes = (1025, 0, 1, 2049, 1023, 1024)
    rng = np.random.default_rng(5)
    bins = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    n, K = len(bins), 3
    ci = np.exp2(rng.uniform(-30, 6, (K, n))) * (rng.random((K, n)) > 0.05)
    ct = rng.uniform(0, 20, (K, n))
    seg = native.share_segments_depth(up(ci), up(ct), up(bins, np.int32), len(sizes))
    raw = seg["raw"].cpu().numpy()
    assert raw.shape == (K, len(sizes), 4) and raw.dtype == np.int64
    for k in range(K):
        check_records(raw[k], rr.records(ci[k], ct[k], bins, len(sizes)), f"plane {k}")
        assert [int(v) for v in seg["leaves"][k].cpu()] == list(sizes) and (raw[k, 1] == 0).all()
        single = native.share_segments(up(ci[k]), up(ct[k]), up(bins, np.int32), len(sizes))["raw"].cpu().numpy()
        assert np.array_equal(raw[k], single), k                              # every plane sums as scp_share_segments_f64 does (k = 0: the promise)
    assert seg["leaves"].dtype == torch.int64 and seg["ideal_bits"].dtype == torch.float64 and seg["max_ideal_bits"].shape == (K, len(sizes))
    assert np.array_equal(seg["ideal_bits"].cpu().numpy().view(np.int64), raw[..., 1])
    again = native.share_segments_depth(up(ci), up(ct), up(bins, np.int32), len(sizes))["raw"].cpu().numpy()
    assert np.array_equal(again, raw)                                         # the same bits in every run
    # a plane does not care how many others the launch holds
    assert np.array_equal(native.share_segments_depth(up(ci[:1]), up(ct[:1]), up(bins, np.int32), len(sizes))["raw"].cpu().numpy(), raw[:1])
    # the C entry point with a plane stride above n: the planes as rows of a wider table
    wide_i, wide_t = np.full((K, n + 7), -3.0), np.full((K, n + 7), -3.0)
    wide_i[:, :n], wide_t[:, :n] = ci, ct
    di, dt, db = up(wide_i), up(wide_t), up(bins, np.int32)
    ordered, order = torch.sort(db, stable=True)
    seg_off = torch.searchsorted(ordered, torch.arange(len(sizes) + 1, dtype=torch.int32, device=dev())).to(torch.int64).contiguous()
    out = torch.full((K, len(sizes), 4), -7, dtype=torch.int64, device=dev())
    rc = native.lib().scp_share_segments_depth_f64(di.data_ptr(), dt.data_ptr(), order.data_ptr(), n, seg_off.data_ptr(), len(sizes), K, n + 7, out.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(out.cpu().numpy(), raw)
    with pytest.raises(native.ScpError, match="bins expected"):
        native.share_segments_depth(up(ci), up(ct), up(bins, np.int32), 4097)
    with pytest.raises(native.ScpError, match="device tensor of"):
        native.share_segments_depth(up(ci).cpu(), up(ct), up(bins, np.int32), 3)
    with pytest.raises(native.ScpError, match=r"cost_ideal \[K, n\]"):
        native.share_segments_depth(up(ci)[0], up(ct)[0], up(bins, np.int32), 3)
    with pytest.raises(native.ScpError, match="planes expected"):
        native.share_segments_depth(up(np.zeros((23, 4))), up(np.zeros((23, 4))), up(np.zeros(4), np.int32), 3)


def test_a_bin_of_a_plane_depends_on_its_own_rows_only():
    """Other bins' rows, other planes and the number of bins leave a (plane, bin) record bit-identical."""
    from scp_amd import native
    rng = np.random.default_rng(8)
    n, K = 5000, 2
    ci, ct = rng.uniform(0, 4, (K, n)), rng.uniform(0, 4, (K, n))
    bins = rng.integers(0, 6, n).astype(np.int32)
    base = native.share_segments_depth(up(ci), up(ct), up(bins, np.int32), 6)["raw"].cpu().numpy()
    keep = bins == 2
    cib, ctb, binsb = ci.copy(), ct.copy(), bins.copy()
    cib[:, ~keep] = rng.uniform(0, 9, (K, int((~keep).sum())))
    ctb[:, ~keep] *= 3.0
    binsb[~keep] = rng.integers(3, 40, int((~keep).sum()))                   # other bins, more of them - and none below bin 2 any more
    other = native.share_segments_depth(up(cib), up(ctb), up(binsb, np.int32), 40)["raw"].cpu().numpy()
    assert np.array_equal(other[:, 2], base[:, 2]) and not np.array_equal(other[:, 3], base[:, 3])
    alone = native.share_segments_depth(up(ci[:, keep]), up(ct[:, keep]), up(np.zeros(int(keep.sum())), np.int32), 1)["raw"].cpu().numpy()
    assert np.array_equal(alone[:, 0], base[:, 2])
    swapped = native.share_segments_depth(up(ci[::-1].copy()), up(ct[::-1].copy()), up(bins, np.int32), 6)["raw"].cpu().numpy()
    assert np.array_equal(swapped[::-1], base)                                # a plane's records do not depend on its place


# ---------------------------------------------------------------------------------------------------------------------------- refusals
SENT = -7


def raw_depth(nd, bi, bt, table, total_leaves, max_drop, short_by=0, planes=None):
    """scp_rate_depth_share through ctypes with pre-filled outputs -> (return code, leaves, cost_ideal, cost_table)."""
    from scp_amd import native
    L = native.lib()
    N = int(nd["occ"].shape[0])
    table = np.ascontiguousarray(table, np.int64)
    wsb = int(L.scp_rate_depth_share_workspace_bytes(N, len(table)))
    ws = torch.empty(wsb // 8, dtype=torch.int64, device=dev())
    planes = (max(max_drop, 0) + 1) if planes is None else planes
    leaves = torch.full((N,), SENT, dtype=torch.int64, device=dev())
    ci = torch.full((planes * max(int(total_leaves), 1),), float(SENT), dtype=torch.float64, device=dev())
    ct = torch.full((planes * max(int(total_leaves), 1),), float(SENT), dtype=torch.float64, device=dev())
    rc = L.scp_rate_depth_share(nd["occ"].data_ptr(), nd["level"].data_ptr(), nd["parent"].data_ptr(), N, bi.data_ptr(), bt.data_ptr(), table.ctypes.data,
                                len(table), int(total_leaves), int(max_drop), leaves.data_ptr(), ci.data_ptr(), ct.data_ptr(), ws.data_ptr(), wsb - short_by,
                                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, leaves, ci, ct


def test_malformed_tables_bad_depths_and_short_workspaces_are_refused_and_nothing_is_written():
    """The malformed tables of the rate per ring's test, max_drop = -1 and SCP_MAX_DEPTH + 1 and a workspace one byte short: SCP_EINVAL,
    the pre-filled outputs untouched (the planes were sized for SCP_MAX_DEPTH + 1, so a call that had run would have stayed in
    bounds), and the next well-formed call works."""
    from scp_amd import native
    g = build("skew-then-frame5k")
    nd = g.nodes(("occ", "level", "parent"))
    N, table = g.total_nodes, native.share_table(g.info)
    total = sum(int(i.n_leaves) for i in g.info)
    bi, bt = (up(x) for x in bits_for(g, 3))
    base1 = int(g.info[1].node_base)
    P = MAX_DEPTH + 2                                                         # planes of every output buffer here: room for any max_drop tried

    def untouched(out):
        rc, leaves, ci, ct = out
        return rc == -1 and bool((leaves == SENT).all()) and bool((ci == SENT).all()) and bool((ct == SENT).all())
    good = raw_depth(nd, bi, bt, table, total, 2, planes=P)
    assert good[0] == 0 and int(good[1][0]) == g.info[0].n_leaves and bool((good[2][:3 * total] >= 0).all()) and bool((good[2][3 * total:] == SENT).all())
    assert untouched(raw_depth(nd, bi, bt, table, total, -1, planes=P))
    assert untouched(raw_depth(nd, bi, bt, table, total, MAX_DEPTH + 1, planes=P))
    assert untouched(raw_depth(nd, bi, bt, table, total, 2, short_by=1, planes=P))
    assert raw_depth(nd, bi, bt, table, total, MAX_DEPTH, planes=P)[0] == 0
    # the host's checks: tables that do not tile the node table or the leaf table
    for bad in (table[:1], table[::-1], np.array([[0, base1 - 1, 10, 0], list(table[1])]), np.array([list(table[0]), [base1, N - base1, 10, total]])):
        assert untouched(raw_depth(nd, bi, bt, bad, total, 2, planes=P)), bad
    assert untouched(raw_depth(nd, bi, bt, table, int(table[1][3]), 2, planes=P))       # the last segment left without leaves

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
        assert untouched(raw_depth(cols, bi, bt, table, total, 3, planes=P)), what
    with pytest.raises(native.ScpError, match="SCP_EINVAL"):
        native.rate_depth_share(nd["occ"], nd["level"], broken("parent", base1 + 5, N + 100)["parent"], bi, bt, table, total, 2)
    again = raw_depth(nd, bi, bt, table, total, 2, planes=P)
    assert again[0] == 0 and torch.equal(again[2], good[2]) and torch.equal(again[1], good[1]) and torch.equal(again[3], good[3])
    # the Python binding's own refusals
    with pytest.raises(native.ScpError, match="one entry per node"):
        native.rate_depth_share(nd["occ"], nd["level"], nd["parent"], bi[:-1], bt, table, total, 2)
    with pytest.raises(native.ScpError, match=r"int64 \[S,4\]"):
        native.rate_depth_share(nd["occ"], nd["level"], nd["parent"], bi, bt, table[:, :3], total, 2)
    for bad in (-1, MAX_DEPTH + 1):
        with pytest.raises(native.ScpError, match="max_drop"):
            native.rate_depth_share(nd["occ"], nd["level"], nd["parent"], bi, bt, table, total, bad)


# ----------------------------------------------------------------------------------------------------------------- encoder and decoder
FRAMES = {"L12-spher": (12, False), "L14-multi-level": (14, True)}


@functools.lru_cache(maxsize=None)
def encoded(tag):
    """One frame encoded once with the feature: (encoder, input cloud, device cloud, result, depth report with max_drop = 3, the LOD
    cells per k and shell as host int64 arrays, shell depths) - shared by the encoder and the decoder tests, read-only."""
    from scp_amd.encoder import FrameEncoder
    from scp_amd.synth import synth_frame
    level, mullevel = FRAMES[tag]
    xyz = synth_frame(4)[::30].copy()
    enc = FrameEncoder(ehem_model(), "kitti", level, spher=True, mullevel=mullevel, device=dev(), rate=True, rate_rows=True)
    x = torch.from_numpy(xyz).to(dev())
    res = enc.encode(xyz)
    rep = enc.depth_report(x, max_drop=3)
    cells = {k: [c.cpu().numpy().astype(np.int64) for c in enc.lod_cells(k)] for k in range(4)}
    return enc, xyz, x, res, rep, cells, [int(i.depth) for i in enc.geom.info]


@pytest.mark.parametrize("tag", list(FRAMES))
def test_encoder_report_joins_the_siblings_at_k_0_and_conserves_the_bits_of_every_depth(tag):
    from scp_amd import metrics, native
    from scp_amd.encoder import FrameEncoder
    level, mullevel = FRAMES[tag]
    enc, xyz, x, res, rep, cells, depths = encoded(tag)
    shells = 3 if mullevel else 1
    assert enc.encode(xyz)["bytes"] == res["bytes"]                           # (the shared encoder holds this frame again, whatever ran in between)
    assert enc.depth_report(x, max_drop=3) == rep                             # the same from call to call
    assert json.loads(json.dumps(rep)) == rep
    assert sorted(rep) == ["edges", "levels", "shell_depths", "shell_leaves"] and rep["edges"] == list(metrics.default_edges("kitti"))
    assert rep["shell_depths"] == depths and len(depths) == shells and len(rep["levels"]) == 4 and [lv["drop"] for lv in rep["levels"]] == [0, 1, 2, 3]
    # k = 0 is the three sibling reports
    ring, drep, dist = enc.ring_rate(x), enc.distortion_report(x), enc.distortion(x)
    first = rep["levels"][0]
    assert {k: first["rate"][k] for k in first["rate"] if k in ring} == {k: ring[k] for k in ring if k in first["rate"]}
    assert sorted(set(first["rate"]) & set(ring)) == ["edges", "groups", "rings", "total"]
    assert {k: first["distortion"][k] for k in first["distortion"] if k in drep} == {k: drep[k] for k in drep if k in first["distortion"]}
    assert sorted(set(first["distortion"]) & set(drep)) == ["a_to_b", "b_to_a", "edges"]
    assert first["d1"]["psnr"] == dist["psnr"] and first["d1"] == {k: dist[k] for k in first["d1"]}
    assert first["cells"] == rep["shell_leaves"] == ring["shell_leaves"]
    # conservation per depth: plane k holds what the rate report counted on levels <= D_s - k of every shell
    rate = res["rate"]
    assert len(rate["levels"]) == sum(depths)
    for k, lv in enumerate(rep["levels"]):
        kept, off = [], 0
        for d in depths:
            kept += rate["levels"][off:off + d - k]
            off += d
        flat = [e for g in lv["rate"]["groups"] for e in g]
        for name in ("ideal_bits", "table_bits"):
            got, want = math.fsum(e[name] for e in flat), math.fsum(e[name] for e in kept)
            print(tag, k, name, got, want, got - want)
            assert abs(got - want) <= rate_ref.segment_tolerance(sum(e["nodes"] for e in kept), want), (k, name)
            assert lv["rate"]["total"][name] == got
        assert [e["leaves"] for e in flat] == [e["leaves"] for g in first["rate"]["groups"] for e in g]       # the bins are those of the finest leaves
        assert lv["cells"] == [len(c) for c in cells[k]]
        assert [sum(e["rows"] for e in g) for g in lv["distortion"]["b_to_a"]["groups"]] == lv["cells"]
        assert lv["distortion"]["a_to_b"]["total"]["rows"] == len(xyz)
    # bits and cells do not grow with k; the error of these frames does
    for a, b in zip(rep["levels"], rep["levels"][1:]):
        assert b["rate"]["total"]["ideal_bits"] <= a["rate"]["total"]["ideal_bits"] and b["rate"]["total"]["table_bits"] <= a["rate"]["total"]["table_bits"]
        assert all(cb <= ca for ca, cb in zip(a["cells"], b["cells"]))
        for ga, gb in zip(a["rate"]["groups"], b["rate"]["groups"]):
            assert all(eb["ideal_bits"] <= ea["ideal_bits"] for ea, eb in zip(ga, gb))
    print(tag, "bpp ideal and D1 PSNR per k:", [(lv["rate"]["total"]["ideal_bits_per_point"], lv["d1"]["psnr"]) for lv in rep["levels"]])
    # the cells against the reference: (leaf >> k) << k of the shell's leaves, in their order
    for k in range(4):
        for s in range(shells):
            want, _ = ref.cell_origins(enc.geom.leaves(s).cpu().numpy(), k)
            assert np.array_equal(cells[k][s], want), (k, s)
    # the LOD points are the encoder's dequantiser on the centres
    pts1 = torch.cat([metrics.dequantize(metrics.lod_centres(torch.from_numpy(c).to(dev()), 1), i.qs, i.offset, spher=True, f32=not mullevel).double()
                      for c, i in zip(cells[1], enc._infos)])
    assert metrics.chamfer_psnr(x, pts1, metrics.PEAK["kitti"]) == rep["levels"][1]["d1"]
    # other depths and edges on request
    two = enc.depth_report(x, max_drop=1, edges=[0.0, 25.0])
    assert two["edges"] == [0.0, 25.0] and len(two["levels"]) == 2 and two["levels"][1]["cells"] == rep["levels"][1]["cells"]
    assert two["levels"][1]["d1"] == rep["levels"][1]["d1"]
    assert two["levels"][1]["rate"]["total"]["ideal_bits"] == pytest.approx(rep["levels"][1]["rate"]["total"]["ideal_bits"], rel=1e-12)
    assert enc.depth_report(x, max_drop=0)["levels"][0] == first
    # the stream: identical after the report and identical to an encoder without the feature
    assert enc.encode(xyz)["bytes"] == res["bytes"]
    plain = FrameEncoder(ehem_model(), "kitti", level, spher=True, mullevel=mullevel, device=dev())
    assert plain.encode(xyz)["bytes"] == res["bytes"]
    # refusals: no rows, max_drop too large, an asynchronous call
    with pytest.raises(native.ScpError, match="rate=True and rate_rows=True"):
        plain.depth_report(x)
    for bad in (min(depths), -1, 1.5):
        with pytest.raises(native.ScpError, match=rf"max_drop .* outside 0 \.\. {min(depths) - 1}"):
            enc.depth_report(x, max_drop=bad)
    assert len(enc.depth_report(x, max_drop=min(depths) - 1)["levels"]) == min(depths)          # down to the root level
    enc.finish(enc.encode_async(xyz))
    with pytest.raises(native.ScpError, match="after a synchronous encode"):
        enc.depth_report(x)
    assert enc.encode(xyz)["bytes"] == res["bytes"]                           # (the shared encoder holds its frame again)


def write_stream(enc, res, stem):
    from scp_amd.decoder import write_sidecar
    out = enc.outfile(stem, res)
    with open(out, "wb") as f:
        f.write(res["bytes"])
    torch.save(torch.Tensor(res["pos_mm"].astype(np.float32)), out + ".dat")
    write_sidecar(out, enc, res, "EHEM")
    return out


@pytest.mark.parametrize("tag", list(FRAMES))
def test_decoder_lod_stops_early_and_returns_the_encoders_cells(tag, tmp_path):
    from scp_amd import metrics, native
    from scp_amd.decoder import _ehem_job, decode_file, dequantise_leaves
    level, mullevel = FRAMES[tag]
    enc, xyz, x, res, rep, cells, depths = encoded(tag)
    out = write_stream(enc, res, str(tmp_path / "f"))
    model = ehem_model()
    today = decode_file(out, model, mullevel=mullevel, device=dev())
    zero = decode_file(out, model, mullevel=mullevel, device=dev(), lod=0)
    assert sorted(zero) == sorted(today) and "lod" not in zero
    assert all(torch.equal(a, b) for a, b in zip(zero["codes"], today["codes"])) and all(torch.equal(a, b) for a, b in zip(zero["leaves"], today["leaves"]))
    assert torch.equal(zero["points"], today["points"]) and len(zero["codes"]) == len(depths)
    job = _ehem_job(out, mullevel=mullevel)
    for k in (1, 3):
        got = decode_file(out, model, mullevel=mullevel, device=dev(), lod=k)
        assert got["lod"] == k and len(got["cells"]) == len(depths)
        for s, c in enumerate(got["cells"]):
            assert c.dtype == torch.int64 and np.array_equal(c.cpu().numpy(), cells[k][s]), (k, s)       # integer for integer, per shell
        assert [int(c.shape[0]) for c in got["cells"]] == rep["levels"][k]["cells"]
        want = torch.cat([dequantise_leaves(metrics.lod_centres(c, k), q, b, job["z_offset"], job["spher"], job["cylin"], job["data_type"])
                          for c, q, b in zip(got["cells"], job["qs"], job["bins"])])
        assert got["points"].dtype == torch.float64 and torch.equal(got["points"], want)
        assert got["levels_decoded"] == sum(depths) - k                       # every shell in full but the last, which stops after D - k
        if not mullevel:
            assert got["levels_decoded"] == depths[0] - k and got["leaves"] == [None]
        # the decoded levels are today's, the stopped shell holds fewer codes, the shells before it all of theirs and their leaves
        for s, (c, full) in enumerate(zip(got["codes"], today["codes"])):
            assert torch.equal(c, full[:len(c)]) and (len(c) < len(full)) == (s == len(depths) - 1)
        for a, b in zip(got["leaves"][:-1], today["leaves"][:-1]):
            assert torch.equal(a, b)
        assert got["leaves"][-1] is None
    for bad in (min(depths), -1):
        with pytest.raises(native.ScpError, match=rf"lod .* outside 0 \.\. {min(depths) - 1}"):
            decode_file(out, model, mullevel=mullevel, device=dev(), lod=bad)


# --------------------------------------------------------------------------------------------------------------------------------- CLI
REPORTS = (".depth.json", ".rings.json", ".rate.json", ".dist.json")


def two_frames(tmp_path):
    from scp_amd.synth import synth_frame, write_kitti_bin
    seq = tmp_path / "seq07"
    seq.mkdir()
    for i in range(2):
        write_kitti_bin(str(seq / f"{i:06d}.bin"), synth_frame(i)[::60])
    return seq


def run_encode(tmp_path, seq, tag, flags):
    """encode.py on the two frames in a process of its own -> (output directory, stdout)."""
    out = tmp_path / ("out_" + tag)
    cmd = [sys.executable, os.path.join(ROOT, "encode.py"), "--test_files", str(seq / "*.bin"), "--type", "kitti", "--lidar_level", "12",
           "--spher", "--random_weights", "0", "--out_dir", str(out)] + flags
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("depth k: ideal bpp, D1 PSNR :") == (2 if "--depth_report" in flags else 0)
    return out, r.stdout


def check_docs_against_the_api(out, seq, streams, drop, edges):
    """Every <stream>.depth.json of `out` holds the figures FrameEncoder.depth_report gives for its frame -> the loaded documents."""
    from scp_amd.data_preproc import pt as pointCloud
    from scp_amd.encoder import FrameEncoder
    enc = FrameEncoder(ehem_model(), "kitti", 12, spher=True, device=dev(), rate=True, rate_rows=True)
    docs = sorted(p for p in out.iterdir() if p.name.endswith(".depth.json"))
    assert [d.name[:-len(".depth.json")] + ".bin" for d in docs] == streams
    loaded = []
    for d, frame in zip(docs, sorted(str(p) for p in seq.iterdir())):
        doc = json.load(open(d))
        xyz = pointCloud.ptread(frame)
        res = enc.encode(xyz)
        want = enc.depth_report(torch.from_numpy(np.ascontiguousarray(xyz[:, :3], np.float32)).to(dev()), drop, edges)
        assert res["bytes"] == (out / (d.name[:-len(".depth.json")] + ".bin")).read_bytes()
        assert {k: doc[k] for k in want} == want
        assert doc["lidar_level"] == 12 and doc["type"] == "kitti" and doc["n_points"] == res["n_points"] and doc["bits"] == res["bits"]
        assert len(doc["levels"]) == drop + 1 and len(doc["shell_depths"]) == 1
        loaded.append(doc)
    return loaded


def test_cli_depth_report_writes_the_json_leaves_the_streams_alone_and_the_decoder_previews_it(tmp_path):
    from scp_amd import native
    from scp_amd.cli import decode_main
    from scp_amd.data_preproc import pt as pointCloud
    seq = two_frames(tmp_path)
    plain, plain_out = run_encode(tmp_path, seq, "plain", [])
    depth, depth_out = run_encode(tmp_path, seq, "depth", ["--depth_report", "2"])
    assert len(depth_out.splitlines()) == len(plain_out.splitlines()) + 2                         # one more line per frame
    files = {tag: sorted(p.name for p in out.iterdir() if not p.name.endswith(REPORTS)) for tag, out in (("plain", plain), ("depth", depth))}
    streams = [f for f in files["plain"] if f.endswith(".bin")]
    assert len(streams) == 2 and any(f.endswith(".dat") for f in files["plain"]) and any(f.endswith(".scp.json") for f in files["plain"])
    assert files["depth"] == files["plain"]
    assert not [p for p in depth.iterdir() if p.name.endswith(REPORTS[1:])]                       # the flag alone writes no other report
    assert not [p for p in plain.iterdir() if p.name.endswith(REPORTS)]
    for f in files["plain"]:
        assert (depth / f).read_bytes() == (plain / f).read_bytes(), f
    docs = check_docs_against_the_api(depth, seq, streams, 2, None)
    # the decoder's preview: as many vertices as the report counts cells at k = 1
    dec = ["--test_files", str(seq), "--random_weights", "0", "--out_dir", str(depth)]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "decode_ehem.py")] + dec + ["--lod", "1"], capture_output=True, text=True, cwd=str(tmp_path),
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    plys = sorted(p for p in depth.iterdir() if p.name.endswith(".ply"))
    assert len(plys) == 2
    for ply, doc in zip(plys, docs):
        assert len(pointCloud.ptread(str(ply))) == sum(doc["levels"][1]["cells"]), ply
    with pytest.raises(native.ScpError, match="--lod with --streams above 1"):                    # (refused before anything is decoded: no process needed)
        decode_main(dec + ["--lod", "1", "--streams", "2"])


def test_cli_depth_report_next_to_its_siblings_leaves_their_files_alone(tmp_path):
    seq = two_frames(tmp_path)
    others = ["--rate_rings", "0,10,20,40", "--distortion_report", "0,10,20,40", "--rate_report", "--metrics"]
    sib, sib_out = run_encode(tmp_path, seq, "siblings", others)
    both, both_out = run_encode(tmp_path, seq, "all", ["--depth_report", "2:0,10,20,40"] + others)
    assert len(both_out.splitlines()) == len(sib_out.splitlines()) + 2 and both_out.count("ideal bits per leaf by ring :") == 2
    names = sorted(p.name for p in sib.iterdir())
    assert names == sorted(p.name for p in both.iterdir() if not p.name.endswith(".depth.json"))
    assert len([n for n in names if n.endswith(REPORTS[1:])]) == 6
    for f in names:                                                                               # streams, .dat, sidecars and the three other reports
        assert (sib / f).read_bytes() == (both / f).read_bytes(), f
    docs = check_docs_against_the_api(both, seq, [n for n in names if n.endswith(".bin")], 2, (0.0, 10.0, 20.0, 40.0))
    assert all(doc["edges"] == [0.0, 10.0, 20.0, 40.0] for doc in docs)
