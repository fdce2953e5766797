#!/usr/bin/env python3
"""Cost of the rate per ring (csrc/ringrate.hip) on full frames: synth_frame(0) at level 12 --spher and as the level-16 multi-level workload.

Per workload the frame is encoded once (synchronously, rate=True, rate_rows=True); then every launch group of FrameEncoder.ring_rate is
timed on its own with device events over --reps calls after a warm-up - microseconds per call:
    node_bits       coding order -> node plumbing (torch index kernels)
    leaf_share      scp_rate_leaf_share: validation, leaves bottom-up, costs top-down (2 * depth + 1 kernels, one small read-back)
    ring_bins       scp_ring_bins_f64 on the reconstructed cloud (and on the input cloud: ring_bins_points)
    share_segments  the stable sort of the bins (torch) + scp_share_segments_f64
    ring_rate       the whole method, read-backs and host work included (wall clock as well)
next to scp_softmax_cdf and scp_rate_segments on the same frame's table in the same run - the yardsticks.  Also the number of kernels
scp_rate_leaf_share launches.  Writes one JSON document (--out, by default profiles/rate_rings.json).  A measurement tool, not a product path.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def device_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def workload(model, dev, level, mullevel, args):
    from scp_amd import native
    from scp_amd.encoder import FrameEncoder, _rate_layout
    from scp_amd.synth import synth_frame
    xyz = synth_frame(0)
    x = torch.from_numpy(xyz).to(dev)
    enc = FrameEncoder(model, "kitti", level, spher=True, mullevel=mullevel, device=dev, rate=True, rate_rows=True)
    res = enc.encode(xyz)
    table, sym = res["_debug"]["table"], res["_debug"]["sym_coded"]
    lohi = native.softmax_cdf(table, sym)["lohi"]
    row_ideal, row_table, plan = enc._rate_rows
    off, _ = _rate_layout(plan.level_sizes, enc.context_size)
    seg_off = torch.tensor(off, dtype=torch.int64, device=dev)
    g = enc.geom
    edges = native.dist_edges([0.0, 5.0, 10.0, 15.0, 20.0, 30.0, 40.0, 60.0, 80.0])
    nd = g.nodes(("occ", "level", "parent"))
    node_of_row = torch.cat([torch.arange(int(i.node_base), int(i.node_base) + g.rows(s), device=dev) for s, i in enumerate(g.info)])
    order = plan.coding_order_device(dev)
    table_segs, total_leaves = native.share_table(g.info), sum(int(i.n_leaves) for i in g.info)
    bi, bt = native.node_bits(order, node_of_row, row_ideal, row_table, g.total_nodes)
    share = native.rate_leaf_share(nd["occ"], nd["level"], nd["parent"], bi, bt, table_segs, total_leaves)
    pts = enc._reconstructed()
    quant = torch.cat(pts)
    group = torch.cat([torch.full((p.shape[0],), k, dtype=torch.int32, device=dev) for k, p in enumerate(pts)])
    bins = native.ring_bins(quant, edges, group, len(pts))
    xd = x[:, :3].double().contiguous()
    t = dict(
        cdf_us=device_us(lambda: native.softmax_cdf(table, sym), args.reps),
        rate_us=device_us(lambda: native.rate_segments(table, sym, lohi, seg_off), args.reps),
        rate_with_rows_us=device_us(lambda: native.rate_segments(table, sym, lohi, seg_off, want_rows=True), args.reps),
        node_bits_us=device_us(lambda: native.node_bits(order, node_of_row, row_ideal, row_table, g.total_nodes), args.reps),
        leaf_share_us=device_us(lambda: native.rate_leaf_share(nd["occ"], nd["level"], nd["parent"], bi, bt, table_segs, total_leaves), args.reps),
        ring_bins_us=device_us(lambda: native.ring_bins(quant, edges, group, len(pts)), args.reps),
        ring_bins_points_us=device_us(lambda: native.ring_bins(xd, edges), args.reps),
        share_segments_us=device_us(lambda: native.share_segments(share["cost_ideal"], share["cost_table"], bins, len(pts) * len(edges)), args.reps),
        ring_rate_us=device_us(lambda: enc.ring_rate(x, edges), args.reps))
    wall = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = enc.ring_rate(x, edges)
        wall.append((time.perf_counter() - t0) * 1e3)
    depth = max(int(i.depth) for i in g.info)
    rate = res["rate"]
    return dict(level=level, mullevel=mullevel, points=int(x.shape[0]), nodes=int(g.total_nodes), leaves=total_leaves, segments=len(g.info),
                deepest_tree=depth, leaf_share_kernels=2 * depth + 1, ring_rate_wall_ms=wall, **t,
                report=dict(ideal_bits=rate["ideal_bits"], ring_ideal_bits=rep["total"]["ideal_bits"], table_bits=rate["table_bits"],
                            ring_table_bits=rep["total"]["table_bits"],
                            rings=[dict(leaves=e["leaves"], points=e["points"], ideal_bits_per_leaf=e["ideal_bits_per_leaf"]) for e in rep["rings"]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_rings.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from cfgs import ehem_cfg
    from scp_amd import native
    from scp_amd.models import EHEM
    from scp_amd.weights import fill_weights
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    native.lib()
    dev = torch.device("cuda:0")
    model = fill_weights(EHEM(ehem_cfg()), 0).to(dev).eval()
    res = dict(frame="synth_frame(0)", weights="fill_weights seed 0", reps=args.reps, device=torch.cuda.get_device_name(0),
               workloads=dict(L12_spher=workload(model, dev, 12, False, args), L16_mullevel_spher=workload(model, dev, 16, True, args)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
