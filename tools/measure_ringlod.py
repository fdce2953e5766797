#!/usr/bin/env python3
"""Cost and effect of ring LOD (csrc/ringlod.hip) on full frames: synth_frame(0) at level 12 --spher and as the level-16 multi-level
workload, RANDOM weights.

Per workload the frame is encoded once with the rate kernels and its depth report taken (max_drop 3, edges 0,10,25,50).  From that
report ONE table is read: per ring the largest k <= 3 whose D1 error of the ring (original points against the LOD-k cloud) stays within
6 dB - four times the mean squared error, one octree level - of the error the worst ring has at k = 0.  The frame is then encoded again with
that table.  Recorded: coded, coded-table and ideal bits and the D1 PSNR, plain and ring-LOD, next to what the depth report predicted
for the table (per ring its plane k_r: ideal bits; the report has no plane for a mixed table's D1).  Timed with device events over
--reps calls after a warm-up, in microseconds per call: scp_ringlod_cells as the snap (all points of all shells) and as the implied
mask (all nodes of all shells, per-node start sizes), scp_force_rows on the coding-order table, and scp_softmax_cdf from the same run.
Random weights say nothing about a trained model: the figures show the mechanism at work, not what the option buys on a checkpoint.
Writes one JSON document (--out, by default profiles/ringlod.json).  A measurement tool, not a product path.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EDGES = (0.0, 10.0, 25.0, 50.0)
MAX_DROP = 3
BUDGET = 4.0            # a ring's mean squared error may grow to this many times the worst ring's at k = 0: one octree level, 6 dB


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


def table_from(rep):
    """Per ring the largest k whose ring error stays within BUDGET (6 dB) of the worst ring's error at k = 0."""
    rings = [lv["distortion"]["a_to_b"]["rings"] for lv in rep["levels"]]
    accept = BUDGET * max([e["mse"] for e in rings[0] if e["rows"]] or [0.0])
    drops = []
    for r in range(len(EDGES)):
        ok = [k for k in range(len(rings)) if rings[k][r]["rows"] == 0 or rings[k][r]["mse"] <= accept]
        drops.append(max(ok) if ok else 0)
    return drops


def bits_of(res, dist):
    return dict(coded_bits=res["bits"], table_bits=res["rate"]["table_bits"], ideal_bits=res["rate"]["ideal_bits"], bpp=res["bpp"],
                n_points=res["n_points"], n_nodes=res["n_nodes"], psnr_d1=dist["psnr"], chamfer=dist["chamfer"])


def workload(model, dev, level, mullevel, args):
    from scp_amd import native
    from scp_amd.encoder import EncodePlan, FrameEncoder
    from scp_amd.synth import synth_frame
    frame = synth_frame(0)
    x = torch.from_numpy(frame).to(dev)
    kw = dict(spher=True, mullevel=mullevel, device=dev)
    plain = FrameEncoder(model, "kitti", level, rate=True, rate_rows=True, **kw)
    pres = plain.encode(frame)
    rep = plain.depth_report(x, MAX_DROP, EDGES)
    pdist = plain.distortion(x)
    drops = table_from(rep)
    predicted = sum(rep["levels"][k]["rate"]["rings"][r]["ideal_bits"] for r, k in enumerate(drops))
    out = dict(level=level, mullevel=mullevel, edges=list(EDGES), drops=drops, plain=bits_of(pres, pdist),
               depth_report=[dict(drop=lv["drop"], ideal_bits=lv["rate"]["total"]["ideal_bits"], psnr_d1=lv["d1"]["psnr"]) for lv in rep["levels"]],
               predicted_ideal_bits=predicted)
    if not any(drops):
        out["note"] = "the rule drops nothing on this frame: no ring-LOD encode"
        return out
    enc = FrameEncoder(model, "kitti", level, rate=True, ring_lod=(EDGES, drops), **kw)
    res = enc.encode(frame)
    out["ring_lod"] = dict(bits_of(res, enc.distortion(x)), **{k: res["ring_lod"][k] for k in ("snapped", "implied_rows", "leaves", "thresholds")})
    out["ideal_bits_measured_over_predicted"] = res["rate"]["ideal_bits"] / predicted if predicted else None
    # the two entry points, on this frame's own arrays
    qs, _, _ = enc.quantize(x)
    q = torch.cat(qs).contiguous()
    thr, cuts = res["ring_lod"]["thresholds"], [0]
    for c in qs:
        cuts.append(cuts[-1] + int(c.shape[0]))
    segs = [(a, b - a, 0, k) for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
    snap_us = device_us(lambda: native.ringlod_cells(q, thr, drops, segs=segs, snapped=True), args.reps)
    pre = enc.preprocess(x)
    nd = enc.geom.nodes(("level", "pos"))
    nsegs = [(int(i.node_base), int(i.n_nodes), int(i.depth), s) for s, i in enumerate(enc.geom.info)]
    mask_us = device_us(lambda: native.ringlod_cells(nd["pos"], thr, drops, level=nd["level"], segs=nsegs), args.reps)
    plan = EncodePlan(pre["level_sizes"], enc.context_size)
    table = enc.logits_in_coding_order(pre, plan)
    sym = enc._sym_coded(pre, plan)
    mask = pre["ring"]["mask_rows"][plan.coding_order_device(dev)].contiguous()
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    force_us = device_us(lambda: native.force_rows(table, mask, sym, counter), args.reps)
    cdf_us = device_us(lambda: native.softmax_cdf(table, sym), args.reps)
    out.update(points=int(q.shape[0]), nodes=int(nd["pos"].shape[0]), rows=int(table.shape[0]), table_row_stride=int(table.stride(0)),
               cells_snap_us=snap_us, cells_mask_us=mask_us, force_rows_us=force_us, cdf_us=cdf_us)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ringlod.json"))
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
               note="RANDOM weights: recorded values, not targets - they show the mechanism at work and say nothing about a trained model; "
                    "what the option saves on a trained checkpoint has not been measured",
               workloads=dict(L12_spher=workload(model, dev, 12, False, args), L16_mullevel_spher=workload(model, dev, 16, True, args)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
